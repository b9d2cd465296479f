"""Float64 restatement of w2e_modconv_down_rgbfold (include/w2e.h K1f): the stride-2 input-gradient conv of an up-sampling
StyledConv with, in its epilogue, the ToRGB backward of the level it writes and the activation backward of the StyledConv below
that ToRGB node.  Written from the definitions with torch's float64 convolutions; tests/test_rgbfold_ref_host.py holds it to
autograd through the forward composition, tests/test_gpu_rgbfold.py holds the HIP kernels to it."""
import torch
import torch.nn.functional as F


def rgb_weight(wrgb, style):
    """w[b,c,o]: wrgb [3,n] * style [b,n] (the shared-weight form), or wrgb [b,3,n] itself (style None)."""
    w = wrgb.double().cpu()
    return w[None] * style.double().cpu()[:, None, :] if style is not None else w


def rgbfold_ref(g, wt, s_in, s_out, x, gy, wrgb, style, noise, slope=0.2, gain=2 ** 0.5):
    """g [B,K,2h+1,2w+1]; wt [N,K,3,3]; s_in [B,K]; s_out [B,N]; x [B,N,h,w] (the ACTIVATED output of the StyledConv below);
    gy [B,3,h,w]; wrgb / style: see rgb_weight; noise [h*w] (any shape with h*w elements) or None.
    -> dict of (value, scale) pairs in float64, `scale` = the same sum over the magnitudes of its terms:
       gpre [B,N,h,w], dot [B,N], sums3 [B,N,3], gw ([B,N] with style, else [B,3,N])."""
    gd = g.double().cpu() * s_in.double().cpu()[:, :, None, None]
    wd = wt.double().cpu()
    so = s_out.double().cpu()[:, :, None, None]
    xd, gyd = x.double().cpu(), gy.double().cpu()
    raw, absraw = F.conv2d(gd, wd, stride=2), F.conv2d(gd.abs(), wd.abs(), stride=2)
    w = rgb_weight(wrgb, style)
    v = raw * so + torch.einsum("bco,bchw->bohw", w, gyd)
    av = absraw * so.abs() + torch.einsum("bco,bchw->bohw", w.abs(), gyd.abs())
    pos = xd > 0
    fac = torch.where(pos, torch.full_like(xd, gain), torch.full_like(xd, gain * slope))
    gpre, agpre = v * fac, av * fac
    pre = xd / fac  # the pre-activation: x = lrelu(pre) * gain
    nz = noise.double().cpu().reshape(1, 1, *xd.shape[2:]) if noise is not None else torch.zeros(1, 1, *xd.shape[2:], dtype=torch.float64)
    sums3 = torch.stack([(gpre * pre).sum((2, 3)), (gpre * nz).sum((2, 3)), gpre.sum((2, 3))], -1)
    asums3 = torch.stack([(agpre * pre.abs()).sum((2, 3)), (agpre * nz.abs()).sum((2, 3)), agpre.sum((2, 3))], -1)
    u, au = torch.einsum("bohw,bchw->bco", xd, gyd), torch.einsum("bohw,bchw->bco", xd.abs(), gyd.abs())
    if style is not None:
        wsc = wrgb.double().cpu()
        gw, agw = (wsc[None] * u).sum(1), (wsc.abs()[None] * au).sum(1)
    else:
        gw, agw = u, au
    return {"gpre": (gpre, agpre), "dot": ((raw * xd).sum((2, 3)), (absraw * xd.abs()).sum((2, 3))), "sums3": (sums3, asums3),
            "gw": (gw, agw)}
