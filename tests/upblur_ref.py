"""Float64 restatement of an up-sampling StyledConv as the kernels factor it (shared weight, per-sample in / out scales):

    out = lrelu(blur(conv_transpose2d(x * s, W, stride 2) * d) + nw * noise + bias, 0.2) * sqrt(2)

with blur = the 4x4 FIR on the (2H+1)x(2W+1) image padded by one zero on every side (Blur(pad=(1,1)) of the reference's
ModulatedConv2d).  tests/test_upblur_ref_host.py holds it to the oracle's styled_conv; tests/test_gpu_upblur.py holds the HIP
kernels to it."""
import torch
import torch.nn.functional as F

SQRT2 = 2 ** 0.5


def blur_pad1(t, kernel):
    """True 2-D convolution of [B,C,h,w] with a [4,4] kernel after one zero on every side: [B,C,h-1,w-1]."""
    c = t.shape[1]
    wk = torch.flip(kernel.to(t.dtype), (0, 1)).reshape(1, 1, 4, 4).expand(c, 1, 4, 4)
    return F.conv2d(F.pad(t, (1, 1, 1, 1)), wk, groups=c)


def upblur_ref(x, wt, s, d, kernel, noise=None, nw=None, bias=None):
    """x [B,K,H,W]; wt [N,K,3,3] (the forward weight as [out,in], already scaled); s [B,K]; d [B,N] or None; kernel [4,4];
    noise [1,1,2H,2W], nw [1], bias [N] or None.  -> (ref, scale) in float64, [B,N,2H,2W]: the result and the sum of the
    magnitudes of the terms of every output (the same arithmetic on absolute values), the yardstick of a per-plane error."""
    xd = x.double().cpu() * s.double().cpu()[:, :, None, None]
    wd = wt.double().cpu().permute(1, 0, 2, 3)  # conv_transpose2d wants [in, out, k, k]
    kd = kernel.double().cpu()
    dd = d.double().cpu()[:, :, None, None] if d is not None else 1.0
    t = F.conv_transpose2d(xd, wd, stride=2) * dd
    at = F.conv_transpose2d(xd.abs(), wd.abs(), stride=2) * (dd.abs() if d is not None else 1.0)
    pre, scale = blur_pad1(t, kd), blur_pad1(at, kd.abs())
    if noise is not None:
        nz = nw.double().cpu() * noise.double().cpu()
        pre, scale = pre + nz, scale + nz.abs()
    if bias is not None:
        bd = bias.double().cpu()[None, :, None, None]
        pre, scale = pre + bd, scale + bd.abs()
    return F.leaky_relu(pre, 0.2) * SQRT2, scale * SQRT2
