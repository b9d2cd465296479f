"""float64 restatement, on the CPU and in stock torch ops, of the generator's small kernels: the ToRGB entry points of csrc/torgb.hip
and w2e_bias_act_*, w2e_demod_*, w2e_style_affine_* and w2e_mask_blend_* of csrc/elementwise.hip.  Written from the comments of
include/w2e.h and the semantics of models/stylegan2/model.py / op/fused_act.py / op/upfirdn2d.py -- not from the kernels: the ToRGB skip
is zero-stuffed and convolved with F.conv2d (no 2x2 tap shortcut), the sums are einsums, the nearest resize is an index_select.

Every function has a `*_scale` twin: the same formula on absolute values (sum |w|*|x| + |bias| + sum |k|*|skip|, ...), one term scale
per output element, which is what tests/test_gpu_gen_small_kernels.py judges every element against.  tests/test_gen_small_ref_host.py
holds this file to oracle/ and to float64 autograd."""
import torch
import torch.nn.functional as F


def f64(t):
    """float64 on the CPU; a float64 CPU tensor passes through as it is, so that autograd can run through every function here."""
    return None if t is None else torch.as_tensor(t).double().cpu()


# ---------------------------------------------------------------------------------------------- ToRGB
def up2(skip, upk):
    """Upsample of model.py:31-49: zero-stuff by 2 (sample, then a zero), pad 2 in front and 1 behind, TRUE convolution with the
    4x4 kernel (= correlation with the kernel flipped in both axes, op/upfirdn2d.py:47).  skip [B,C,hs,ws] -> [B,C,2hs,2ws]."""
    skip, upk = f64(skip), f64(upk)
    b, c, hs, ws = skip.shape
    z = skip.new_zeros(b, c, 2 * hs, 2 * ws)
    z[:, :, ::2, ::2] = skip
    z = F.pad(z, (2, 1, 2, 1))
    k = torch.flip(upk, (0, 1)).reshape(1, 1, 4, 4).expand(c, 1, 4, 4)
    return F.conv2d(z, k, groups=c)


def _weights(wmod, style):
    """[B,3,cin]: the per-sample weight itself, or wsc[c,i] * style[b,i] of the styled form."""
    wmod = f64(wmod)
    return wmod if style is None else wmod[None] * f64(style)[:, None, :]


def torgb_fwd(x, wmod, bias, skip, upk, style=None):
    """y[b,c] = sum_i w[b,c,i] x[b,i] + bias[c] + up2(skip)[b,c]."""
    y = torch.einsum("bci,bihw->bchw", _weights(wmod, style), f64(x))
    if bias is not None:
        y = y + f64(bias).reshape(1, 3, 1, 1)
    if skip is not None:
        y = y + up2(skip, upk)
    return y


def torgb_fwd_scale(x, wmod, bias, skip, upk, style=None):
    ab = lambda t: None if t is None else f64(t).abs()
    return torgb_fwd(ab(x), ab(wmod), ab(bias), ab(skip), ab(upk), ab(style))


def torgb_bwd(x, wmod, gy, gx_acc=None, style=None):
    """(gx, gw): gx[b,i] = sum_c w[b,c,i] gy[b,c] (+ gx_acc); gw = gwmod[b,c,i] = sum_p x[b,i,p] gy[b,c,p], or for the styled form the
    style gradient gstyle[b,i] = sum_c wsc[c,i] * that sum."""
    x, gy = f64(x), f64(gy)
    gx = torch.einsum("bci,bchw->bihw", _weights(wmod, style), gy)
    if gx_acc is not None:
        gx = gx + f64(gx_acc)
    gw = torch.einsum("bihw,bchw->bci", x, gy)
    if style is not None:
        gw = (gw * f64(wmod)[None]).sum(1)
    return gx, gw


def torgb_bwd_scale(x, wmod, gy, gx_acc=None, style=None):
    ab = lambda t: None if t is None else f64(t).abs()
    return torgb_bwd(ab(x), ab(wmod), ab(gy), ab(gx_acc), ab(style))


def _act_factor(y, slope, gain):
    """gain * (y > 0 ? 1 : slope): the derivative of lrelu(.)*gain, read off the sign of the OUTPUT (0 and -0 take the slope)."""
    y = f64(y)
    return gain * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))


def _pre(y, slope, gain):
    """The pre-activation an output y came from: y/gain (y > 0) or y/(gain*slope)."""
    y = f64(y)
    return torch.where(y > 0, y / gain, y / (gain * slope))


def torgb_bwd_actbwd(x, wmod, style, gy, gx_acc, noise, slope, gain):
    """(gpre, gw, sums3): x is the activated output of the layer below; gpre = gx * gain * (x > 0 ? 1 : slope) and sums3[b,i] =
    (sum_p gpre*pre, sum_p gpre*noise, sum_p gpre) as w2e_bias_act_bwd_reduce defines them.  gw as torgb_bwd (on x itself)."""
    gx, gw = torgb_bwd(x, wmod, gy, gx_acc, style)
    gpre = gx * _act_factor(x, slope, gain)
    b, cin, h, w = gpre.shape
    nz = torch.zeros(h, w, dtype=torch.float64) if noise is None else f64(noise).reshape(h, w)
    sums = torch.stack([(gpre * _pre(x, slope, gain)).sum((2, 3)), (gpre * nz).sum((2, 3)), gpre.sum((2, 3))], -1)
    return gpre, gw, sums


def torgb_bwd_actbwd_scale(x, wmod, style, gy, gx_acc, noise, slope, gain):
    gx, gw = torgb_bwd_scale(x, wmod, gy, gx_acc, style)
    gpre = gx * _act_factor(x, slope, gain)
    b, cin, h, w = gpre.shape
    nz = torch.zeros(h, w, dtype=torch.float64) if noise is None else f64(noise).abs().reshape(h, w)
    sums = torch.stack([(gpre * _pre(x, slope, gain).abs()).sum((2, 3)), (gpre * nz).sum((2, 3)), gpre.sum((2, 3))], -1)
    return gpre, gw, sums


# ---------------------------------------------------------------------------------------------- bias + noise + LeakyReLU * gain
def _bias_act_pre(x, bias, noise, noise_w, absolute=False):
    x = f64(x)
    assert x.ndim == 3, "x as [outer, channels, inner]"
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    v = ab(x)
    if bias is not None:
        v = v + ab(f64(bias)).reshape(1, -1, 1)
    if noise is not None:
        v = v + ab(f64(noise_w).reshape(()) * f64(noise).reshape(1, 1, -1))
    return v


def bias_act_fwd(x, bias, noise, noise_w, slope, gain):
    """y = lrelu(x + noise_w*noise[i] + bias[c], slope) * gain (op/fused_act.py:23-39 with model.py:285-290 folded in)."""
    return F.leaky_relu(_bias_act_pre(x, bias, noise, noise_w), slope) * gain


def bias_act_fwd_scale(x, bias, noise, noise_w, slope, gain):
    """(|x| + |bias| + |noise_w*noise|) times the factor of the branch the float64 pre-activation takes."""
    v = _bias_act_pre(x, bias, noise, noise_w)
    return _bias_act_pre(x, bias, noise, noise_w, True) * torch.where(v > 0, torch.ones_like(v), torch.full_like(v, abs(slope))) * gain


def bias_act_bwd(gy, y, slope, gain):
    """gx = gy * gain * (y > 0 ? 1 : slope)."""
    return f64(gy) * _act_factor(y, slope, gain)


def bias_act_bwd_scale(gy, y, slope, gain):
    return f64(gy).abs() * _act_factor(y, slope, gain).abs()


def bias_act_bwd_reduce(gy, y, noise, slope, gain):
    """(gx, sums [outer,C,3]) for gy, y [outer,C,inner]: sums = (sum gx*pre, sum gx*noise, sum gx)."""
    gx = bias_act_bwd(gy, y, slope, gain)
    nz = torch.zeros(gx.shape[-1], dtype=torch.float64) if noise is None else f64(noise).reshape(-1)
    return gx, torch.stack([(gx * _pre(y, slope, gain)).sum(-1), (gx * nz).sum(-1), gx.sum(-1)], -1)


def bias_act_bwd_reduce_scale(gy, y, noise, slope, gain):
    gx = bias_act_bwd_scale(gy, y, slope, gain)
    nz = torch.zeros(gx.shape[-1], dtype=torch.float64) if noise is None else f64(noise).abs().reshape(-1)
    return gx, torch.stack([(gx * _pre(y, slope, gain).abs()).sum(-1), (gx * nz).sum(-1), gx.sum(-1)], -1)


# ---------------------------------------------------------------------------------------------- demodulation
def demod_sum(s, wsq):
    """sum_i s[b,i]^2 wsq[o,i]  [B,cout]: every term is >= 0 for a wsq of squares, so it is its own scale."""
    return f64(s).pow(2) @ f64(wsq).t()


def demod_fwd(s, wsq, eps):
    """d[b,o] = rsqrt(sum_i s[b,i]^2 wsq[o,i] + eps)  (model.py:241-243)."""
    return torch.rsqrt(demod_sum(s, wsq) + eps)


def demod_fwd_scale(s, wsq, eps):
    """|d| itself: the relative error of d is half the relative error of the (all-positive) sum, plus rsqrt's own."""
    return torch.rsqrt(f64(s).pow(2) @ f64(wsq).abs().t() + eps)


def demod_dz(sums, dz, noise_w, bias, absolute=False):
    """dz[b,o] as given, or rebuilt from the fused activation sums: s1 - noise_w*s2 - bias[o]*s3."""
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    if dz is not None:
        return ab(f64(dz))
    q = f64(sums)
    out, sign = ab(q[..., 0]), (1.0 if absolute else -1.0)
    if noise_w is not None:
        out = out + sign * ab(f64(noise_w).reshape(()) * q[..., 1])
    if bias is not None:
        out = out + sign * ab(f64(bias).reshape(1, -1) * q[..., 2])
    return out


def demod_bwd(sums, dz, noise_w, bias, d, s, wsq, gs0):
    """(gs, gd): gs = gs0 - s[b,i] * sum_o dz[b,o] d[b,o]^2 wsq[o,i]; gd = dz / d."""
    z = demod_dz(sums, dz, noise_w, bias)
    d, s = f64(d), f64(s)
    return f64(gs0) - s * ((z * d * d) @ f64(wsq)), z / d


def demod_bwd_scale(sums, dz, noise_w, bias, d, s, wsq, gs0):
    z = demod_dz(sums, dz, noise_w, bias, True)
    d, s = f64(d).abs(), f64(s).abs()
    return f64(gs0).abs() + s * ((z * d * d) @ f64(wsq).abs()), z / d


# ---------------------------------------------------------------------------------------------- the stacked style affines
def style_affine_fwd(latent, w, bias, layers):
    """layers = [(W+ index, width)] in stacking order; w [R,D], bias [R] or None.  One [B,width] tensor per layer:
    latent[:, widx] @ W_l^T + b_l (EqualLinear, model.py:151-158, with scale and lr_mul already folded into w and bias)."""
    latent, w = f64(latent), f64(w)
    out, off = [], 0
    for widx, cw in layers:
        y = latent[:, widx] @ w[off:off + cw].t()
        if bias is not None:
            y = y + f64(bias)[off:off + cw]
        out.append(y)
        off += cw
    return out


def style_affine_fwd_scale(latent, w, bias, layers):
    ab = lambda t: None if t is None else f64(t).abs()
    return style_affine_fwd(ab(latent), ab(w), ab(bias), layers)


def style_affine_bwd(gouts, w, layers, n_latent):
    """glatent [B,n_latent,D] = sum over the layers of a W+ index of gout_l @ W_l; 0 for an index no layer uses."""
    w = f64(w)
    gl = torch.zeros(gouts[0].shape[0], n_latent, w.shape[1], dtype=torch.float64)
    off = 0
    for (widx, cw), g in zip(layers, gouts):
        gl[:, widx] += f64(g) @ w[off:off + cw]
        off += cw
    return gl


def style_affine_bwd_scale(gouts, w, layers, n_latent):
    return style_affine_bwd([f64(g).abs() for g in gouts], f64(w).abs(), layers, n_latent)


# ---------------------------------------------------------------------------------------------- region-attention blend
def nearest_index(size, ms):
    """Source index of every destination index for torch's default `nearest` resize of ms -> size:
    min(floor(dst * fp32(ms / size)), ms - 1), the product in fp32 as torch (and the kernel) forms it -- in float64 a ratio such as 9/7
    rounds differently and a pixel on a cell border would move."""
    scale = torch.tensor(float(ms), dtype=torch.float32) / torch.tensor(float(size), dtype=torch.float32)
    src = torch.floor(torch.arange(size, dtype=torch.float32) * scale).long()
    return src.clamp_max(ms - 1)


def resized_mask(mask, h, w):
    mask = f64(mask)
    ms = mask.shape[-1]
    return mask.index_select(2, nearest_index(h, ms)).index_select(3, nearest_index(w, ms))


def mask_blend_fwd(a, b, mask):
    """m*a + (1-m)*b with m the nearest-resized mask [B,1,ms,ms] (attention_model.py:548-549)."""
    a, b = f64(a), f64(b)
    m = resized_mask(mask, a.shape[2], a.shape[3])
    return m * a + (1 - m) * b


def mask_blend_fwd_scale(a, b, mask):
    a, b = f64(a).abs(), f64(b).abs()
    m = resized_mask(mask, a.shape[2], a.shape[3])
    return m.abs() * a + (1 + m.abs()) * b


def _to_cells(t, ms, h, w):
    """Sum a [B,1,h,w] map into the mask cells its pixels map to: [B,1,ms,ms]; a cell no pixel maps to stays 0."""
    iy, ix = nearest_index(h, ms), nearest_index(w, ms)
    out = torch.zeros(t.shape[0], 1, ms, w, dtype=torch.float64).index_add_(2, iy, t)
    return torch.zeros(t.shape[0], 1, ms, ms, dtype=torch.float64).index_add_(3, ix, out)


def mask_blend_bwd(gout, a, b, mask):
    """(ga, gb, gmask): ga = m*gout, gb = (1-m)*gout, gmask[b,my,mx] = sum over channels and the cell's pixels of gout*(a-b)."""
    gout, a, b = f64(gout), f64(a), f64(b)
    h, w = a.shape[2:]
    m = resized_mask(mask, h, w)
    return m * gout, (1 - m) * gout, _to_cells((gout * (a - b)).sum(1, keepdim=True), mask.shape[-1], h, w)


def mask_blend_bwd_scale(gout, a, b, mask):
    gout, a, b = f64(gout).abs(), f64(a).abs(), f64(b).abs()
    h, w = a.shape[2:]
    m = resized_mask(mask, h, w).abs()
    return m * gout, (1 + m) * gout, _to_cells((gout * (a + b)).sum(1, keepdim=True), mask.shape[-1], h, w)


def pixels_per_cell(size, ms):
    """How many destination indices map to each of the ms source indices."""
    return torch.bincount(nearest_index(size, ms), minlength=ms)
