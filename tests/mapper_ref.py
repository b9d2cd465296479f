"""The latent mappers' arithmetic in float64 on the CPU: a plain restatement of the formulas in the K7 comments of include/w2e.h (the
level mappers w2e_mapper_* and the style-space mappers w2e_ssmapper_*), the reference tests/test_gpu_mapper_rest_kernels.py holds the
kernels of csrc/mapper.hip to.  Nothing here touches the library; tests/test_mapper_ref_host.py holds these functions to
oracle/mappers.py and to float64 autograd.

Every output has a `*_scale` twin: the same formula on absolute values (sum |terms|), the scale an element's error is judged against.
The one constant that is not exact in the kernels' arithmetic enters as the float the kernels use: EPS = float32(1e-8)."""
import math

import torch

D = 512                                              # the level mappers' width
U = 2.0 ** -24                                       # one fp32 rounding, relative
SLOPE, GAIN = 0.2, math.sqrt(2.0)                    # fused_lrelu
EPS = float(torch.tensor(1e-8, dtype=torch.float32))  # PixelNorm's epsilon as the kernels add it (1e-8f)


def f64(t):
    return t.detach().to("cpu", torch.float64)


# ---------------------------------------------------------------------------------------------- layouts
def gather_rows(t, levels):
    """[B, n_latent, 512] -> group-major rows: row r0_g + b * len_g + l = latent l0_g + l of sample b."""
    return torch.cat([t[:, l0:l0 + ln].reshape(-1, t.shape[-1]) for l0, ln in levels], 0)


def split_rows(rows, batch, levels):
    """Group-major rows -> the list of per-group [B * len_g, 512] blocks."""
    out, r = [], 0
    for _, ln in levels:
        out.append(rows[r:r + batch * ln])
        r += batch * ln
    assert r == rows.shape[0]
    return out


def scatter_rows(rows, batch, n_latent, levels):
    """Group-major rows -> [B, n_latent, 512], latents outside every level 0."""
    out = torch.zeros(batch, n_latent, rows.shape[-1], dtype=rows.dtype)
    for (l0, ln), blk in zip(levels, split_rows(rows, batch, levels)):
        out[:, l0:l0 + ln] = blk.reshape(batch, ln, -1)
    return out


def ss_pack(codes):
    """A list of [B, dims[c]] code tensors -> the packed code-major vector: code c is the row-major block at B * sum_{i<c} dims[i]."""
    return torch.cat([c.reshape(-1) for c in codes], 0)


def ss_unpack(flat, batch, dims):
    out, off = [], 0
    for d in dims:
        out.append(flat[off:off + batch * d].view(batch, d))
        off += batch * d
    assert off == flat.numel()
    return out


# ---------------------------------------------------------------------------------------------- PixelNorm
def pixelnorm(x, dim, eps=EPS):
    """x * rsqrt(mean over `dim` of x^2 + eps)."""
    x = f64(x)
    return x * torch.rsqrt((x * x).mean(dim=dim, keepdim=True) + eps)


def levels_pixelnorm(x, levels, eps=EPS):
    """w2e_mapper_pixelnorm: PixelNorm over the LATENTS of each level of x [B, n_latent, 512] (dim = 1 of the [B, len, 512] slice), gathered
    into group-major rows.  Latents outside every level are not read."""
    return torch.cat([pixelnorm(x[:, l0:l0 + ln], 1, eps).reshape(-1, x.shape[-1]) for l0, ln in levels], 0)


def ss_pixelnorm(codes, eps=EPS):
    """w2e_ssmapper_pixelnorm: PixelNorm over the FEATURES of each [B, dims[c]] code, packed."""
    return ss_pack([pixelnorm(c.reshape(c.shape[0], -1), 1, eps) for c in codes])


# ---------------------------------------------------------------------------------------------- one EqualLinear + fused lrelu
def linear_fwd(a, w, bias, w_scale, b_scale):
    """out = lrelu(w_scale * a W^T + b_scale * bias, 0.2) * sqrt2  (W [out, in], row = output feature); bias may be None."""
    pre = w_scale * f64(a) @ f64(w).T + (b_scale * f64(bias) if bias is not None else 0.0)
    return torch.where(pre > 0, pre, pre * SLOPE) * GAIN


def linear_fwd_scale(a, w, bias, w_scale, b_scale, n):
    """sum |terms| of linear_fwd times the slope the reference took; an element whose pre-activation lies within the bound (n roundings
    of its terms) of 0 is judged with slope 1: lrelu is 1-Lipschitz times its gain."""
    pre = w_scale * f64(a) @ f64(w).T + (b_scale * f64(bias) if bias is not None else 0.0)
    tot = w_scale * f64(a).abs() @ f64(w).abs().T + (b_scale * f64(bias).abs() if bias is not None else 0.0)
    slope = torch.where(pre < -n * U * tot, torch.full_like(pre, SLOPE), torch.ones_like(pre))
    return tot * slope * GAIN


def gpre(gy, y):
    """The gradient at the pre-activation of a layer whose output was y: gy * sqrt2 * (y > 0 ? 1 : 0.2).  The branch is y > 0: y == 0
    and y == -0.0 take 0.2."""
    y = f64(y)
    return f64(gy) * GAIN * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))


def linear_bwd(gp, w, w_scale):
    """The layer's input gradient: w_scale * gpre W, the weight as stored."""
    return w_scale * f64(gp) @ f64(w)


def linear_bwd_scale(gp, w, w_scale):
    return w_scale * f64(gp).abs() @ f64(w).abs()


def wgrad(gp, h_in, w_scale, b_scale):
    """(gW, gb) = (w_scale * gpre^T h_in, b_scale * column sums of gpre) of one group / one code: gp [rows, out], h_in [rows, in]."""
    return w_scale * f64(gp).T @ f64(h_in), b_scale * f64(gp).sum(0)


def wgrad_scale(gp, h_in, w_scale, b_scale):
    return w_scale * f64(gp).abs().T @ f64(h_in).abs(), b_scale * f64(gp).abs().sum(0)


# ---------------------------------------------------------------------------------------------- a whole Mapper, layer by layer
def mapper_forward(h0, weights, biases, w_scale, b_scale):
    """[h0, h1, ..., h4]: h0 = the PixelNorm output [rows, d], h_{j+1} = linear_fwd(h_j, weights[j], biases[j])."""
    h = [f64(h0)]
    for w, b in zip(weights, biases):
        h.append(linear_fwd(h[-1], w, b, w_scale, b_scale))
    return h


def mapper_backward(h, weights, gout, w_scale, b_scale):
    """The weight and bias gradients of every layer for the output gradient gout [rows, d], as the autograd nodes of mapper_hip.py
    walk them: gpre of layer j from (gy, h_{j+1}), its wgrad with h_j, then gy = linear_bwd.  -> ([gW_0..], [gb_0..])."""
    gws, gbs, gy = [None] * len(weights), [None] * len(weights), f64(gout)
    for j in range(len(weights) - 1, -1, -1):
        gp = gpre(gy, h[j + 1])
        gws[j], gbs[j] = wgrad(gp, h[j], w_scale, b_scale)
        gy = linear_bwd(gp, weights[j], w_scale)
    return gws, gbs
