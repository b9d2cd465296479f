"""Float64 restatements of the entry points of csrc/disc.hip (K8: fromRGB, the minibatch-stddev layer, their forward-mode halves, the
per-row sum of squares) and of w2e_modconv_wgrad_finish / w2e_modconv_wsq (csrc/wgrad.hip), with the term scale T of every output
element, the rounding counts K the kernels are held to (|got - ref| <= K * 2^-24 * T), fp32 restatements of the stddev kernels in the
kernels' own operation order, the two input families and the shape lists.  tests/test_disc_ref_host.py holds all of it on the CPU (to
float64 autograd of tests/disc64.py, tests/r1_ref.py and oracle/stylegan2.py); tests/test_gpu_disc_kernels.py holds the kernels to it.

Layouts: images are [B, C, hw] (the kernels never look at rows and columns); the stddev group of sample b = g * M + m is m (model.py:
690-698: view(group, -1, ...), var(0)), so a [B, ...] tensor viewed as [group, M, ...] has the group's members along dim 0."""
import math
import zlib

import torch

U = 2.0 ** -24
SQRT2 = math.sqrt(2.0)
SLOPE = 0.2
F64, F32 = torch.float64, torch.float32
FR_PPB, FR_MAX_C, STREAM_CAP = 1024, 512, 2048 * 256   # pixels per workgroup of fromrgb_bwd_kernel; its channel limit; stream_grid's cap
SQ_CHUNK = 4096


def f64(t):
    return torch.as_tensor(t).detach().to(F64).cpu()


def f32scale(scale):
    """The float the C ABI receives for a Python `scale` (ctypes c_float rounds it): the references use this value."""
    return float(torch.tensor(float(scale), dtype=F32))


# ---------------------------------------------------------------------------------------------- inputs
def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def heavy(key, shape):
    """The suite's heavy-tailed family (test_gpu_discriminator._heavy): a normal times a log-normal spread of magnitudes."""
    gen = _gen(key)
    return (torch.randn(shape, generator=gen) * torch.exp(1.5 * torch.randn(shape, generator=gen))).contiguous()


def separated(key, shape):
    """[B, ...] with the members of a stddev group well apart: randn + 3 * g for sample b = g * M + m, so (x - mean) / sd is well
    conditioned and a tight bound is not carried by cancellation alone."""
    b = shape[0]
    group = min(b, 4)
    g = (torch.arange(b) // (b // group)).to(F32).view(b, *([1] * (len(shape) - 1)))
    return (torch.randn(shape, generator=_gen(key)) + 3.0 * g).contiguous()


FAMILIES = {"heavy": heavy, "separated": separated}


def layer_output(key, shape):
    """A saved activation for the slope masks: both signs, one entry in eight exactly 0, one in sixty-four -0.0 (both on the 0.2 side)."""
    y = heavy(key, shape)
    y.view(-1)[::8] = 0.0
    y.view(-1)[4::64] = -0.0
    return y


# ---------------------------------------------------------------------------------------------- the shape lists
MBSTD_BATCHES = (1, 2, 3, 4, 8, 12)       # groups 1, 2, 3, 4, 4, 4 with M = 1, 1, 1, 1, 2, 3 workgroups
MBSTD_REFUSED = (5, 6, 7)                 # no multiple of min(batch, 4)
MBSTD_SHAPES = {                          # (C, hw) -> the path it reaches
    (512, 16): "the model's shape: n = 8192, 32 strides of the element loop, group * hw <= 64",
    (1, 1): "n = 1: one thread works, the tree adds zeros, the mean over n divides by 1",
    (3, 5): "n = 15 < 256: most threads idle, one stride",
    (7, 37): "n = 259: a second stride of 3 elements; hw odd",
    (3, 100): "group * hw up to 400 > 256: the gsum loop and the stddev write-out take a second stride",
}

FROMRGB_CASES = {                         # name -> ((B, C, hw), the path it reaches)
    "px1_c1": ((1, 1, 1), "one pixel, C = 1 (below the 3 input channels)"),
    "px1023_c3": ((1, 3, 1023), "one short of FR_PPB: the last thread of the backward's last pixel slot idles"),
    "px1024_c255": ((1, 255, 1024), "exactly one backward workgroup; the partial write-out loop one short of 256"),
    "px1025_c256": ((1, 256, 1025), "a second backward workgroup with one pixel; write-out exactly 256"),
    "straddle_c257": ((3, 257, 407), "1221 pixels: a workgroup straddles two samples; write-out takes a second stride"),
    "rows258_c1": ((2, 1, 131600), "263200 pixels = 258 partial rows: fromrgb_finish_kernel's row loop takes a second stride; C = 1"),
    "capped_c2": ((1, 2, 524288 + 37), "37 pixels past the stream_grid cap (2048 blocks x 256): threads walk a second pixel"),
    "model_b3": ((3, 512, 1024), "the 32^2 Discriminator at batch 3: C = FR_MAX_C"),
    "model_b4": ((4, 512, 1024), "the 32^2 Discriminator at batch 4"),
}
FROMRGB_REFUSED = ((1, 513, 16), (1, 4, 0))   # C above FR_MAX_C; hw = 0

SUMSQ_LENGTHS = (1, 255, 256, 4095, 4096, 4097, 4096 * 256 + 5, 3 * 32 * 32)   # around SQ_CHUNK; 257 chunks (a second finish stride); the 32^2 image
SUMSQ_BATCHES = (1, 3)

FINISH_SPLITS = (1, 3, 4, 5, 9)           # fewer than the 4 waves, exactly 4, a second stride for wave 0, a third
FINISH_TAPS = (1, 9)
FINISH_DIMS = ((1, 1), (3, 7), (5, 13), (33, 20))   # (cout, cin): n = taps * cout * cin from 1 (< 64) over 189 (no multiple of 64) to 5940 (93 blocks)
FINISH_BATCHES = (1, 3)
FINISH_FORMS = ("none", "dz", "sums_nw_bias", "sums_nw", "sums_bias", "sums")
WSQ_DIMS = ((1, 1), (15, 17), (257, 1))   # cout * cin = 1, 255, 257: below, one short of and one past a 256-thread block


# ---------------------------------------------------------------------------------------------- fromRGB
def fromrgb_fwd(x, w, bias, scale):
    """(y, T): y [B,C,hw] = lrelu(scale * w x + bias, 0.2) * sqrt2 from x [B,3,hw], w [C,3], bias [C] or None; T the term scale:
    sqrt2 * (scale * |w| |x| + |bias|), times 0.2 where the pre-activation is negative by more than FROMRGB_FWD_K roundings of it
    (LeakyReLU is 1-Lipschitz, so nearer to 0 the error of y is at most the error of the pre-activation)."""
    x, w = f64(x), f64(w)
    v = scale * torch.einsum("oi,bip->bop", w, x)
    t = scale * torch.einsum("oi,bip->bop", w.abs(), x.abs())
    if bias is not None:
        v = v + f64(bias).view(1, -1, 1)
        t = t + f64(bias).abs().view(1, -1, 1)
    y = torch.where(v > 0, v, SLOPE * v) * SQRT2
    safe_neg = v < -FROMRGB_FWD_K * U * t
    return y, SQRT2 * t * (1.0 - (1.0 - SLOPE) * safe_neg.to(F64))


def slope_of(y):
    """1 where the saved activation is positive, 0.2 elsewhere (0 and -0.0 included), in float64."""
    one = torch.ones((), dtype=F64)
    return torch.where(f64(y) > 0, one, SLOPE * one)


def gpre(gy, y):
    """gy * sqrt2 * (y > 0 ? 1 : 0.2): the pre-activation gradient from the saved OUTPUT y (0 and -0.0 sit on the 0.2 side)."""
    return f64(gy) * SQRT2 * slope_of(y)


def fromrgb_bwd(gy, y, x, w, scale):
    """(gx [B,3,hw], dw [C,3], db [C]) and their term scales (the same formulas on absolute values)."""
    g, x, w = gpre(gy, y), f64(x), f64(w)
    out = (scale * torch.einsum("oi,bop->bip", w, g), scale * torch.einsum("bop,bip->oi", g, x), g.sum((0, 2)))
    ga = g.abs()
    scl = (scale * torch.einsum("oi,bop->bip", w.abs(), ga), scale * torch.einsum("bop,bip->oi", ga, x.abs()), ga.sum((0, 2)))
    return out, scl


def fromrgb_jvp(dx, y, w, scale):
    """(t, T): t [B,C,hw] = sqrt2 * (y > 0 ? 1 : 0.2) * scale * w dx."""
    m = SQRT2 * slope_of(y)
    return (m * scale * torch.einsum("oi,bip->bop", f64(w), f64(dx)),
            m * scale * torch.einsum("oi,bip->bop", f64(w).abs(), f64(dx).abs()))


def fromrgb_rows(batch, hw):
    return -(-batch * hw // FR_PPB)


# Rounding counts, from csrc/disc.hip (a fp32 constant's own error counts as a fraction of a rounding: 0.2f 0.25, sqrt2f 0.3):
#   fromrgb_fwd_kernel   w * scale 1, the products 1, two additions 2, + bias 1, * 0.2f 1.25, * sqrt2f 1.3 = 7.55
FROMRGB_FWD_K = 8
#   fromrgb_jvp_kernel   w * scale 1, the products 1, two additions 2, * (0.2f * sqrt2f) 1 + 1.05 for the folded constant = 6.05
FROMRGB_JVP_K = 7


def fromrgb_gx_k(c):
    """fromrgb_bwd_kernel, gx: gpre = gy * sqrt2f * 0.2f 2.55, then ga += w * g once per output channel in ascending order (one rounding
    each when fused, the product's and the sum's otherwise: the chain is C long, + 1 for the unfused product), scale * ga 1."""
    return c + 5


def fromrgb_dw_k(rows):
    """dw: gpre 2.55, g * x 1, the thread's four pixels 3 additions, the 64-lane butterfly 6, the four waves 3, fromrgb_finish_kernel's
    row loop ceil(rows / 256), its 256-wide tree 8, scale * 1 = 24.55 + ceil(rows / 256)."""
    return 25 + -(-rows // 256)


def fromrgb_db_k(rows):
    """db: as dw without the product and the scale."""
    return 23 + -(-rows // 256)


# ---------------------------------------------------------------------------------------------- the minibatch stddev layer
def mbstd_group(batch):
    return min(batch, 4)


def _grouped(t, group):
    return t.reshape(group, t.shape[0] // group, *t.shape[1:])


def mbstd_stats(x):
    """x [B,C,hw] -> (group, v [group,M,n], c = v - mean over the group, sd [M,n] = sqrt(var + 1e-8)), float64."""
    x = f64(x)
    group = mbstd_group(x.shape[0])
    v = _grouped(x.reshape(x.shape[0], -1), group)
    c = v - v.mean(0, keepdim=True)
    return group, v, c, torch.sqrt((c * c).mean(0) + 1e-8)


def mbstd_value(x):
    """s [M]: the stddev channel's value of every group."""
    return mbstd_stats(x)[3].mean(1)


def mbstd_fwd(x):
    """y [B,C+1,hw] = [x | s of the sample's group]."""
    x = f64(x)
    b, c, hw = x.shape
    group = mbstd_group(b)
    s = mbstd_value(x)
    return torch.cat([x, s.repeat(group).view(b, 1, 1).expand(b, 1, hw)], 1)


def _coef(gy, group, n):
    """(coef [M], cabs [M]): the sum of the group's stddev-channel cotangents over samples and pixels / (group * n), and the same on
    absolute values -- the scale of the errors of that signed fp32 sum itself (and of nothing else: mbstd_scales)."""
    gs = _grouped(f64(gy)[:, -1, :], group)          # [group, M, hw]
    return gs.sum((0, 2)) / (group * n), gs.abs().sum((0, 2)) / (group * n)


def mbstd_bwd(gy, x):
    """(gx [B,C,hw], its stddev part alone): gx = gy[:, :C] + coef * (x - mean) / sd."""
    b, c, hw = x.shape
    group, v, cen, sd = mbstd_stats(x)
    coef, _ = _coef(gy, group, c * hw)
    part = (coef.view(1, -1, 1) * cen / sd).reshape(b, c, hw)
    return f64(gy)[:, :c] + part, part


def mbstd_jvp(x, dx):
    """jv [M]: the tangent of the stddev value along dx = the mean over n of sum_g c_g dx_g / (group * sd)."""
    group, v, cen, sd = mbstd_stats(x)
    d = _grouped(f64(dx).reshape(dx.shape[0], -1), group)
    return ((cen * d).sum(0) / (group * sd)).mean(1)


def mbstd_hvp(gy, x, dx):
    """mu [B,C,hw] = coef * ((dx - mean dx) / sd - P c / (group * sd^3)), P = sum_g c_g dx_g (the header comment of mbstd_hvp_kernel)."""
    b, c, hw = x.shape
    group, v, cen, sd = mbstd_stats(x)
    coef, _ = _coef(gy, group, c * hw)
    d = _grouped(f64(dx).reshape(b, -1), group)
    p = (cen * d).sum(0)
    mu = coef.view(1, -1, 1) * ((d - d.mean(0, keepdim=True)) / sd - p * cen / (group * sd ** 3))
    return mu.reshape(b, c, hw)


def mbstd_scales(x, gy=None, dx=None):
    """The term scales of the four stddev outputs (whichever the operands allow), as a dict:
      s   [M]       mean_e A_e + s * log2 n                                       A_e = max_g |x_g,e|
      gx  [B,C,hw]  ceff_gx * amp_e * (1 + cs)                                    amp_e = max(1, A_e / sd_e), cs = |x - mean| / sd
      jv  [M]       mean_e[amp_e * D_e * (1 + max_g cs)] + |jv| * log2 n          D_e = max_g |dx_g,e|
      mu  [B,C,hw]  (ceff_mu / sd_e) * amp_e * D_e * (1 + cs) * (1 + max_g cs)
    ceff = |coef| + (Dg / K) * cabs with K the output's rounding count (mbstd_gx_k, mbstd_mu_k): K roundings of the scale on |coef|
    for the chain behind the coefficient, and the Dg roundings of the coefficient's own signed fp32 sum (block_sum_256 and the
    division), which are relative to cabs = the sum on absolute values, not to |coef|.  So the bound K * 2^-24 * T is
    (K |coef| + Dg cabs) * 2^-24 * amp (1 + cs): only the coefficient's own sum is charged to cabs.  "coef" and "cabs" are returned too."""
    b, c, hw = x.shape
    n = c * hw
    group, v, cen, sd = mbstd_stats(x)
    a = v.abs().amax(0)
    amp = (a / sd).clamp_min(1.0)
    cs = cen.abs() / sd
    out = {"s": a.mean(1) + sd.mean(1) * math.log2(n)}
    if gy is not None:
        coef, cabs = _coef(gy, group, n)
        dg = _dn(group * hw)
        out["coef"], out["cabs"] = coef, cabs
        ceff = coef.abs() + dg / mbstd_gx_k(group, c, hw) * cabs
        out["gx"] = (ceff.view(1, -1, 1) * amp * (1 + cs)).reshape(b, c, hw)
    if dx is not None:
        dd = _grouped(f64(dx).reshape(b, -1), group).abs().amax(0)
        mcs = cs.amax(0)
        out["jv"] = (amp * dd * (1 + mcs)).mean(1) + mbstd_jvp(x, dx).abs() * math.log2(n)
        if gy is not None:
            ceff = coef.abs() + dg / mbstd_mu_k(group, c, hw) * cabs
            out["mu"] = ((ceff.view(-1, 1) / sd) * amp * dd * (1 + cs) * (1 + mcs)).reshape(b, c, hw)
    return out


# Rounding counts of the stddev kernels, from csrc/disc.hip.  With g = group:
#   E = 1.5 g + 4: one factor (x - mean) / sd in units of amp.  The mean: g - 1 additions and the division, each at most one rounding
#       of A (g); x - mean one rounding of at most 2 A (2): the centred value is off by (g + 2) roundings of A, and so is sd, which is
#       1-Lipschitz in the centred values; sd's own arithmetic -- the squares 1, g - 1 additions, / group 1, + 1e-8f 1, halved by the
#       square root, + the square root's rounding -- adds g / 2 + 2 roundings of sd <= A.
#   Dn = ceil(n / 256) + 9: block_sum_256 behind the element loop: the thread's strided sum, the 64-lane butterfly 6, the four waves 3,
#       / n 1.   Dg = ceil(g * hw / 256) + 9: the same behind the gsum loop, with the division by group * n.
def _e(group):
    return 1.5 * group + 4


def _dn(n):
    return -(-n // 256) + 9


def mbstd_s_k(group, c, hw):
    """mbstd_fwd_kernel: every sd_e is within E roundings of A_e; the all-positive sum over n and the division are within Dn roundings
    of s, and the scale counts s log2 n times."""
    n = c * hw
    return max(_e(group), _dn(n) / math.log2(n) if n > 1 else 0.0)


def mbstd_gx_k(group, c, hw):
    """mbstd_bwd_kernel, stddev part, behind the coefficient (whose own Dg roundings are charged to cabs in mbstd_scales): one factor
    (x - mean) / sd E, coef / sd 1, its product with x - mean 1.  (With the identity part the final addition adds one rounding of |gx|.)"""
    return _e(group) + 2


def mbstd_jv_k(group, c, hw):
    """mbstd_jvp_kernel: the centred values in the dot product E, sd E, the dot product's g fused steps and the division by
    group * sd (within the 4 and the slack of 2 E), the sum over n and the division Dn."""
    return _dn(c * hw) + 2 * _e(group) + 4


def mbstd_mu_k(group, c, hw):
    """mbstd_hvp_kernel, behind the coefficient (its own Dg roundings are charged to cabs in mbstd_scales): sd enters the second term to
    the third power (3 E), the centred values of x and of dx in the dot product and in the two factors (one more E); 8 for the
    products, the two divisions and the final subtraction."""
    return 4 * _e(group) + 8


# ---- fp32 restatements of the stddev kernels in their own operation order (CPU): what the bounds must hold for before any kernel runs
def _block_sum32(terms):
    """block_sum_256 of fp32 terms [M, count]: thread t adds elements t, t + 256, ... in order; the xor butterfly over each wave's 64
    lanes (offsets 32 ... 1); the four waves' sums in wave order."""
    m, count = terms.shape
    steps = max(1, -(-count // 256))
    pad = torch.zeros(m, steps * 256, dtype=F32)
    pad[:, :count] = terms
    pad = pad.view(m, steps, 256)
    acc = torch.zeros(m, 256, dtype=F32)
    for k in range(steps):
        acc = acc + pad[:, k]
    w = acc.view(m, 4, 64)
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lanes ^ off]
    r = w[..., 0]
    return ((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]


def _stats32(x):
    x = x.to(F32)
    group = mbstd_group(x.shape[0])
    v = _grouped(x.reshape(x.shape[0], -1), group)
    mean = v[0].clone()
    for g in range(1, group):
        mean = mean + v[g]
    mean = mean / float(group)
    cen = v - mean
    var = torch.zeros_like(mean)
    for g in range(group):
        var = var + cen[g] * cen[g]
    return group, v, mean, cen, var / float(group) + torch.tensor(1e-8, dtype=F32)


def _coef32(gy, group, n):
    gs = _grouped(gy.to(F32)[:, -1, :], group)     # [group, M, hw]: the kernel's e = g * hw + p
    return _block_sum32(gs.permute(1, 0, 2).reshape(gs.shape[1], -1)) / (float(group) * float(n))


def mbstd_value32(x):
    group, v, mean, cen, sd2 = _stats32(x)
    return _block_sum32(torch.sqrt(sd2)) / float(v.shape[2])


def mbstd_bwd32(gy, x):
    b, c, hw = x.shape
    group, v, mean, cen, sd2 = _stats32(x)
    k = _coef32(gy, group, c * hw).view(-1, 1) / torch.sqrt(sd2)
    return gy.to(F32)[:, :c] + (k * cen).reshape(b, c, hw)


def mbstd_jvp32(x, dx):
    group, v, mean, cen, sd2 = _stats32(x)
    d = _grouped(dx.to(F32).reshape(dx.shape[0], -1), group)
    dot = torch.zeros_like(mean)
    for g in range(group):
        dot = dot + cen[g] * d[g]
    return _block_sum32(dot / (float(group) * torch.sqrt(sd2))) / float(v.shape[2])


def mbstd_hvp32(gy, x, dx):
    b, c, hw = x.shape
    group, v, mean, cen, sd2 = _stats32(x)
    d = _grouped(dx.to(F32).reshape(b, -1), group)
    dmean = d[0].clone()
    for g in range(1, group):
        dmean = dmean + d[g]
    dmean = dmean / float(group)
    dot = torch.zeros_like(mean)
    for g in range(group):
        dot = dot + cen[g] * (d[g] - dmean)
    k1 = _coef32(gy, group, c * hw).view(-1, 1) / torch.sqrt(sd2)
    k2 = k1 * dot / (float(group) * sd2)
    return (k1 * (d - dmean) - k2 * cen).reshape(b, c, hw)


def mbstd_inputs(family, batch, c, hw):
    """(x [B,C,hw], dx [B,C,hw], gy [B,C+1,hw]) of one family, fp32, seeded by the case."""
    make = FAMILIES[family]
    key = f"disc_ref.mbstd.{family}.{batch}.{c}.{hw}"
    return make(key + ".x", (batch, c, hw)), make(key + ".dx", (batch, c, hw)), heavy(key + ".gy", (batch, c + 1, hw))


# ---------------------------------------------------------------------------------------------- sumsq_rows
def sumsq(x):
    """[B, n] -> [B] (its own term scale: every term is positive)."""
    return (f64(x) ** 2).sum(1)


def sumsq_parts(n):
    """w2e_sumsq_rows_parts: ceil(n / SQ_CHUNK) for 0 < n < SQ_CHUNK * 65535, else 0."""
    return -(-n // SQ_CHUNK) if 0 < n < SQ_CHUNK * 65535 else 0


def sumsq_k(n):
    """sumsq_part_kernel: the square 1, the thread's 16 elements 15 additions, the butterfly 6, the four waves 3; sumsq_finish_kernel:
    its chunk loop ceil(chunks / 256), the butterfly 6, the four waves 3."""
    return 34 + -(-sumsq_parts(n) // 256)


# ---------------------------------------------------------------------------------------------- the weight-gradient finish
def finish_dz(form, sums, dz, noise_w, bias):
    """(dz [B,Cout], its term scale) of an operand form: given directly, or sums[b,o,0] - noise_w * sums[b,o,1] - bias[o] * sums[b,o,2]
    with either of noise_w / bias absent (0)."""
    if form == "dz":
        return f64(dz), f64(dz).abs()
    s = f64(sums)
    nw = float(noise_w) if "nw" in form else 0.0
    bv = f64(bias).view(1, -1) if "bias" in form else torch.zeros(1, s.shape[1], dtype=F64)
    return s[..., 0] - nw * s[..., 1] - bv * s[..., 2], s[..., 0].abs() + abs(nw) * s[..., 1].abs() + bv.abs() * s[..., 2].abs()


def finish(slab, weight, dzv, d, s, scale):
    """The closed form in the header comment of csrc/wgrad.hip: dW [Cout,Cin,taps] = scale * sum_k slab[k][tap][o][i]
    - scale^2 * W[o,i,tap] * sum_b dz[b,o] d[b,o]^2 s[b,i]^2 (the second term only where dzv is given): (the slab term, the
    demodulation term), to be added; handed |operands| they give the two term scales."""
    slab_term = scale * f64(slab).sum(0).permute(1, 2, 0)      # [splits][taps][o][i] -> [o][i][taps]
    if dzv is None:
        return slab_term, torch.zeros_like(slab_term)
    m = torch.einsum("bo,bi->oi", f64(dzv) * f64(d) ** 2, f64(s) ** 2)
    return slab_term, -(scale * scale) * f64(weight) * m.unsqueeze(2)


def finish_slab_k(splits):
    """modconv_wgrad_finish_kernel, the slab sum: a wave's interleaved quarter of the splits ceil(splits / 4), the four waves 3, scale * 1."""
    return -(-splits // 4) + 4


def finish_demod_k(form, batch):
    """The demodulation term: dz from the sums 4 (two products, two subtractions; 0 when dz is given), dz * d * d * s * s 4, the sum
    over the batch, scale * scale * W * m 3."""
    return (4 if form != "dz" else 0) + 4 + batch + 3


def wsq(weight, scale):
    """[Cout,Cin,taps] -> [Cout,Cin]: sum over the taps of (scale * W)^2 (its own term scale)."""
    return ((scale * f64(weight)) ** 2).sum(2)


def wsq_k(taps):
    """modconv_wsq_kernel: scale * W 1, counted twice in the square; the square 1; taps - 1 additions."""
    return taps + 2
