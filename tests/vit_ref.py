"""The CLIP transformer kernels of include/w2e_vit.h restated in plain torch float64 (CPU only): the GEMM with its prologue and epilogues,
LayerNorm forward (mean, rstd) and input gradient (+ add), the attention core and its gradient on the packed [B, L, 3, H, 64] layout,
the split-K slab sums, the QuickGELU pair and its derivative, and the K-quad-major packings (fp32 and fp16).  tests/test_vit_ref_host.py
holds this file to oracle/clip_model.py and to autograd; tests/test_gpu_vit_kernels.py holds the kernels to it.

Beside each function f:
  f_scale   the same formula on absolute values: the size of the terms that were rounded on the way to each output ELEMENT.  Where an
            output depends on an intermediate with an error of its own (the softmax on its logits, LayerNorm on its mean), the scale is
            the first-order propagation of that error; the derivation stands in the docstring.
  f_bound   N in  |got - ref| <= N * 2^-24 * scale,  counted from the kernel source: the number of dependent fp32 roundings on the
            longest chain to that output (a K-term contraction in any order with `splits` slab additions: K + splits + the epilogue).
            A bound may be a tensor (one N per element or per row) where the count depends on the data: __expf(x) is taken as
            (1.5 |x| + EXP_E) * 2^-24 relative -- the rounding of x * log2(e) carried through exp2, plus the exp2 instruction itself.
Every scale carries TINY = 2^-126 / 2^-24, so that N * 2^-24 * scale never asks for less than the fp32 underflow threshold (QuickGELU
of -100 is 1e-72 in float64 and 0 in fp32).  No element is excluded anywhere.

The two numbers nothing on a development machine can derive are named assumptions: RSQRT_ULP (device rsqrtf, as DESIGN.md already
assumes) and EXP2_ULP (the exp2 instruction behind __expf)."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126 / U
RSQRT_ULP = 2  # assumed: no statement of device rsqrtf's error was found in the ROCm headers / documents
EXP2_ULP = 1   # assumed: the accuracy of the hardware exp2 instruction __expf ends in (the ISA documents say 1 ulp; not measurable here)
EXP_E = 2 * EXP2_ULP  # an ulp is at most 2 * 2^-24 relative
F64 = torch.float64


def D(t):
    return None if t is None else torch.as_tensor(t).to(F64)


def expf_bound(x):
    """Relative error of __expf(x) in 2^-24: 1.5 |x| (x * log2(e) is rounded: an absolute error of |x| log2(e) 2^-24 in the argument of
    exp2, a relative one of |x| 2^-24 in its value; log2(e) itself is rounded: less than half as much again) + EXP_E."""
    return 1.5 * D(x).abs() + EXP_E


# ---------------------------------------------------------------------------------------------- QuickGELU
def qgelu(x):
    x = D(x)
    return x * torch.sigmoid(1.702 * x)


def _sig_bound(x, s):
    """s = 1 / (1 + __expf(-1.702f * x)): the product is rounded (relative 1 -> |1.702 x| relative in the exponential), __expf's own
    expf_bound, each weighted by d log s / d log e = 1 - s; the addition and the division: 2."""
    return (1.702 * x.abs() + expf_bound(1.702 * x)) * (1 - s) + 2


def qgelu_scale(x):
    return qgelu(x).abs() + TINY


def qgelu_bound(x):
    """x / (1 + e): the sigmoid's roundings; the value is one quotient, so the scale is the value."""
    x = D(x)
    return _sig_bound(x, torch.sigmoid(1.702 * x))


def qgelu_grad(x):
    x = D(x)
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x * (1 - s))


def qgelu_grad_scale(x):
    x = D(x)
    s = torch.sigmoid(1.702 * x)
    return s * (1 + 1.702 * x.abs() * (1 - s)) + TINY


def qgelu_grad_bound(x):
    """s (1 + 1.702 x (1 - s)) with s~ = s (1 + ds), ds = _sig_bound: t = 1 - s~ has the absolute error s ds + |t| (for large x, t is
    what the subtraction leaves of s's rounding: the cancellation is counted, not excluded); p = 1.702 x t: 1.702 |x| (s ds + 3 |t|);
    q = 1 + p: + |q|; s~ q: + ds + 1.  Relative to the scale s (1 + 1.702 |x| (1 - s)):
    N = ds + 2 + 1.702 |x| (s ds + 3 (1 - s)) / (1 + 1.702 |x| (1 - s))."""
    x = D(x)
    s = torch.sigmoid(1.702 * x)
    ds = _sig_bound(x, s)
    ax = 1.702 * x.abs()
    return ds + 2 + ax * (s * ds + 3 * (1 - s)) / (1 + ax * (1 - s))


# ---------------------------------------------------------------------------------------------- GEMM (w2e_gemm_ex)
def gemm_core(a, b, trans_b, a_gelu=False):
    """(pro(A) x B, the same on absolute values, the prologue's share of the error in 2^-24): the part of a case that its epilogue
    variants share.  B is [N,K] (trans_b) or [K,N]."""
    a, b = D(a), D(b)
    bt = b.t() if trans_b else b
    pa = qgelu(a) if a_gelu else a
    core, scale = pa @ bt, pa.abs() @ bt.abs()
    pro = (qgelu_bound(a) * pa.abs()) @ bt.abs() if a_gelu else None
    return core, scale, pro


def gemm(core, bias=None, residual=None, aux=None):
    """epi(core): + bias[N] + residual[M,N], then * QuickGELU'(aux[M,N])."""
    c = core[0] if isinstance(core, tuple) else core
    if bias is not None:
        c = c + D(bias)
    if residual is not None:
        c = c + D(residual)
    return c * qgelu_grad(aux) if aux is not None else c


def gemm_scale(core, bias=None, residual=None, aux=None):
    s = core[1] + TINY
    if bias is not None:
        s = s + D(bias).abs()
    if residual is not None:
        s = s + D(residual).abs()
    return s * qgelu_grad_scale(aux) if aux is not None else s


def gemm_bound(core, k, splits=1, aux=None):
    """K products accumulated in any order (four accumulators per output, merged: + 2) + one addition per K slice onto C (atomic or
    not) + bias + residual = K + splits + 4.  With the QuickGELU prologue each term |g(a)| |b| carries qgelu_bound(a) more: their
    sum relative to the scale.  With aux: the factor's own qgelu_grad_bound and the product (each slice multiplies its own partial)."""
    n = float(k + splits + 4)
    if core[2] is not None:
        n = n + core[2] / core[1].clamp_min(1e-300)
    if aux is not None:
        n = n + qgelu_grad_bound(aux) + 1
    return n


def gemm_split(k, want):
    """(splits, k_per) of w2e_gemm_ex for a requested split count: slices are multiples of 128, an empty last slice is dropped."""
    k_per = -(-(-(-k // max(want, 1))) // 128) * 128
    return -(-k // k_per), k_per


def gemm_cost_splits(m, n, k):
    """The split count w2e_gemm_ex's cost model picks (ldc == n, default options)."""
    tiles = -(-n // 64) * -(-m // 64)
    best, splits = 0.0, 1
    for sp in range(1, 17):
        kp = -(-(-(-k // sp)) // 128) * 128
        if sp > 1 and -(-k // kp) != sp:
            continue
        cost = -(-tiles * sp // 256) * ((kp // 64) * 0.9 + (3.2 if sp > 1 else 0.0)) + 2.0 + (3.0 if sp > 1 else 0.0)
        if sp == 1 or cost < best * 0.97:
            best, splits = cost, sp
    return splits


# ---------------------------------------------------------------------------------------------- split-K slabs
def slab_sum(part, bias=None, residual=None):
    """sum_s part[s] (+ bias[dim]) (+ residual): the slabs in ascending order (the order does not matter in float64)."""
    x = D(part).sum(0)
    if bias is not None:
        x = x + D(bias)
    return x + D(residual) if residual is not None else x


def slab_sum_scale(part, bias=None, residual=None):
    return slab_sum(D(part).abs(), None if bias is None else D(bias).abs(), None if residual is None else D(residual).abs()) + TINY


def slab_sum_bound(nsplit, bias=False, residual=False):
    """One addition per slab (the first, onto an exact zero, is exact: counted all the same) + bias + residual."""
    return nsplit + int(bool(bias)) + int(bool(residual))


def reduce_gelu(part, bias=None, aux=None, mode=0):
    """mode 0: (h, g) = (sum + bias, QuickGELU(h));  mode 1: sum * QuickGELU'(aux)."""
    if mode == 0:
        h = slab_sum(part, bias)
        return h, qgelu(h)
    return slab_sum(part) * qgelu_grad(aux)


def reduce_gelu_scale(part, bias=None, aux=None, mode=0):
    """mode 0, g: h's error (slab_sum_bound of its scale hs) passes through |QuickGELU'(h)| <= qgelu_grad_scale(h); the activation's own
    is relative to |g|: scale = hs * qgelu_grad_scale(h) + |g|."""
    if mode == 0:
        h, hs = slab_sum(part, bias), slab_sum_scale(part, bias)
        return hs, hs * qgelu_grad_scale(h) + qgelu_scale(h)
    return slab_sum_scale(part) * qgelu_grad_scale(aux)


def reduce_gelu_bound(nsplit, h=None, aux=None, mode=0):
    if mode == 0:
        n = slab_sum_bound(nsplit, True)
        return n, n + qgelu_bound(h)
    return slab_sum_bound(nsplit) + 1 + qgelu_grad_bound(aux)


# ---------------------------------------------------------------------------------------------- LayerNorm
def n_sum(dim):
    """Roundings on the longest chain of a row sum: ceil(dim / 64) accumulations of a lane (the float4 kernels: 2 + dim / 256, less)
    + the 6 levels of the wave's butterfly."""
    return -(-dim // 64) + 6


def ln_fwd(x, gamma, beta, eps):
    """y = (x - mean) * rstd * gamma + beta over the last dim, rstd = (var + eps)^-1/2, var about the mean: (y, mean, rstd)."""
    x = D(x)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = (d.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return d * rstd * D(gamma) + D(beta), mean.squeeze(-1), rstd.squeeze(-1)


def _ln_parts(x, eps, xs, n_in):
    x = D(x)
    xs = x.abs() if xs is None else D(xs)
    dim = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var_e = d.pow(2).mean(-1, keepdim=True) + eps
    ms = xs.mean(-1, keepdim=True) + TINY
    n_mean = n_in + n_sum(dim) + 1
    # var~ - var = 2 mean(d (dx + rho)) + Delta^2 to first order in the element errors dx (n_in of xs) and rho (the rounding of x - mean:
    # |d|), second order in the mean's error Delta (sum d = 0); + the squares, the sum, the division and the + eps: n_sum + 4
    n_var = (2 * n_in * (d.abs() * xs).mean(-1, keepdim=True) + (n_mean * ms) ** 2 * U) / var_e + n_sum(dim) + 6
    n_rstd = n_var / 2 + 2 * RSQRT_ULP + 1  # rsqrt halves a relative error; the instruction itself: RSQRT_ULP ulp
    return x, xs, d, var_e.rsqrt(), ms, n_mean, n_rstd


def ln_fwd_scale(x, gamma, beta, eps, xs=None, n_in=0):
    """mean: mean(xs).  rstd: itself.  y: d~ = x~ - mean~ has the absolute error n_in xs + n_mean mean(xs) + |d|, so the formula on
    absolute values is (xs + mean(xs) + |d|) rstd |gamma| + |beta| -- on a row with |mean| >> std that is far above |y|: the
    cancellation in x - mean is the algorithm's, and the scale says so.  xs / n_in: x is itself a rounded sum (the slab consumers)."""
    x, xs, d, rstd, ms, _, _ = _ln_parts(x, eps, xs, n_in)
    return (xs + ms + d.abs()) * rstd * D(gamma).abs() + D(beta).abs() + TINY, ms.squeeze(-1), rstd.squeeze(-1)


def ln_fwd_bound(x, eps, xs=None, n_in=0):
    """(N_y [rows,1], N_mean, N_rstd [rows]): y = d~ * rstd~ * gamma + beta: max(n_in, n_mean, n_rstd + 3) + 1."""
    _, _, _, _, _, n_mean, n_rstd = _ln_parts(x, eps, xs, n_in)
    return torch.clamp(n_rstd + 3, min=float(max(n_in, n_mean))) + 1, float(n_mean), n_rstd.squeeze(-1)


def ln_bwd(gy, x, gamma, mean, rstd, add=None):
    """gx = rstd * (g - mean(g) - xhat * mean(g * xhat)) (+ add), g = gy * gamma, xhat = (x - mean) * rstd, with the SAVED mean / rstd."""
    g, xh = D(gy) * D(gamma), (D(x) - D(mean).unsqueeze(-1)) * D(rstd).unsqueeze(-1)
    gx = D(rstd).unsqueeze(-1) * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return gx + D(add) if add is not None else gx


def ln_bwd_scale(gy, x, gamma, mean, rstd, add=None):
    """The formula on absolute values (gy may be the scale of a slab sum)."""
    g, xh = D(gy).abs() * D(gamma).abs(), ((D(x) - D(mean).unsqueeze(-1)) * D(rstd).unsqueeze(-1)).abs()
    s = D(rstd).abs().unsqueeze(-1) * (g + g.mean(-1, keepdim=True) + xh * (g * xh).mean(-1, keepdim=True)) + TINY
    return s + D(add).abs() if add is not None else s


def ln_bwd_bound(dim, n_in=0):
    """g: n_in + 1; xhat: 2; g * xhat: 1; the row sum and its division: n_sum + 1; xhat * s2: 1; the two subtractions: 2; * rstd, + add: 2."""
    return n_in + n_sum(dim) + 12


# ---------------------------------------------------------------------------------------------- attention
def _heads(qkv):
    b, l = qkv.shape[:2]
    q, k, v = D(qkv).reshape(b, l, 3, -1, 64).permute(2, 0, 3, 1, 4)  # [B,H,L,64] each
    return q, k, v


def _merge(o):
    b, h, l, _ = o.shape
    return o.transpose(1, 2).reshape(b, l, h * 64)


def _probs(q, k, causal):
    s = q @ k.transpose(-1, -2) / 8
    if causal:
        s = s + torch.full(s.shape[-2:], float("-inf"), dtype=F64).triu(1)
    return s, s.softmax(-1)


def attn_fwd(qkv, causal=False):
    """out[B, L, H*64] = softmax(Q K^T / 8 (+ the causal mask)) V per (batch, head); qkv [B, L, 3, H, 64] (any shape that views so)."""
    q, k, v = _heads(qkv)
    return _merge(_probs(q, k, causal)[1] @ v)


def _prob_error(q, k, qs, ks, n_in):
    """(P, relP): the relative error of P_ij in 2^-24.  S_ij = q_i . k_j / 8 has the absolute error ns * Ss_ij, Ss = qs . ks / 8 the
    logit's own term scale, ns = 64 + 2 n_in (64 products, the operands' own roundings; / 8 is exact).  w_ij = __expf(S_ij - mx): the
    subtraction (|S_ij - mx| relative in w) + expf_bound: e_ij = ns Ss_ij + 2.5 |S_ij - mx| + EXP_E.  P_ij = w_ij / sum_l w_il:
    d log P_ij = d log w_ij - sum_l P_il d log w_il, the row sum's L additions, the reciprocal and the product:
    relP_ij = e_ij + sum_l P_il e_il + L + 2."""
    s, p = _probs(q, k, False)
    ss = qs @ ks.transpose(-1, -2) / 8
    e = (64 + 2 * n_in) * ss + 2.5 * (s - s.amax(-1, keepdim=True)).abs() + EXP_E
    return p, e + (p * e).sum(-1, keepdim=True) + s.shape[-1] + 2


def attn_bound(seq, n_in=0):
    """The contraction over the L live columns or rows (the padding to 64 adds exact zeros) + the operand's own roundings + the 1/8."""
    return seq + n_in + 2


def attn_fwd_scale(qkv, qkv_s=None, n_in=0):
    """O_id = sum_j P_ij V_jd, first order: |dO_id| <= 2^-24 sum_j P_ij Vs_jd (N + relP_ij), N = attn_bound: the scale is
    sum_j P_ij Vs_jd (1 + relP_ij / N) -- P |V| times (1 + the logit error in units of its own term scale).  qkv_s / n_in: the
    operands are rounded slab sums of that scale."""
    q, k, v = _heads(qkv)
    qs, ks, vs = (q.abs(), k.abs(), v.abs()) if qkv_s is None else _heads(qkv_s)
    p, relp = _prob_error(q, k, qs, ks, n_in)
    return _merge((p * (1 + relp / attn_bound(q.shape[2], n_in))) @ vs) + TINY


def attn_bwd(qkv, gout):
    """gqkv [B, L, 3, H, 64] from gout [B, L, H*64]: dP = dO V^T, dS = P (dP - sum_j dP P), dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO."""
    q, k, v = _heads(qkv)
    b, h, l, _ = q.shape
    go = D(gout).reshape(b, l, h, 64).transpose(1, 2)
    _, p = _probs(q, k, False)
    dp = go @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    return torch.stack([ds @ k / 8, ds.transpose(-1, -2) @ q / 8, p.transpose(-1, -2) @ go], 0).permute(1, 3, 0, 2, 4).reshape(b, l, 3, h, 64)


def attn_bwd_scale(qkv, gout, qkv_s=None, gout_s=None, n_in=0, n_g=0):
    """With A_ij = |dP_ij| + sum_l P_il |dP_il| (the terms of dP_ij - dot_i), Ds = gos . vs (dP's term scale, nd = 64 + n_in + n_g
    roundings) and relP from the forward, the absolute error of dS_ij in 2^-24 is
      EdS_ij = P_ij [ relP_ij A_ij + nd Ds_ij + sum_l P_il (nd Ds_il + relP_il |dP_il|) + (L + 4) A_ij ]
    (P's error on the difference; dP's own; the same two inside the dot; the dot's L additions, the subtraction and the product).  Then
      dQ_id: sum_j (EdS_ij |K_jd| + N P_ij A_ij Ks_jd) / 8       dK_jd: sum_i (EdS_ij |Q_id| + N P_ij A_ij Qs_id) / 8
      dV_jd: sum_i P_ij Gs_id (N + relP_ij)                      N = attn_bound(L, n_in | n_g)
    each divided by its N to give the scale."""
    q, k, v = _heads(qkv)
    b, h, l, _ = q.shape
    qs, ks, vs = (q.abs(), k.abs(), v.abs()) if qkv_s is None else _heads(qkv_s)
    go = D(gout).reshape(b, l, h, 64).transpose(1, 2)
    gs = go.abs() if gout_s is None else D(gout_s).reshape(b, l, h, 64).transpose(1, 2)
    p, relp = _prob_error(q, k, qs, ks, n_in)
    dp, dsc = (go @ v.transpose(-1, -2)).abs(), gs @ vs.transpose(-1, -2)
    a = dp + (p * dp).sum(-1, keepdim=True)
    nd = 64 + n_in + n_g
    eds = p * (relp * a + nd * dsc + (p * (nd * dsc + relp * dp)).sum(-1, keepdim=True) + (l + 4) * a)
    n, ng = attn_bound(l, n_in), attn_bound(l, n_g)
    pa = p * a
    sq = (eds / n @ k.abs() + pa @ ks) / 8
    sk = (eds.transpose(-1, -2) / n @ q.abs() + pa.transpose(-1, -2) @ qs) / 8
    sv = (p * (1 + relp / ng)).transpose(-1, -2) @ gs
    return torch.stack([sq, sk, sv], 0).permute(1, 3, 0, 2, 4).reshape(b, l, 3, h, 64) + TINY


def attn_bwd_bound(seq, heads, n_in=0, n_g=0):
    """[3, H, 64] of N: dQ / dK by attn_bound(L, n_in), dV by attn_bound(L, n_g)."""
    t = torch.empty(3, heads, 64, dtype=F64)
    t[:2], t[2] = attn_bound(seq, n_in), attn_bound(seq, n_g)
    return t


# ---------------------------------------------------------------------------------------------- K-quad-major packings
def kq_pack(x, rows_padded):
    """X [rows, K] -> P [K/4, rows_padded, 4], P[q][r] = X[r][4q .. 4q+3], zero for r >= rows (w2e_pack_kq; any dtype, bit-exact)."""
    rows, k = x.shape
    p = torch.zeros(k // 4, rows_padded, 4, dtype=x.dtype)
    p[:, :rows] = x.reshape(rows, k // 4, 4).permute(1, 0, 2)
    return p


def kq_unpack(p, rows):
    return p[:, :rows].permute(1, 0, 2).reshape(rows, -1)


def kq_pack_h(x, rows_padded):
    """X [rows, K] -> fp16 PH [K/8, rows_padded, 8]: entry (2 s + h, r), component c holds X[r][16 s + 8 (c >> 2) + 4 h + (c & 3)]
    rounded to nearest even (w2e_pack_kq_h)."""
    rows, k = x.shape
    p = torch.zeros(k // 8, rows_padded, 8, dtype=torch.float16)
    p[:, :rows] = x.to(torch.float16).reshape(rows, k // 16, 2, 2, 4).permute(1, 3, 0, 2, 4).reshape(k // 8, rows, 8)
    return p


def kq_unpack_h(p, rows):
    k = p.shape[0] * 8
    return p[:, :rows].reshape(k // 16, 2, rows, 2, 4).permute(2, 0, 3, 1, 4).reshape(rows, k)


def pk_split(k, splits, depth=8):
    """(units per slice, admissible) of w2e_gemm_pk (depth 8: chunks) / w2e_gemm_pk_h (16: steps): slices are multiples of 4 units."""
    units = k // depth
    per = -(-(-(-units // splits)) // 4) * 4
    return per, 1 <= splits <= units and (splits - 1) * per < units


def gemm_pk_bound(k, splits, depth=8):
    """A slab is a contraction over its own slice of K, no epilogue: the terms of one slice (+ 1 for the test's float64 sum of slabs
    read back as fp32)."""
    return pk_split(k, splits, depth)[0] * depth + 1


# ---------------------------------------------------------------------------------------------- input families
def family(name, g, rows, cols):
    """A [rows, cols] fp32 input from the seeded CPU generator g.
    plain:       N(0,1).
    clip-like:   N(0,1) with one channel in 64 multiplied by 300 (the residual stream's massive channels), row 1 of mean 50 and
                 std 1, row 2 constant (3.0: every partial sum of the row is exact, so its variance is exactly 0).
    qgelu-wide:  half the elements uniform over [-100, 100], half N(0, 3^2), exact +0 and -0 planted."""
    x = torch.randn(rows, cols, generator=g)
    if name == "clip-like":
        x[:, 5 % cols::64] *= 300.0
        if rows > 1:
            x[1] = 50.0 + torch.randn(cols, generator=g)
        if rows > 2:
            x[2] = 3.0
    elif name == "qgelu-wide":
        wide = torch.rand(rows, cols, generator=g) * 200.0 - 100.0
        x = torch.where(torch.rand(rows, cols, generator=g) < 0.5, wide, 3.0 * x)
        flat = x.reshape(-1)
        flat[0] = 0.0
        if flat.numel() > 1:
            flat[1] = -0.0
        if flat.numel() > 3:
            flat[2], flat[3] = 100.0, -100.0
    else:
        assert name == "plain", name
    return x


def family_qkv(name, g, nsplit, b, l, heads):
    """(slabs [nsplit, B*L, 3*H*64], bias [3*H*64]) whose sum is the packed QKV.  clip-like: Q and K scaled by sqrt(10), so that the
    logits q . k / 8 ~ N(0, 10^2) span about +-30, and K of head 0 exactly zero in every slab and in the bias (a uniform softmax)."""
    d3 = 3 * heads * 64
    slabs = torch.randn(nsplit, b * l, d3, generator=g) / math.sqrt(nsplit)
    bias = torch.randn(d3, generator=g) * 0.3
    if name == "clip-like":
        slabs[:, :, :2 * heads * 64] *= math.sqrt(10.0)
        slabs[:, :, heads * 64:heads * 64 + 64] = 0.0
        bias[heads * 64:heads * 64 + 64] = 0.0
    else:
        assert name == "plain", name
    return slabs, bias


def family_weight(name, g, n, k):
    """A Linear weight [n, k]: plain N(0,1); clip-like: one OUTPUT channel in 64 multiplied by 300 -- the rows that make the residual
    stream's massive channels (the K axis stays plain: the massive terms of A meet ordinary weights)."""
    w = torch.randn(n, k, generator=g)
    if name == "clip-like":
        w[7 % n::64] *= 300.0
    return w


# ---------------------------------------------------------------------------------------------- the case tables (host and GPU tests)
GEMM_SHAPES = {1: [(1, 1, 4), (63, 65, 60), (64, 64, 128), (65, 129, 132), (200, 768, 3072)], 0: [(37, 68, 72), (130, 192, 260)]}
GEMM_EPILOGUES = [(), ("bias",), ("residual",), ("aux",), ("bias", "residual", "aux")]
GEMM_TUNE = [0, 2, 3, 16]                      # "tune_gemm_s": 0 = the cost model
GEMM_SPLIT_SHAPES = [(70, 132, 256), (70, 132, 260), (200, 768, 3072), (70, 132, 132)]  # two exact slices; a last slice 4 deep; K = 3072; 16 -> 2
LN_VEC_DIMS, LN_GENERIC_DIMS, LN_ROWS = [512, 768, 1024], [1, 3, 64, 100, 128, 2048], [1, 4, 5, 7]
ATTN_SEQ, ATTN_BH = [1, 2, 3, 4, 5, 49, 50, 63, 64], [(1, 1), (3, 2), (2, 12)]
ATTN2_NSPLIT, ATTN2_GSPLIT = [1, 3, 4, 7], [1, 6, 7]
REDUCE_DIMS, REDUCE_ROWS, REDUCE_NSPLIT = [512, 768, 1024], [1, 33], [1, 4, 5, 9]
PK_SHAPES, PK_H_K = [(1, 1, 8), (33, 65, 40), (32, 64, 32), (77, 200, 104), (200, 768, 768)], [16, 48, 80, 112, 768]
