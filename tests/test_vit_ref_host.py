"""tests/vit_ref.py held to the model and to itself, without a GPU.
(1) The restatement is the model: vit_ref composed into a residual block, visual and causal, equals oracle/clip_model.resblock in
    float64; its gradients equal float64 autograd of the stock torch composition; the packings round-trip.
(2) The bounds are not too tight: for the cases of tests/test_gpu_vit_kernels.py a straightforward torch fp32 evaluation of the same
    formula (the sum split into slabs where the kernel splits) stays within the bound at EVERY element.
(3) The bounds are not too loose: planted defects in that fp32 evaluation exceed the bound at some element; printed beside it whether
    the global criterion the earlier tests used (helpers.rel_err <= 1e-5) would have let the defect through."""
import pytest
import torch
import torch.nn.functional as F

import vit_ref as R
from helpers import rel_err
from oracle import clip_model as OC

U = R.U
F32 = torch.float32


def _gen(*key):
    return torch.Generator().manual_seed(7000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def worst(got, ref, scale, bound):
    """max over the elements of |got - ref| / (bound * 2^-24 * scale): <= 1 is within the bound."""
    got, ref = R.D(got), R.D(ref).reshape(got.shape)
    assert bool(torch.isfinite(got).all())
    bound = torch.as_tensor(bound, dtype=torch.float64)
    return float(((got - ref).abs() / (U * R.D(scale).reshape(got.shape) * bound)).max())


# ---------------------------------------------------------------------------------------------- (1) the restatement is the model
def _block_sd(g, dim):
    sd = {"b.ln_1.weight": 1 + 0.2 * torch.randn(dim, generator=g), "b.ln_1.bias": 0.2 * torch.randn(dim, generator=g),
          "b.ln_2.weight": 1 + 0.2 * torch.randn(dim, generator=g), "b.ln_2.bias": 0.2 * torch.randn(dim, generator=g)}
    for name, (n, k) in {"attn.in_proj_": (3 * dim, dim), "attn.out_proj.": (dim, dim), "mlp.c_fc.": (4 * dim, dim), "mlp.c_proj.": (dim, 4 * dim)}.items():
        sd["b." + name + "weight"], sd["b." + name + "bias"] = torch.randn(n, k, generator=g) * k ** -0.5, 0.1 * torch.randn(n, generator=g)
    return {k: v.double() for k, v in sd.items()}


def _ref_block(sd, x, heads, causal):
    """The residual block out of vit_ref's pieces, as the kernels compose it (tensors [B*L, dim])."""
    b, l, dim = x.shape
    x2 = x.reshape(b * l, dim)
    y1, mean1, rstd1 = R.ln_fwd(x2, sd["b.ln_1.weight"], sd["b.ln_1.bias"], 1e-5)
    qkv = R.gemm(R.gemm_core(y1, sd["b.attn.in_proj_weight"], True), sd["b.attn.in_proj_bias"])
    att = R.attn_fwd(qkv.reshape(b, l, -1), causal).reshape(b * l, dim)
    x_mid = R.gemm(R.gemm_core(att, sd["b.attn.out_proj.weight"], True), sd["b.attn.out_proj.bias"], x2)
    y2, mean2, rstd2 = R.ln_fwd(x_mid, sd["b.ln_2.weight"], sd["b.ln_2.bias"], 1e-5)
    h = R.gemm(R.gemm_core(y2, sd["b.mlp.c_fc.weight"], True), sd["b.mlp.c_fc.bias"])
    out = R.gemm(R.gemm_core(h, sd["b.mlp.c_proj.weight"], True, a_gelu=True), sd["b.mlp.c_proj.bias"], x_mid)
    return out.reshape(b, l, dim), (x2, mean1, rstd1, qkv, x_mid, mean2, rstd2, h)


def _ref_block_bwd(sd, saved, g, b, l, heads):
    """The backward of _ResBlock / _TransformerV3 in vit_ref's pieces."""
    x2, mean1, rstd1, qkv, x_mid, mean2, rstd2, h = saved
    gh = R.gemm(R.gemm_core(g, sd["b.mlp.c_proj.weight"], False), aux=h)
    gy2 = R.gemm(R.gemm_core(gh, sd["b.mlp.c_fc.weight"], False))
    g_mid = R.ln_bwd(gy2, x_mid, sd["b.ln_2.weight"], mean2, rstd2, add=g)
    ga = R.gemm(R.gemm_core(g_mid, sd["b.attn.out_proj.weight"], False))
    gqkv = R.attn_bwd(qkv.reshape(b, l, -1), ga.reshape(b, l, -1)).reshape(b * l, -1)
    gy1 = R.gemm(R.gemm_core(gqkv, sd["b.attn.in_proj_weight"], False))
    return R.ln_bwd(gy1, x2, sd["b.ln_1.weight"], mean1, rstd1, add=g_mid)


@pytest.mark.parametrize("causal", [False, True], ids=["visual", "causal"])
def test_restatement_is_the_oracles_residual_block(causal):
    g = _gen(1, causal)
    b, l, heads = 2, 7, 2
    dim = heads * 64
    sd = _block_sd(g, dim)
    x = torch.randn(b, l, dim, generator=g).double().requires_grad_(True)
    ref = OC.resblock(sd, "b", x, heads, causal)
    out, saved = _ref_block(sd, x.detach(), heads, causal)
    assert rel_err(out, ref.detach()) <= 1e-12
    if not causal:  # (the kernels have no causal backward: the text tower is forward only)
        r = torch.randn(b, l, dim, generator=g).double()
        (gref,) = torch.autograd.grad(ref, x, r)
        assert rel_err(_ref_block_bwd(sd, saved, r.reshape(b * l, dim), b, l, heads), gref.reshape(b * l, dim)) <= 1e-12


def test_pieces_against_float64_autograd_of_the_stock_composition():
    g = _gen(2)
    x = torch.randn(5, 100, generator=g).double().requires_grad_(True)
    gamma, beta, gy, add = (torch.randn(*s, generator=g).double() for s in ((100,), (100,), (5, 100), (5, 100)))
    y, mean, rstd = R.ln_fwd(x.detach(), gamma, beta, 1e-5)
    yr = F.layer_norm(x, (100,), gamma, beta, 1e-5)
    (gx,) = torch.autograd.grad(yr, x, gy)
    assert rel_err(y, yr.detach()) <= 1e-12 and rel_err(R.ln_bwd(gy, x.detach(), gamma, mean, rstd, add), gx + add) <= 1e-12
    a = torch.randn(6, 9, generator=g).double().requires_grad_(True)
    s = torch.sigmoid(1.702 * a)
    (ga,) = torch.autograd.grad((a * s).sum(), a)
    assert rel_err(R.qgelu(a.detach()), (a * s).detach()) <= 1e-12 and rel_err(R.qgelu_grad(a.detach()), ga) <= 1e-12
    qkv = torch.randn(2, 5, 3, 3, 64, generator=g).double().requires_grad_(True)
    go = torch.randn(2, 5, 192, generator=g).double()
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    ref = ((q @ k.transpose(-1, -2) / 8).softmax(-1) @ v).transpose(1, 2).reshape(2, 5, 192)
    (gq,) = torch.autograd.grad(ref, qkv, go)
    assert rel_err(R.attn_fwd(qkv.detach()), ref.detach()) <= 1e-12 and rel_err(R.attn_bwd(qkv.detach(), go), gq) <= 1e-12


def test_packings_round_trip_and_the_fp16_pack_is_the_documented_k_order():
    g = _gen(3)
    x = torch.randn(37, 48, generator=g)
    p = R.kq_pack(x, 64)
    assert p.shape == (12, 64, 4) and torch.equal(R.kq_unpack(p, 37), x) and float(p[:, 37:].abs().sum()) == 0.0
    assert torch.equal(p[3, 5], x[5, 12:16])
    ph = R.kq_pack_h(x, 64)
    assert ph.shape == (6, 64, 8) and ph.dtype == torch.float16 and torch.equal(R.kq_unpack_h(ph, 37), x.half())
    # tests/test_gpu_clip.py: the pack holds fp16(W) at k = 16 s + 8 (c >> 2) + 4 h + (c & 3) for entry (s, h), component c
    for s_, h_, c_ in ((0, 0, 0), (1, 1, 5), (2, 0, 7), (2, 1, 2)):
        assert ph[2 * s_ + h_, 9, c_] == x[9, 16 * s_ + 8 * (c_ >> 2) + 4 * h_ + (c_ & 3)].half()
    wr = ph[:, :37].float().reshape(48 // 16, 2, 37, 2, 4).permute(2, 0, 3, 1, 4).reshape(37, 48)  # that file's own unpacking
    assert torch.equal(wr, x.half().float())


# ---------------------------------------------------------------------------------------------- the fp32 evaluations (and the defects)
def f32_qgelu(x):
    return x / (1 + torch.exp(-1.702 * x))


def f32_qgelu_grad(x, defect=None):
    if defect in ("y >= 0", "y > 0"):  # the sign-split sigmoid some kernels use: the two comparisons differ at x == 0 only, where both give 1/2
        pos = x >= 0 if defect == "y >= 0" else x > 0
        e = torch.exp(-1.702 * x.abs())
        s = torch.where(pos, 1 / (1 + e), e / (1 + e))
    else:
        s = 1 / (1 + torch.exp(-1.702 * x))
    return s * (1 + 1.702 * x * (1 - s))


def f32_gemm(a, b, trans_b, a_gelu=False, bias=None, residual=None, aux=None, want=1, defect=None, ldc=None):
    """C as w2e_gemm_ex computes it, in torch fp32: K in slices of k_per, slice 0 carries bias + residual, every slice multiplies its
    own partial by QuickGELU'(aux) and is added onto C."""
    m, k = a.shape
    splits, k_per = R.gemm_split(k, want)
    bt = b.t() if trans_b else b
    pa = f32_qgelu(a) if a_gelu else a.clone()
    whole = None
    if defect == "one K quad dropped from one output row":  # ... of one wave's 32-column block (columns 32 .. 63, where there are as many)
        whole = f32_gemm(a, b, trans_b, a_gelu, bias, residual, aux, want)
        pa[m // 2, 4 * ((k // 4) // 2):4 * ((k // 4) // 2) + 4] = 0.0
    if defect == "residual read at stride n instead of ldc":
        n = bt.shape[1]
        flat = torch.zeros(m, ldc).reshape(-1)
        flat[:] = float("nan")
        full = flat.reshape(m, ldc)
        full[:, :n] = residual
        full[:, n:] = 0.5  # (what a gap would hold)
        residual = full.reshape(-1)[:m * n].reshape(m, n)
    c = torch.zeros(m, bt.shape[1])
    for z in range(splits):
        sl = slice(z * k_per, min(k, (z + 1) * k_per))
        v = pa[:, sl] @ bt[sl]
        if bias is not None and (z == 0 or defect == "bias added by every slab instead of once"):
            v = v + bias
        if residual is not None and z == 0:
            v = v + residual
        if aux is not None:
            v = v * f32_qgelu_grad(aux)
        c = c + v
    if whole is not None and c.shape[1] > 32:
        whole[m // 2, 32:64] = c[m // 2, 32:64]
        return whole
    return c


def f32_slab_sum(part, bias=None, residual=None):
    x = torch.zeros_like(part[0])
    for s in range(part.shape[0]):
        x = x + part[s]
    if bias is not None:
        x = x + bias
    return x + residual if residual is not None else x


def f32_ln_fwd(x, gamma, beta, eps, defect=None):
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    d = x - mean
    var = ((x if defect == "variance about 0" else d).pow(2)).sum(-1, keepdim=True) / x.shape[-1]
    rstd = (var + eps).rsqrt()
    return d * rstd * gamma + beta, mean.squeeze(-1), rstd.squeeze(-1)


def f32_ln_bwd(gy, x, gamma, mean, rstd, add=None):
    g, xh = gy * gamma, (x - mean.unsqueeze(-1)) * rstd.unsqueeze(-1)
    dim = x.shape[-1]
    gx = rstd.unsqueeze(-1) * (g - g.sum(-1, keepdim=True) / dim - xh * ((g * xh).sum(-1, keepdim=True) / dim))
    return gx + add if add is not None else gx


def _f32_probs(q, k, defect):
    s = q @ k.transpose(-1, -2) * 0.125
    l = s.shape[-1]
    if defect == "softmax over roundup4(L) columns":
        s = F.pad(s, (0, -l % 4))  # the padded K rows are zero: logit 0
    w = torch.exp(s - s.amax(-1, keepdim=True))
    return (w * (1 / w.sum(-1, keepdim=True)))[..., :l]


def f32_attn_fwd(qkv, defect=None):
    b, l = qkv.shape[:2]
    q, k, v = qkv.reshape(b, l, 3, -1, 64).permute(2, 0, 3, 1, 4)
    return (_f32_probs(q, k, defect) @ v).transpose(1, 2).reshape(b, l, -1)


def f32_attn_bwd(qkv, gout, defect=None):
    b, l = qkv.shape[:2]
    q, k, v = qkv.reshape(b, l, 3, -1, 64).permute(2, 0, 3, 1, 4)
    go = gout.reshape(b, l, -1, 64).transpose(1, 2)
    p = _f32_probs(q, k, None)
    dp = go @ v.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dk = ds.transpose(-1, -2) @ q * (1.0 if defect == "dK without its 1/8" else 0.125)
    return torch.stack([ds @ k * 0.125, dk, p.transpose(-1, -2) @ go], 0).permute(1, 3, 0, 2, 4).reshape(b, l, 3, -1, 64)


def f32_gemm_pk(a, w, splits, depth=8, defect=None):
    """The slabs of w2e_gemm_pk (depth 8) / w2e_gemm_pk_h (depth 16: operands rounded to fp16, products and sums in fp32)."""
    m, k = a.shape
    per = R.pk_split(k, splits, depth)[0] * depth
    if depth == 16:
        a, w = a.half().float(), w.half().float()
    c = torch.stack([a[:, z * per:min(k, (z + 1) * per)] @ w[:, z * per:min(k, (z + 1) * per)].t() for z in range(splits)])
    if defect == "the two lane halves' quads swapped for one chunk":
        # chunk ch = quads 2 ch (lane half 0) and 2 ch + 1 (half 1); swapped in the SECOND B operand of the first wave only (the 32
        # rows x columns 32 .. 63 it accumulates in acc1), or, where the matrix has no such columns, in all it has
        ch = min((k // 8) // 2 | 1, k // 8 - 1)
        ws = w.clone()
        ws[:, 8 * ch:8 * ch + 8] = torch.cat([w[:, 8 * ch + 4:8 * ch + 8], w[:, 8 * ch:8 * ch + 4]], 1)
        bad = torch.stack([a[:, z * per:min(k, (z + 1) * per)] @ ws[:, z * per:min(k, (z + 1) * per)].t() for z in range(splits)])
        cols = slice(32, 64) if w.shape[0] > 32 else slice(0, w.shape[0])
        c[:, :32, cols] = bad[:, :32, cols]
    return c


# ---------------------------------------------------------------------------------------------- (2) the bounds are not too tight
def _gemm_inputs(fam, m, n, k, trans_b, seed=0):
    g = _gen(m, n, k, trans_b, len(fam), seed)
    a = R.family("plain" if fam == "qgelu-wide" else fam, g, m, k)
    w = R.family_weight(fam, g, n, k)
    b = w if trans_b else w.t().contiguous()
    bias, res, aux = torch.randn(n, generator=g), R.family("plain", g, m, n), R.family("qgelu-wide" if fam == "qgelu-wide" else "plain", g, m, n)
    return a, b, bias, res, aux


@pytest.mark.parametrize("fam", ["plain", "clip-like"])
@pytest.mark.parametrize("trans_b", [1, 0])
def test_fp32_gemm_stays_within_the_bound(trans_b, fam):
    for m, n, k in R.GEMM_SHAPES[trans_b] + [s_ for s_ in R.GEMM_SPLIT_SHAPES if s_ not in R.GEMM_SHAPES[trans_b]]:
        a, b, bias, res, aux = _gemm_inputs(fam, m, n, k, trans_b)
        core = R.gemm_core(a, b, trans_b)
        for epi in R.GEMM_EPILOGUES:
            kw = dict(bias=bias if "bias" in epi else None, residual=res if "residual" in epi else None, aux=aux if "aux" in epi else None)
            for want in (1, 2, 3, 16):
                splits = R.gemm_split(k, want)[0]
                w_ = worst(f32_gemm(a, b, trans_b, want=want, **kw), R.gemm(core, **kw), R.gemm_scale(core, **kw), R.gemm_bound(core, k, splits, kw["aux"]))
                assert w_ <= 1.0, (m, n, k, epi, want, w_)


def test_fp32_gemm_with_the_quickgelu_prologue_and_wide_arguments_stays_within_the_bound():
    for m, n, k in R.GEMM_SHAPES[1] + [s_ for s_ in R.GEMM_SPLIT_SHAPES if s_ not in R.GEMM_SHAPES[1]]:
        g = _gen(m, n, k, 5)
        a, w = R.family("qgelu-wide", g, m, k), R.family_weight("plain", g, n, k)
        bias, res, aux = torch.randn(n, generator=g), R.family("plain", g, m, n), R.family("qgelu-wide", g, m, n)
        core = R.gemm_core(a, w, True, a_gelu=True)
        for kw in (dict(), dict(aux=aux), dict(bias=bias, residual=res), dict(bias=bias, residual=res, aux=aux)):
            for want in (1, 2, 3, 16):
                w_ = worst(f32_gemm(a, w, True, a_gelu=True, want=want, **kw), R.gemm(core, **kw), R.gemm_scale(core, **kw),
                           R.gemm_bound(core, k, R.gemm_split(k, want)[0], kw.get("aux")))
                assert w_ <= 1.0, (m, n, k, list(kw), want, w_)
    x = R.family("qgelu-wide", _gen(6), 64, 3072)
    assert worst(f32_qgelu(x), R.qgelu(x), R.qgelu_scale(x), R.qgelu_bound(x)) <= 1.0
    assert worst(f32_qgelu_grad(x), R.qgelu_grad(x), R.qgelu_grad_scale(x), R.qgelu_grad_bound(x)) <= 1.0
    assert torch.equal(f32_qgelu_grad(x, "y >= 0"), f32_qgelu_grad(x, "y > 0")), "`>=` for `>` must make no difference"
    assert int((x == 0).sum()) >= 2


@pytest.mark.parametrize("fam", ["plain", "clip-like"])
def test_fp32_layernorm_stays_within_the_bounds(fam):
    for dim in R.LN_VEC_DIMS + R.LN_GENERIC_DIMS:
        for rows in R.LN_ROWS:
            g = _gen(dim, rows, len(fam))
            x, gy, add = R.family(fam, g, rows, dim), R.family("plain", g, rows, dim), R.family("plain", g, rows, dim)
            gamma, beta = 1 + 0.2 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g)
            y, mean, rstd = f32_ln_fwd(x, gamma, beta, 1e-5)
            refs, scales, bounds = R.ln_fwd(x, gamma, beta, 1e-5), R.ln_fwd_scale(x, gamma, beta, 1e-5), R.ln_fwd_bound(x, 1e-5)
            for got, r, s, n in zip((y, mean, rstd), refs, scales, bounds):
                assert worst(got, r, s, n) <= 1.0, (dim, rows)
            for ad in (None, add):
                gx = f32_ln_bwd(gy, x, gamma, mean, rstd, ad)
                assert worst(gx, R.ln_bwd(gy, x, gamma, mean, rstd, ad), R.ln_bwd_scale(gy, x, gamma, mean, rstd, ad), R.ln_bwd_bound(dim)) <= 1.0, (dim, rows)


@pytest.mark.parametrize("fam", ["plain", "clip-like"])
def test_fp32_slab_consumers_stay_within_the_bounds(fam):
    for dim in R.REDUCE_DIMS:
        for rows in R.REDUCE_ROWS:
            for nsplit in R.REDUCE_NSPLIT:
                g = _gen(dim, rows, nsplit, len(fam))
                part = torch.stack([R.family(fam, g, rows, dim) for _ in range(nsplit)]) / nsplit
                bias, res, gamma, beta = torch.randn(dim, generator=g), R.family("plain", g, rows, dim), 1 + 0.2 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g)
                x = f32_slab_sum(part, bias, res)
                xr, xs, n_in = R.slab_sum(part, bias, res), R.slab_sum_scale(part, bias, res), R.slab_sum_bound(nsplit, True, True)
                assert worst(x, xr, xs, n_in) <= 1.0
                y, mean, rstd = f32_ln_fwd(x, gamma, beta, 1e-5)
                refs, scales, bounds = R.ln_fwd(xr, gamma, beta, 1e-5), R.ln_fwd_scale(xr, gamma, beta, 1e-5, xs, n_in), R.ln_fwd_bound(xr, 1e-5, xs, n_in)
                for got, r, s, n in zip((y, mean, rstd), refs, scales, bounds):
                    assert worst(got, r, s, n) <= 1.0, (dim, rows, nsplit)
                gx = f32_ln_bwd(f32_slab_sum(part), x, gamma, mean, rstd, res)
                assert worst(gx, R.ln_bwd(R.slab_sum(part), x, gamma, mean, rstd, res), R.ln_bwd_scale(R.slab_sum_scale(part), x, gamma, mean, rstd, res),
                             R.ln_bwd_bound(dim, nsplit)) <= 1.0, (dim, rows, nsplit)
    for n in (4, 3072):
        for nsplit in R.REDUCE_NSPLIT:
            g = _gen(n, nsplit, 9)
            part = torch.stack([R.family("qgelu-wide", g, 33, n) for _ in range(nsplit)]) / nsplit
            bias, aux = torch.randn(n, generator=g), R.family("qgelu-wide", g, 33, n)
            h = f32_slab_sum(part, bias)
            (hr, gr), (hs, gs) = R.reduce_gelu(part, bias), R.reduce_gelu_scale(part, bias)
            nh, ng = R.reduce_gelu_bound(nsplit, hr)
            assert worst(h, hr, hs, nh) <= 1.0 and worst(f32_qgelu(h), gr, gs, ng) <= 1.0, (n, nsplit)
            out = f32_slab_sum(part) * f32_qgelu_grad(aux)
            assert worst(out, R.reduce_gelu(part, aux=aux, mode=1), R.reduce_gelu_scale(part, aux=aux, mode=1), R.reduce_gelu_bound(nsplit, aux=aux, mode=1)) <= 1.0


@pytest.mark.parametrize("fam", ["plain", "clip-like"])
def test_fp32_attention_stays_within_the_bounds(fam):
    for l in R.ATTN_SEQ:
        for b, h in R.ATTN_BH:
            for nsplit, gsplit in ((ns, gs_) for ns in R.ATTN2_NSPLIT for gs_ in R.ATTN2_GSPLIT):
                g = _gen(l, b, h, nsplit, gsplit, len(fam))
                slabs, bias = R.family_qkv(fam, g, nsplit, b, l, h)
                gs = torch.randn(gsplit, b * l, h * 64, generator=g) / gsplit
                qkv, go = f32_slab_sum(slabs, bias).reshape(b, l, -1), f32_slab_sum(gs).reshape(b, l, -1)
                qr, qs, gr, gss = R.slab_sum(slabs, bias).reshape(b, l, -1), R.slab_sum_scale(slabs, bias).reshape(b, l, -1), R.slab_sum(gs).reshape(b, l, -1), R.slab_sum_scale(gs).reshape(b, l, -1)
                n_in = R.slab_sum_bound(nsplit, True)
                assert worst(f32_attn_fwd(qkv), R.attn_fwd(qr), R.attn_fwd_scale(qr, qs, n_in), R.attn_bound(l, n_in)) <= 1.0, (l, b, h, nsplit)
                bound = R.attn_bwd_bound(l, h, n_in, gsplit).expand(b, l, 3, h, 64)
                assert worst(f32_attn_bwd(qkv, go), R.attn_bwd(qr, gr), R.attn_bwd_scale(qr, gr, qs, gss, n_in, gsplit), bound) <= 1.0, (l, b, h, nsplit)


def test_fp32_packed_gemm_stays_within_the_bound():
    for m, n, k in R.PK_SHAPES + [(77, 200, kk) for kk in R.PK_H_K]:
        for depth in (8, 16):
            if k % depth:
                continue
            g = _gen(m, n, k, depth)
            a, w = R.family("clip-like", g, m, k), R.family_weight("clip-like", g, n, k) * (k ** -0.5 if depth == 16 else 1.0)
            core = R.gemm_core(a.half() if depth == 16 else a, w.half() if depth == 16 else w, True)
            for sp in range(1, k // depth + 1):
                if not R.pk_split(k, sp, depth)[1]:
                    continue
                got = f32_gemm_pk(a, w, sp, depth).double().sum(0)
                assert worst(got, core[0], core[1] + R.TINY, R.gemm_pk_bound(k, sp, depth)) <= 1.0, (m, n, k, depth, sp)


# ---------------------------------------------------------------------------------------------- (3) the bounds are not too loose
GLOBAL_TOL = 1e-5  # what tests/test_gpu_clip.py holds these kernels to: helpers.rel_err, max |a - b| / max |b| over the whole tensor


def _gemm_defect(defect):
    out = []
    for trans_b in (1, 0):
        for m, n, k in R.GEMM_SHAPES[trans_b] + R.GEMM_SPLIT_SHAPES[:2]:
            a, b, bias, res, _ = _gemm_inputs("clip-like", m, n, k, trans_b)
            core = R.gemm_core(a, b, trans_b)
            want = 3 if defect.startswith("bias") else 1
            if defect.startswith("bias") and R.gemm_split(k, want)[0] == 1:
                continue
            got = f32_gemm(a, b, trans_b, bias=bias, residual=res, want=want, defect=defect, ldc=n + 8)
            ref = R.gemm(core, bias, res)
            out.append(((m, n, k, trans_b), worst(got, ref, R.gemm_scale(core, bias, res), R.gemm_bound(core, k, R.gemm_split(k, want)[0])), rel_err(got, ref)))
    return out


def _pk_defect(defect):
    out = []
    for m, n, k in R.PK_SHAPES:
        g = _gen(m, n, k, 8)
        a, w = R.family("clip-like", g, m, k), R.family_weight("clip-like", g, n, k)
        core = R.gemm_core(a, w, True)
        got = f32_gemm_pk(a, w, 1, defect=defect).double().sum(0)
        out.append(((m, n, k), worst(got, core[0], core[1] + R.TINY, R.gemm_pk_bound(k, 1)), rel_err(got, core[0])))
    return out


def _softmax_defect(defect):
    out = []
    for l in R.ATTN_SEQ:
        for b, h in R.ATTN_BH:
            g = _gen(l, b, h, 1, len("clip-like"))
            slabs, bias = R.family_qkv("clip-like", g, 1, b, l, h)
            qkv = (slabs[0] + bias).reshape(b, l, 3, h, 64)
            got, ref = f32_attn_fwd(qkv, defect), R.attn_fwd(qkv)
            out.append(((l, b, h), worst(got, ref, R.attn_fwd_scale(qkv), R.attn_bound(l)), rel_err(got, ref)))
    return out


def _dk_defect(defect):
    out = []
    for l in R.ATTN_SEQ:
        g = _gen(l, 3, 2, 1, 5)
        slabs, bias = R.family_qkv("plain", g, 1, 3, l, 2)
        qkv, go = (slabs[0] + bias).reshape(3, l, 3, 2, 64), torch.randn(3, l, 128, generator=g)
        got, ref = f32_attn_bwd(qkv, go, defect), R.attn_bwd(qkv, go)
        out.append(((l, 3, 2), worst(got, ref, R.attn_bwd_scale(qkv, go), R.attn_bwd_bound(l, 2).expand(3, l, 3, 2, 64)), rel_err(got, ref)))
    return out


def _ln_defect(defect):
    out = []
    for dim in R.LN_VEC_DIMS + R.LN_GENERIC_DIMS[1:]:
        g = _gen(dim, 5, len("clip-like"))
        x = R.family("clip-like", g, 5, dim)
        gamma, beta = 1 + 0.2 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g)
        assert abs(float(x[1].mean())) > 20 * float(x[1].std())
        got, ref = f32_ln_fwd(x, gamma, beta, 1e-5, defect)[0], R.ln_fwd(x, gamma, beta, 1e-5)[0]
        out.append(((5, dim), worst(got, ref, R.ln_fwd_scale(x, gamma, beta, 1e-5)[0], R.ln_fwd_bound(x, 1e-5)[0]), rel_err(got, ref)))
    return out


DEFECTS = {
    "one K quad dropped from one output row": _gemm_defect,
    "the two lane halves' quads swapped for one chunk": _pk_defect,
    "bias added by every slab instead of once": _gemm_defect,
    "residual read at stride n instead of ldc": _gemm_defect,
    "softmax over roundup4(L) columns": _softmax_defect,
    "variance about 0": _ln_defect,
    "dK without its 1/8": _dk_defect,
}
# The defects the global criterion lets through at one of the listed shapes at least -- a property of these CPU evaluations and inputs,
# not of any kernel.  The other four change a whole head, row or 32 x 32 block by a share of its own size (the swapped quads meet the
# row of mean 50): max |a - b| / max |b| sees them at every listed shape (the swap at 2.6e-5 ... 9.5e-5), and so did the earlier tests.
MISSED_BY_THE_GLOBAL_CRITERION = {"one K quad dropped from one output row", "bias added by every slab instead of once",
                                  "residual read at stride n instead of ldc"}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_planted_defect_exceeds_the_element_bound(defect):
    rows = DEFECTS[defect](defect)
    assert rows
    caught = [r for r in rows if r[1] > 1.0]
    hidden = [r for r in caught if r[2] <= GLOBAL_TOL]
    for shape, w_, e in rows:
        print(f"{defect} {shape}: worst element {w_:.3g} x its bound, global rel err {e:.2e}" + (" -- MISSED by the global criterion" if w_ > 1.0 and e <= GLOBAL_TOL else ""))
    print(f"defect '{defect}': caught by the element bound at {len(caught)} of {len(rows)} shapes; "
          + (f"the global criterion (rel err <= {GLOBAL_TOL}) would have MISSED it at {[r[0] for r in hidden]}" if hidden else "the global criterion sees it too"))
    assert caught, f"no listed shape shows '{defect}' at any element"
    if defect in MISSED_BY_THE_GLOBAL_CRITERION:
        assert hidden, f"'{defect}' is expected to pass the global criterion at one listed shape at least"
