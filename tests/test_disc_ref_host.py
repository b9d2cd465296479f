"""CPU checks of tests/disc_ref.py, the yardstick of tests/test_gpu_disc_kernels.py: every float64 restatement against float64 autograd
of an independent statement of the same layer (tests/disc64.py, _mbstd64, tests/r1_ref.py, oracle/stylegan2.py), the fp32 restatements
of the stddev kernels inside the bounds the kernels are held to on every committed shape, and the shape lists reaching what they say.

The float64 routes differ in summation order only.  Measured here, in units of the term scale: fromRGB 1.1e-15 (y 5.7e-16, gx 1.1e-15,
dw 9.3e-16, db 0, tangent 5.0e-16), the stddev layer 3.2e-16 (y 3.2e-16, gx 2.1e-16, tangent 1.2e-17, mu 5.0e-17), the finish closed
form 1.6e-15.  Every comparison asserts 1e-14 and prints what it measured.  The fp32 restatement of the stddev kernels measured at most
0.94 (s), 0.66 (the stddev part of gx), 0.98 (gx), 0.19 (tangent) and 0.73 (mu) roundings of T against K of 5.5 ... 65; the
cotangent sum's cabs / |coef| reaches 359 on the committed seeds and is charged to the coefficient's own sum only (disc_ref.mbstd_scales)."""
import math

import pytest
import torch
from torch.nn import functional as F

import disc64
import disc_ref as R
import r1_ref
from oracle import stylegan2 as OG
from test_gpu_discriminator import _mbstd64

AGREE = 1e-14   # of the term scale, between two float64 routes (measured: module docstring)


def _agree(a, b, scale, what):
    e = float(((a - b).abs() / scale.clamp_min(1e-300)).max())
    print(f"{what}: two float64 routes differ by {e:.2e} of the term scale")
    assert e <= AGREE, what
    return e


# ---------------------------------------------------------------------------------------------- fromRGB
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("b,c,hw", [(1, 1, 1), (3, 5, 37), (2, 64, 130)])
def test_fromrgb_reference_is_float64_autograd_of_the_layer(b, c, hw, bias):
    """disc64's ConvLayer(3, C, 1) (EqualConv2d scaled by 1 / sqrt(3), FusedLeakyReLU) differentiated by autograd; the masks of the
    backward and of the tangent come from the output y, whose sign is the pre-activation's."""
    key = f"host.fr.{b}.{c}.{hw}"
    x, w, gy, dx = (R.heavy(key + k, s).double() for k, s in (("x", (b, 3, hw)), ("w", (c, 3)), ("gy", (b, c, hw)), ("dx", (b, 3, hw))))
    bv = R.heavy(key + "b", (c,)).double() if bias else torch.zeros(c, dtype=torch.float64)
    scale = 1.0 / math.sqrt(3.0)
    xx, ww, bb = x.clone().requires_grad_(), w.clone().requires_grad_(), bv.clone().requires_grad_()

    def layer(xi):
        return disc64._act(disc64._conv(xi.unsqueeze(3), ww.view(c, 3, 1, 1), 1, 0), bb).squeeze(3)

    y = layer(xx)
    y_ref, t = R.fromrgb_fwd(x, w, bv if bias else None, scale)
    _agree(y_ref, y.detach(), t, "fromrgb y")
    assert bool((t > 0).all()) or c * hw == 1
    gx, dw, db = torch.autograd.grad(y, [xx, ww, bb], gy)
    (rx, rw, rb), (sx, sw, sb) = R.fromrgb_bwd(gy, y.detach(), x, w, scale)
    _agree(rx, gx, sx, "fromrgb gx")
    _agree(rw, dw, sw, "fromrgb dw")
    _agree(rb, db, sb, "fromrgb db")
    _, tangent = torch.autograd.functional.jvp(layer, (x,), (dx,))
    jt, js = R.fromrgb_jvp(dx, y.detach(), w, scale)
    _agree(jt, tangent, js, "fromrgb tangent")


def test_fromrgb_masks_put_both_zeros_on_the_small_slope():
    y = torch.tensor([[[0.0, -0.0, 1.0, -1.0]]])
    g = R.gpre(torch.ones(1, 1, 4), y)
    assert torch.equal(g, torch.tensor([[[0.2, 0.2, 1.0, 0.2]]], dtype=torch.float64) * R.SQRT2)
    t, _ = R.fromrgb_jvp(torch.ones(1, 3, 4), y, torch.ones(1, 3), 1.0)
    assert torch.equal(t, torch.tensor([[[0.2, 0.2, 1.0, 0.2]]], dtype=torch.float64) * R.SQRT2 * 3.0)
    lay = R.layer_output("host.layer", (4, 64))
    zeros = lay[lay == 0]
    assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all()) and bool((lay > 0).any()) and bool((lay < 0).any())


# ---------------------------------------------------------------------------------------------- the stddev layer
MB_HOST = [(b, c, hw) for b in R.MBSTD_BATCHES for (c, hw) in ((3, 5), (7, 37), (1, 1))] + [(4, 512, 16), (12, 3, 100)]


@pytest.mark.parametrize("family", list(R.FAMILIES))
@pytest.mark.parametrize("b,c,hw", MB_HOST)
def test_mbstd_reference_is_float64_autograd(b, c, hw, family):
    """Forward and backward against autograd of _mbstd64 (the layer as tests/disc64.py states it); the tangent and the Hessian-vector
    product against r1_ref.stddev_jvp_hvp (the double-vjp trick) and against torch.autograd.functional.jvp / a second grad."""
    x, dx, gy = (t.double() for t in R.mbstd_inputs(family, b, c, hw))
    n = c * hw
    xx = x.view(b, c, hw, 1).clone().requires_grad_()
    y = _mbstd64(xx)
    _agree(R.mbstd_fwd(x), y.detach().squeeze(3), R.mbstd_fwd(x.abs()).clamp_min(1e-30), "mbstd y")
    sc = R.mbstd_scales(x, gy, dx)
    (gx,) = torch.autograd.grad(y, xx, gy.view(b, c + 1, hw, 1))
    ref_gx, part = R.mbstd_bwd(gy, x)
    _agree(ref_gx, gx.squeeze(3), gy[:, :c].abs() + sc["gx"], "mbstd gx")
    lam = gy[:, c].sum(1)
    jv64, mu64 = r1_ref.stddev_jvp_hvp(x.view(b, c, hw, 1), dx.view(b, c, hw, 1), lam)
    group = R.mbstd_group(b)
    jv = R.mbstd_jvp(x, dx)
    _agree(jv.repeat(group), jv64, sc["jv"].repeat(group), "mbstd tangent (double vjp)")
    mu = R.mbstd_hvp(gy, x, dx)
    if group > 1:
        _agree(mu, mu64.squeeze(3), sc["mu"], "mbstd mu (double vjp)")
    else:
        assert not bool(mu.any()) and not bool(mu64.any()) and not bool(part.any()) and not bool(jv.any())
    # the second route: forward-mode for the tangent, then a plain gradient of <lam, tangent>
    xs = x.clone().requires_grad_()
    _, tan = torch.autograd.functional.jvp(lambda t: r1_ref.stddev(t.view(b, c, hw, 1)), (xs,), (dx,), create_graph=True)
    _agree(jv.repeat(group), tan.detach(), sc["jv"].repeat(group), "mbstd tangent (functional.jvp)")
    if group > 1:
        (mu2,) = torch.autograd.grad((tan * lam).sum(), xs)
        _agree(mu, mu2, sc["mu"], "mbstd mu (second grad)")
    assert n == x[0].numel()


@pytest.mark.parametrize("family", list(R.FAMILIES))
@pytest.mark.parametrize("c,hw", list(R.MBSTD_SHAPES))
@pytest.mark.parametrize("b", R.MBSTD_BATCHES)
def test_fp32_restatement_of_the_stddev_kernels_is_inside_every_bound(b, c, hw, family):
    """The condition the reference alone must pass: the kernels' own operation order in fp32 on the CPU, every element inside
    K * 2^-24 * T on every committed shape and both families; at group 1 the exact zeros the kernels are asked for."""
    x, dx, gy = R.mbstd_inputs(family, b, c, hw)
    group = R.mbstd_group(b)
    sc = R.mbstd_scales(x, gy, dx)
    gs = gy.clone()
    gs[:, :c] = 0

    def worst(got, ref, scale, k, what):
        r = float(((got.double() - ref).abs() / (k * R.U * scale).clamp_min(1e-300)).max())
        print(f"fp32 restatement {what} [b{b} {c}x{hw} {family}]: {r * k:.3f} roundings of T, {r:.4f} of the bound (K = {k:g})")
        assert r <= 1.0, what
    worst(R.mbstd_value32(x), R.mbstd_value(x), sc["s"], R.mbstd_s_k(group, c, hw), "s")
    worst(R.mbstd_bwd32(gs, x), R.mbstd_bwd(gs, x)[1], sc["gx"], R.mbstd_gx_k(group, c, hw), "gx stddev part")
    worst(R.mbstd_bwd32(gy, x), R.mbstd_bwd(gy, x)[0], sc["gx"] + gy[:, :c].double().abs(), R.mbstd_gx_k(group, c, hw) + 1, "gx")
    worst(R.mbstd_jvp32(x, dx), R.mbstd_jvp(x, dx), sc["jv"], R.mbstd_jv_k(group, c, hw), "tangent")
    worst(R.mbstd_hvp32(gy, x, dx), R.mbstd_hvp(gy, x, dx), sc["mu"], R.mbstd_mu_k(group, c, hw), "mu")
    # the coefficient's cancellation is charged to its own sum only: ceff never exceeds |coef| + cabs
    assert bool((sc["gx"] <= (R.mbstd_scales(x, gy.abs(), dx)["gx"]) * (1 + 1e-12)).all())
    print(f"cabs / |coef| [b{b} {c}x{hw} {family}]: {float((sc['cabs'] / sc['coef'].abs().clamp_min(1e-300)).max()):.1f}")
    if group == 1:
        assert not bool(R.mbstd_bwd32(gs, x).any()) and not bool(R.mbstd_hvp32(gy, x, dx).any()) and not bool(R.mbstd_jvp32(x, dx).any())
        assert abs(float(R.mbstd_value32(x)[0]) - 1e-4) <= 1e-10


def test_block_sum_restatement_adds_every_term_once():
    t = torch.arange(1, 601, dtype=torch.float32).view(2, 300)
    assert torch.equal(R._block_sum32(t), t.sum(1))   # (integers: exact in any order)
    assert torch.equal(R._block_sum32(torch.ones(1, 1)), torch.ones(1))


def test_families_are_what_they_say():
    x = R.separated("host.sep", (8, 3, 5))
    m = x.view(4, 2, -1).mean((1, 2))
    assert all(abs(float(m[g]) - 3.0 * g) < 1.0 for g in range(4))    # sample b = g * M + m sits near 3 g
    h = R.heavy("host.heavy", (4096,))
    assert float(h.abs().max()) > 30 * float(h.abs().median())


# ---------------------------------------------------------------------------------------------- the weight-gradient finish
@pytest.mark.parametrize("k", [1, 3])
def test_finish_closed_form_is_float64_autograd_of_the_oracles_weight_branch(k):
    """oracle/stylegan2.py's modulated_conv2d (the per-sample weight scale * W * s, demodulated) + noise + bias, B = 3: the gradient
    of <gpre, z> to W by autograd, against scale * C - scale^2 * W * sum_b dz d^2 s^2 with C cut into 5 slabs, dz taken both from
    the three sums and directly."""
    b, cin, cout, h, w = 3, 5, 4, 6, 7
    gen = torch.Generator().manual_seed(77 + k)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    x, style, weight = rnd(b, cin, h, w), rnd(b, cin) + 1.0, rnd(1, cout, cin, k, k)
    noise, nw, bias, gp = rnd(b, 1, h, w), rnd(1), rnd(cout), rnd(b, cout, h, w)
    scale = 1.0 / math.sqrt(cin * k * k)
    wt = weight.clone().requires_grad_()
    out, _ = OG.modulated_conv2d(x, style.view(b, 1, cin, 1, 1), wt, None, None, demodulate=True, input_is_stylespace=True)
    z = out + nw * noise + bias.view(1, -1, 1, 1)
    (want,) = torch.autograd.grad((gp * z).sum(), wt)
    want = want[0].reshape(cout, cin, k * k)
    # the operands as the kernels see them
    d = torch.rsqrt((scale * weight * style.view(b, 1, cin, 1, 1)).pow(2).sum([2, 3, 4]) + 1e-8)           # [B,Cout]
    dg, sx = gp * d.view(b, cout, 1, 1), F.pad(x * style.view(b, cin, 1, 1), (k // 2,) * 4)
    c = torch.stack([torch.einsum("boyx,biyx->oi", dg, sx[:, :, ky:ky + h, kx:kx + w]) for ky in range(k) for kx in range(k)], 0)
    cut = rnd(5, *c.shape)
    slab = cut - cut.mean(0, keepdim=True) + c / 5                                                        # five slabs that sum to C
    sums = torch.stack([(gp * z.detach()).sum((2, 3)), (gp * noise).sum((2, 3)), gp.sum((2, 3))], 2)      # [B,Cout,3]
    wk = weight[0].reshape(cout, cin, k * k)
    for form, dz_in in (("sums_nw_bias", None), ("dz", (gp * (z.detach() - nw * noise - bias.view(1, -1, 1, 1))).sum((2, 3)))):
        dzv, dzs = R.finish_dz(form, sums, dz_in, nw, bias)
        a, m = R.finish(slab, wk, dzv, d, style, scale)
        sa, sm = R.finish(slab.abs(), wk.abs(), dzs, d, style, scale)
        _agree(a + m, want, sa + sm.abs(), f"finish closed form ({form}, {k}x{k})")
    assert float(m.abs().max()) > 1e-3 * float(a.abs().max())   # (the demodulation term is no rounding-sized correction here)


def test_wsq_reference_is_the_demodulation_sum():
    w = torch.randn(4, 5, 9, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    s = torch.randn(2, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    d = torch.rsqrt((0.3 * w.unsqueeze(0) * s.view(2, 1, 5, 1)).pow(2).sum([2, 3]) + 1e-8)
    assert torch.allclose(d, torch.rsqrt(R.wsq(w, 0.3) @ (s * s).t() + 1e-8).t(), rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------- the shape lists
def test_shape_lists_reach_the_paths_they_name():
    rows = {k: R.fromrgb_rows(b, hw) for k, ((b, c, hw), _) in R.FROMRGB_CASES.items()}
    px = {k: b * hw for k, ((b, c, hw), _) in R.FROMRGB_CASES.items()}
    assert {1, 1023, 1024, 1025} <= set(px.values())
    assert rows["px1024_c255"] == 1 and rows["px1025_c256"] == 2 and rows["rows258_c1"] == 258 > 256
    assert px["capped_c2"] > R.STREAM_CAP and px["capped_c2"] - R.STREAM_CAP == 37
    (b, c, hw), _ = R.FROMRGB_CASES["straddle_c257"]
    assert R.FR_PPB % hw and hw < R.FR_PPB < b * hw   # the first workgroup covers sample 0, sample 1 and a part of sample 2
    assert {c for (b, c, hw), _ in R.FROMRGB_CASES.values()} >= {1, 3, 255, 256, 257, 512} and R.FROMRGB_REFUSED[0][1] == R.FR_MAX_C + 1
    big = [k for k, ((b, c, hw), _) in R.FROMRGB_CASES.items() if b * c * hw > 2 ** 20]
    assert sorted(big) == ["capped_c2", "model_b3", "model_b4"]   # the capped grid, and the shape the 32^2 Discriminator really runs
    assert {R.mbstd_group(b) for b in R.MBSTD_BATCHES} == {1, 2, 3, 4} and all(b % R.mbstd_group(b) for b in R.MBSTD_REFUSED)
    ns = {c * hw for c, hw in R.MBSTD_SHAPES}
    assert 1 in ns and any(1 < n < 256 for n in ns) and any(n > 256 and n % 256 for n in ns) and 8192 in ns
    assert max(4 * hw for _, hw in R.MBSTD_SHAPES) > 256
    assert [R.sumsq_parts(n) for n in R.SUMSQ_LENGTHS[:7]] == [1, 1, 1, 1, 1, 2, 257]
    assert R.sumsq_parts(0) == 0 and R.sumsq_parts(R.SQ_CHUNK * 65535) == 0 and R.sumsq_parts(R.SQ_CHUNK * 65535 - 1) == 65535
    n_fin = sorted(t * o * i for t in R.FINISH_TAPS for o, i in R.FINISH_DIMS)
    assert n_fin[0] < 64 and any(n % 64 for n in n_fin) and n_fin[-1] > 64 * 64
    assert [o * i for o, i in R.WSQ_DIMS] == [1, 255, 257]
