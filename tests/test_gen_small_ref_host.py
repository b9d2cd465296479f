"""tests/gen_small_ref.py held to something independent of the kernels it is the reference of (CPU, float64): the ToRGB forward to
oracle/stylegan2.py's to_rgb at h != w with a non-symmetric 4x4 kernel, every backward formula to float64 autograd through the
matching forward, the mask resize to F.interpolate, and every `*_scale` twin to >= |ref|."""
import math

import pytest
import torch
import torch.nn.functional as F

import gen_small_ref as R
from oracle import ops as O
from oracle import stylegan2 as OG

TOL = 1e-12  # float64 against float64: a few hundred terms of O(1)
SLOPE, GAIN = 0.2, math.sqrt(2.0)


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def close(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    a, b = a.detach(), b.detach()
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err <= TOL, f"{what}: {err:.3e}"


def covers(scale, ref, what):
    assert scale.shape == ref.shape and bool((scale >= ref.abs() * (1 - 1e-12)).all()), f"{what}: the scale twin is below |ref|"


def upk(g):
    """A 4x4 kernel that is neither separable nor symmetric."""
    k = O.make_kernel([1, 3, 3, 1]).double() * 4 + 0.05 * rnd(g, 4, 4)
    assert not torch.allclose(k, k.t()) and not torch.allclose(k, torch.flip(k, (0, 1))) and torch.linalg.matrix_rank(k) > 1
    return k


@pytest.mark.parametrize("h,w", [(6, 10), (10, 6), (4, 14)])
@pytest.mark.parametrize("with_skip", [False, True])
def test_torgb_forward_equals_the_oracle(h, w, with_skip):
    g = torch.Generator().manual_seed(3 * h + w)
    b, cin = 2, 5
    weight, s, bias = rnd(g, 1, 3, cin, 1, 1), rnd(g, b, 1, cin, 1, 1), rnd(g, 1, 3, 1, 1)
    x, k = rnd(g, b, cin, h, w), upk(g)
    skip = rnd(g, b, 3, h // 2, w // 2) if with_skip else None
    sd = {"p.conv.weight": weight, "p.conv.modulation.weight": None, "p.conv.modulation.bias": None, "p.bias": bias, "p.upsample.kernel": k}
    want, _ = OG.to_rgb(sd, "p", x, s, skip, input_is_stylespace=True)
    wsc = weight[0, :, :, 0, 0] / math.sqrt(cin)
    wmod = wsc[None] * s[:, 0, :, 0, 0][:, None, :]
    close(R.torgb_fwd(x, wmod, bias, skip, k), want, "per-sample weight")
    close(R.torgb_fwd(x, wsc, bias, skip, k, style=s.reshape(b, cin)), want, "styled")
    if with_skip:
        close(R.up2(skip, k), O.upfirdn2d(skip, k, up=2, pad=(2, 1)), "up2")
        assert float((R.up2(skip, k) - R.up2(skip, k.t())).abs().max()) > 1e-3 and float((R.up2(skip, k) - R.up2(skip, torch.flip(k, (0, 1)))).abs().max()) > 1e-3
    covers(R.torgb_fwd_scale(x, wmod, bias, skip, k), want, "torgb_fwd_scale")
    covers(R.torgb_fwd_scale(x, wsc, bias, skip, k, style=s.reshape(b, cin)), want, "torgb_fwd_scale styled")


@pytest.mark.parametrize("styled", [False, True])
@pytest.mark.parametrize("with_acc", [False, True])
def test_torgb_backward_equals_autograd(styled, with_acc):
    g = torch.Generator().manual_seed(11 + styled + 2 * with_acc)
    b, cin, h, w = 2, 5, 6, 10
    x = rnd(g, b, cin, h, w).requires_grad_(True)
    wmod = (rnd(g, 3, cin) if styled else rnd(g, b, 3, cin)).requires_grad_(True)
    style = rnd(g, b, cin).requires_grad_(True) if styled else None
    gy, acc = rnd(g, b, 3, h, w), (rnd(g, b, cin, h, w) if with_acc else None)
    y = R.torgb_fwd(x, wmod, rnd(g, 3), rnd(g, b, 3, h // 2, w // 2), upk(g), style)
    loss = (y * gy).sum() + ((x * acc).sum() if with_acc else 0.0)
    gx_ref, gw_ref = torch.autograd.grad(loss, [x, style if styled else wmod])
    gx, gw = R.torgb_bwd(x.detach(), wmod.detach(), gy, acc, None if style is None else style.detach())
    close(gx, gx_ref, "gx"), close(gw, gw_ref, "gstyle" if styled else "gwmod")
    sx, sw = R.torgb_bwd_scale(x.detach(), wmod.detach(), gy, acc, None if style is None else style.detach())
    covers(sx, gx, "gx scale"), covers(sw, gw, "gw scale")


def _activation(pre0, noise, t, u, v, slope, gain):
    """lrelu(t*pre0 + u*noise + v) * gain with per-(b, channel) t = 1, u = 0, v = 0: their gradients are the three sums."""
    pre = t[..., None] * pre0 + u[..., None] * noise.reshape(1, 1, -1) + v[..., None]
    return F.leaky_relu(pre, slope) * gain


@pytest.mark.parametrize("styled", [False, True])
@pytest.mark.parametrize("slope,gain", [(SLOPE, GAIN), (0.35, 1.0)])
def test_torgb_fused_activation_backward_equals_autograd(styled, slope, gain):
    g = torch.Generator().manual_seed(17 + styled)
    b, cin, h, w = 2, 5, 6, 10
    pre0 = rnd(g, b, cin, h * w).requires_grad_(True)
    noise = rnd(g, h * w)
    t = torch.ones(b, cin, dtype=torch.float64, requires_grad=True)
    u, v = (torch.zeros(b, cin, dtype=torch.float64, requires_grad=True) for _ in range(2))
    x = _activation(pre0, noise, t, u, v, slope, gain).reshape(b, cin, h, w)
    wmod = rnd(g, 3, cin) if styled else rnd(g, b, 3, cin)
    style = rnd(g, b, cin) if styled else None
    gy, acc = rnd(g, b, 3, h, w), rnd(g, b, cin, h, w)
    loss = (R.torgb_fwd(x, wmod, None, None, None, style) * gy).sum() + (x * acc).sum()
    gpre_ref, g_t, g_u, g_v = torch.autograd.grad(loss, [pre0, t, u, v])
    gpre, gw, sums = R.torgb_bwd_actbwd(x.detach(), wmod, style, gy, acc, noise, slope, gain)
    close(gpre, gpre_ref.reshape(b, cin, h, w), "gpre")
    close(sums, torch.stack([g_t, g_u, g_v], -1), "sums3")
    close(gw, R.torgb_bwd(x.detach(), wmod, gy, acc, style)[1], "gw")
    for s, r, what in zip(R.torgb_bwd_actbwd_scale(x.detach(), wmod, style, gy, acc, noise, slope, gain), (gpre, gw, sums), ("gpre", "gw", "sums3")):
        covers(s, r, what + " scale")
    assert float(R.torgb_bwd_actbwd(x.detach(), wmod, style, gy, acc, None, slope, gain)[2][..., 1].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 8, 1), (1, 4, 12)])
@pytest.mark.parametrize("operands", ["-", "bias", "noise", "bias+noise"])
def test_bias_act_equals_the_oracle_and_autograd(shape, operands):
    g = torch.Generator().manual_seed(sum(shape) + len(operands))
    x = rnd(g, *shape).requires_grad_(True)
    bias = rnd(g, shape[1]) if "bias" in operands else None
    noise, nw = (rnd(g, shape[2]), rnd(g, 1)) if "noise" in operands else (None, None)
    for slope, gain in ((SLOPE, GAIN), (0.35, 1.0)):
        y = R.bias_act_fwd(x, bias, noise, nw, slope, gain)
        xin = x if noise is None else x + nw * noise
        want = O.fused_leaky_relu(xin.reshape(shape[0], shape[1], shape[2], 1), bias if bias is not None else torch.zeros(shape[1], dtype=torch.float64),
                                  slope, gain).reshape(shape)
        close(y, want, "bias_act_fwd")
        covers(R.bias_act_fwd_scale(x.detach(), bias, noise, nw, slope, gain), y.detach(), "bias_act_fwd_scale")
        gy = rnd(g, *shape)
        (gx_ref,) = torch.autograd.grad((y * gy).sum(), x)
        close(R.bias_act_bwd(gy, y.detach(), slope, gain), gx_ref, "bias_act_bwd")
        covers(R.bias_act_bwd_scale(gy, y.detach(), slope, gain), gx_ref, "bias_act_bwd_scale")


def test_bias_act_backward_takes_the_slope_at_zero_and_the_sums_equal_autograd():
    g = torch.Generator().manual_seed(23)
    b, c, n = 2, 3, 9
    y = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=torch.float64)
    assert R.bias_act_bwd(torch.ones(4), y, SLOPE, GAIN).tolist() == [GAIN * SLOPE, GAIN * SLOPE, GAIN, GAIN * SLOPE]
    pre0, noise = rnd(g, b, c, n).requires_grad_(True), rnd(g, n)
    t = torch.ones(b, c, dtype=torch.float64, requires_grad=True)
    u, v = (torch.zeros(b, c, dtype=torch.float64, requires_grad=True) for _ in range(2))
    out = _activation(pre0, noise, t, u, v, SLOPE, GAIN)
    gy = rnd(g, b, c, n)
    gpre_ref, g_t, g_u, g_v = torch.autograd.grad((out * gy).sum(), [pre0, t, u, v])
    gx, sums = R.bias_act_bwd_reduce(gy, out.detach(), noise, SLOPE, GAIN)
    close(gx, gpre_ref, "gx"), close(sums, torch.stack([g_t, g_u, g_v], -1), "sums")
    sx, ss = R.bias_act_bwd_reduce_scale(gy, out.detach(), noise, SLOPE, GAIN)
    covers(sx, gx, "gx scale"), covers(ss, sums, "sums scale")


@pytest.mark.parametrize("cin,cout", [(5, 5), (65, 33)])
@pytest.mark.parametrize("form", ["dz", "sums", "sums+noise_w+bias"])
def test_demod_equals_the_oracle_and_autograd(cin, cout, form):
    g = torch.Generator().manual_seed(cin + cout + len(form))
    b, hw, eps = 3, 7, 1e-8
    weight = rnd(g, 1, cout, cin, 3, 3)
    s = rnd(g, b, cin).requires_grad_(True)
    wsq = (weight[0] / math.sqrt(cin * 9)).pow(2).sum((2, 3))
    d = R.demod_fwd(s, wsq, eps)
    wmod = weight / math.sqrt(cin * 9) * s.reshape(b, 1, cin, 1, 1)
    close(d, torch.rsqrt(wmod.pow(2).sum([2, 3, 4]) + eps), "d (model.py:241-243 as oracle/stylegan2.py writes it)")
    covers(R.demod_fwd_scale(s.detach(), wsq, eps), d.detach(), "demod_fwd_scale")
    dvar = d.detach().clone().requires_grad_(True)
    z, gpre, noise = rnd(g, b, cout, hw), rnd(g, b, cout, hw), rnd(g, hw)
    nw = rnd(g, 1) if "noise_w" in form else None
    bias = rnd(g, cout) if "bias" in form else None
    gs0 = rnd(g, b, cin)
    # the layer: pre = d*z (+ nw*noise + bias); dL/dpre = gpre; the direct part of gs (through the modulated input) is gs0
    (gd_ref,) = torch.autograd.grad((gpre * (dvar[..., None] * z)).sum(), dvar)
    (gs_ref,) = torch.autograd.grad((gpre * (d[..., None] * z)).sum(), s)
    pre = d.detach()[..., None] * z + (nw * noise if nw is not None else 0.0) + (bias[None, :, None] if bias is not None else 0.0)
    sums = torch.stack([(gpre * pre).sum(-1), (gpre * noise).sum(-1), gpre.sum(-1)], -1)
    dz = (gpre * (d.detach()[..., None] * z)).sum(-1)
    args = (None, dz, None, None) if form == "dz" else (sums, None, nw, bias)
    gs, gd = R.demod_bwd(*args, d.detach(), s.detach(), wsq, gs0)
    close(gs, gs0 + gs_ref, "gs"), close(gd, gd_ref, "gd")
    ss, sd = R.demod_bwd_scale(*args, d.detach(), s.detach(), wsq, gs0)
    covers(ss, gs, "gs scale"), covers(sd, gd, "gd scale")


@pytest.mark.parametrize("with_bias", [False, True])
def test_style_affine_equals_the_oracle_and_autograd(with_bias):
    g = torch.Generator().manual_seed(31)
    b, n_latent, dim = 3, 4, 12
    layers = [(0, 32), (2, 64), (2, 32), (3, 96)]  # W+ index 1 unused, 2 shared
    rows = sum(cw for _, cw in layers)
    latent = rnd(g, b, n_latent, dim).requires_grad_(True)
    raw_w, raw_b, lr_mul = rnd(g, rows, dim), rnd(g, rows), 0.5
    w, bias = raw_w * (lr_mul / math.sqrt(dim)), (raw_b * lr_mul if with_bias else None)
    outs = R.style_affine_fwd(latent, w, bias, layers)
    off = 0
    for (widx, cw), y in zip(layers, outs):
        want = O.equal_linear(latent[:, widx], raw_w[off:off + cw], raw_b[off:off + cw] if with_bias else None, lr_mul)
        close(y, want, f"layer at W+ {widx}")
        off += cw
    for s, y in zip(R.style_affine_fwd_scale(latent.detach(), w, bias, layers), outs):
        covers(s, y.detach(), "style_affine_fwd_scale")
    gouts = [rnd(g, b, cw) for _, cw in layers]
    (gl_ref,) = torch.autograd.grad(sum((y * go).sum() for y, go in zip(outs, gouts)), latent)
    gl = R.style_affine_bwd(gouts, w, layers, n_latent)
    close(gl, gl_ref, "glatent")
    assert float(gl[:, 1].abs().max()) == 0.0
    covers(R.style_affine_bwd_scale(gouts, w, layers, n_latent), gl, "style_affine_bwd_scale")


@pytest.mark.parametrize("h,w,ms", [(6, 10, 5), (10, 6, 3), (12, 20, 4), (5, 7, 9), (8, 130, 8), (4, 260, 4), (12, 12, 5), (7, 7, 7)])
def test_mask_blend_equals_interpolate_and_autograd(h, w, ms):
    g = torch.Generator().manual_seed(h + 3 * w + ms)
    bsz, c = 2, 3
    a = rnd(g, bsz, c, h, w).requires_grad_(True)
    b = rnd(g, bsz, c, h, w).requires_grad_(True)
    mask = torch.rand(bsz, 1, ms, ms, generator=g, dtype=torch.float64).requires_grad_(True)
    # torch's own nearest resize (fp32: the index arithmetic the kernel documents), non-square
    m32 = F.interpolate(mask.detach().float(), size=(h, w))
    assert torch.equal(R.resized_mask(mask.detach().float(), h, w), m32.double()), "the index rule differs from F.interpolate's"
    out = R.mask_blend_fwd(a, b, mask)
    if h == w:
        close(out, O.mask_blend(a, b, mask), "mask_blend_fwd vs oracle/ops.py")
    m64 = F.interpolate(mask.detach(), size=(h, w))
    assert torch.equal(R.resized_mask(mask.detach(), h, w), m64)
    close(out.detach(), m64 * a.detach() + (1 - m64) * b.detach(), "mask_blend_fwd")
    covers(R.mask_blend_fwd_scale(a.detach(), b.detach(), mask.detach()), out.detach(), "fwd scale")
    gout = rnd(g, bsz, c, h, w)
    refs = torch.autograd.grad((out * gout).sum(), [a, b, mask])
    got = R.mask_blend_bwd(gout, a.detach(), b.detach(), mask.detach())
    for x, r, what in zip(got, refs, ("ga", "gb", "gmask")):
        close(x, r, what)
    for s, r, what in zip(R.mask_blend_bwd_scale(gout, a.detach(), b.detach(), mask.detach()), refs, ("ga", "gb", "gmask")):
        covers(s, r, what + " scale")
    empty = (R.pixels_per_cell(h, ms)[:, None] * R.pixels_per_cell(w, ms)[None, :]) == 0
    assert bool((got[2][:, 0][:, empty] == 0).all()) and (ms <= min(h, w)) == (not bool(empty.any()))
