"""The float64 yardstick of the IR-SE50 elementwise kernels (tests/irse_ref.py) against float64 autograd on the CPU, so that the
yardstick is trusted before it judges a kernel (tests/test_gpu_irse_kernels.py): the PReLU backward from the OUTPUT, the SE block's
gate-and-add with both of its gradients, the strided shortcut's adjoint, and the phase-planar packing with its (+1,+1) crop."""
import pytest
import torch
import torch.nn.functional as F

import irse_ref as R

SHAPES = [(2, 5, 6, 10), (3, 5, 7, 9)]  # hw % 4 == 0 and != 0, C no multiple of 4, never square


def _gen(*key):
    return torch.Generator().manual_seed(1000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("slope_zero", [False, True])
def test_kink_free_inputs_keep_every_pre_activation_away_from_zero(shape, slope_zero):
    """The generator the GPU tests draw from: from the fp32 values, in float64 and in fp32 arithmetic, |a*x + b| >= KINK_MARGIN
    and both see the same sign; both signs occur in every plane; the per-channel parameters differ between channels."""
    g = _gen(*shape, slope_zero)
    a, b, slope = R.channel_params(g, shape[1], slope_zero)
    assert len(set(a.tolist())) == len(set(b.tolist())) == shape[1] and (a < 0).any() and (a > 0).any()
    assert (slope == 0).all() if slope_zero else (len(set(slope.tolist())) == shape[1] and (slope > 0.05).all() and (slope < 0.55).all())
    x = R.kink_free_inputs(g, shape, a, b)
    assert x.dtype == torch.float32
    pre64 = a.double().view(1, -1, 1, 1) * x.double() + b.double().view(1, -1, 1, 1)
    pre32 = a.view(1, -1, 1, 1) * x + b.view(1, -1, 1, 1)
    assert float(pre64.abs().min()) >= R.KINK_MARGIN and float(pre32.abs().min()) >= 0.99 * R.KINK_MARGIN
    assert bool(((pre64 > 0) == (pre32 > 0)).all())
    pos = (pre64 > 0).flatten(2)
    assert bool(pos.any(2).all()) and bool((~pos).any(2).all())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("slope_zero", [False, True])
def test_affine_act_and_its_backward_equal_autograd_of_prelu(shape, slope_zero):
    g = _gen(*shape, slope_zero, 7)
    a, b, slope = R.channel_params(g, shape[1], slope_zero)
    x = R.kink_free_inputs(g, shape, a, b)
    gy = torch.randn(shape, generator=g)
    xd = x.double().requires_grad_(True)
    y = F.prelu(a.double().view(1, -1, 1, 1) * xd + b.double().view(1, -1, 1, 1), slope.double())
    (gx,) = torch.autograd.grad(y, xd, gy.double())
    y_ref = R.affine_act(x, a, b, slope)
    assert torch.equal(y_ref, y.detach())
    got = R.affine_act_bwd(gy, y_ref, a, slope)  # from the OUTPUT, as the header states it
    assert float((got - gx).abs().max()) <= 1e-15 * float(gx.abs().max())
    if slope_zero:  # ReLU: y > 0 is exactly pre > 0, and y == 0 takes the slope (= 0) branch
        assert bool(((y_ref == 0) == (got == 0)).all()) and bool((y_ref == 0).any())
    # NULL operands: 1 / 0 / identity
    assert torch.equal(R.affine_act(x), x.double())
    assert torch.equal(R.affine_act_bwd(gy), gy.double())
    assert torch.equal(R.affine_act_bwd(gy, y_ref), gy.double())           # a mask without a slope is the identity
    assert torch.equal(R.affine_act_bwd(gy, None, a, slope), a.double().view(1, -1, 1, 1) * gy.double())  # no y: no mask
    # the scale twins bound the values they scale
    assert bool((R.affine_act_scale(x, a, b, slope) >= y_ref.abs()).all())
    assert bool((R.affine_act_bwd_scale(gy, y_ref, a, slope) >= got.abs()).all())


def test_affine_act_bwd_takes_the_slope_branch_at_an_output_of_exactly_zero():
    gy, y = torch.ones(1, 2, 1, 3), torch.tensor([[[[0.0, -0.0, 1.0]], [[-1.0, 0.0, 2.0]]]])
    slope, a = torch.tensor([0.25, 0.5]), torch.tensor([2.0, -3.0])
    got = R.affine_act_bwd(gy, y, a, slope)
    assert got.flatten().tolist() == [0.5, 0.5, 2.0, -1.5, -1.5, -3.0]


@pytest.mark.parametrize("shape", SHAPES)
def test_se_apply_bwd_and_channel_sums_equal_autograd_of_the_gated_residual(shape):
    """out = t*gate + shortcut, plus a term through the pooled mean of t (what the gate's own backward hands over as gpool): the two
    gradients are se_apply_bwd(gout, gate, gpool) and channel_sums(gout, t)."""
    g = _gen(*shape, 11)
    b, c, h, w = shape
    t, sc, gout = (torch.randn(shape, generator=g) for _ in range(3))
    gate, r = torch.rand(b, c, generator=g), torch.randn(b, c, generator=g)
    td, gd = t.double().requires_grad_(True), gate.double().requires_grad_(True)
    out = td * gd[:, :, None, None] + sc.double()
    assert torch.equal(R.se_apply(t, gate, sc, 0), out.detach())
    loss = (out * gout.double()).sum() + (td.mean((2, 3)) * r.double()).sum()
    g_t, g_gate = torch.autograd.grad(loss, [td, gd])
    gpool = r.double() / (h * w)
    assert float((R.se_apply_bwd(gout, gate, gpool) - g_t).abs().max()) <= 1e-15 * float(g_t.abs().max())
    assert float((R.channel_sums(gout, t) - g_gate).abs().max()) <= 1e-14 * float(R.channel_sums_scale(gout, t).max())
    assert float((R.channel_sums(t) - t.double().sum((2, 3))).abs().max()) == 0.0
    assert bool((R.channel_sums_scale(gout, t) >= R.channel_sums(gout, t).abs()).all())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_strided_shortcut_and_its_adjoint_equal_maxpool_1_s(shape, stride):
    """MaxPool2d(1, s) = x[..., ::s, ::s] on a [B,C,s*H,s*W] input: se_apply reads it, shortcut_add_bwd is its autograd gradient
    added onto what is already there."""
    g = _gen(*shape, stride, 13)
    b, c, h, w = shape
    x = torch.randn(b, c, stride * h, stride * w, generator=g)
    t, gin = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    gate, gx0 = torch.rand(b, c, generator=g), torch.randn(b, c, stride * h, stride * w, generator=g)
    xd = x.double().requires_grad_(True)
    pooled = F.max_pool2d(xd, 1, stride)
    assert pooled.shape == shape and torch.equal(pooled.detach(), xd.detach()[..., ::stride, ::stride])
    assert torch.equal(R.se_apply(t, gate, x, stride), t.double() * gate.double()[:, :, None, None] + pooled.detach())
    (gref,) = torch.autograd.grad(pooled, xd, gin.double())
    assert torch.equal(R.shortcut_add_bwd(gx0, gin, stride), gx0.double() + gref)
    assert torch.equal(R.shortcut_add_bwd(torch.zeros_like(gx0), gin, stride), gref)


@pytest.mark.parametrize("h,w", [(3, 5), (6, 2), (1, 17), (1, 1)])
def test_planar_crop_of_to_planar_is_the_dense_image_without_its_first_row_and_column(h, w):
    """to_planar on a [B,C,2h+1,2w+1] image with h != w: the layout's shape and pitch, T[Y][X] = planar[Y&1][X&1][Y>>1][X>>1]
    element by element, the fill everywhere else, from_planar as its inverse and the crop the kernels read."""
    from where2edit_amd import functional as K
    g = _gen(h, w, 17)
    dense = torch.randn(2, 3, 2 * h + 1, 2 * w + 1, generator=g)
    fill = 1e30
    p = R.to_planar(dense, fill)
    wp = K.planar_pitch(w)
    assert p.shape == (2, 3, 2, 2, h + 1, wp) and wp % 16 == 0 and wp >= w + 1 and wp - (w + 1) < 16 and p.dtype == dense.dtype
    for yy in range(2 * h + 1):
        for xx in range(2 * w + 1):
            assert torch.equal(p[:, :, yy & 1, xx & 1, yy >> 1, xx >> 1], dense[:, :, yy, xx])
    assert int((p == fill).sum()) == p.numel() - dense.numel()
    assert torch.equal(R.from_planar(p, 2 * h + 1, 2 * w + 1), dense)
    crop = R.planar_crop(p, 2 * h, 2 * w)
    assert crop.shape == (2, 3, 2 * h, 2 * w) and torch.equal(crop, dense[..., 1:, 1:])
    assert not bool((crop == fill).any())
