"""Every elementwise / reduction entry point of csrc/irse.hip (include/w2e_irse.h) on its own against the float64 restatement of
tests/irse_ref.py -- non-square, C = 5, more than one pass of the grid, both `hw % 4` classes, unaligned views, every optional operand,
sentinels around what may be written and inside what may not be read -- and a census of the (entry point, path class) pairs that
IR-SE50, IDLoss and the e4e encoder really call, held against the COVERAGE table below.

How the error is judged.  The elementwise kernels do at most three rounded fp32 operations per element (a*x, + b, * slope; t*gate, + s;
a*gy, * mask), so every ELEMENT is held to |y - ref| <= 4 * 2^-24 * scale with `scale` the reference formula on absolute values
(irse_ref.*_scale), beside the global helpers.assert_close.  w2e_channel_sums: see test_channel_sums.  Where the result is a copy or
one correctly rounded sum it is compared bit for bit."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import irse_ref as R
from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------- the table the census is held to
# (entry point, path class) -> (the test that covers it, "run" = a class the census runs reach | "ABI only" = reachable through the C
# ABI alone).  The path class is what path_class() computes from a call's arguments: the kernel / form the dispatch picks and the
# optional operands that are not NULL.
_OPS3 = ["-", "a", "b", "slope", "a+b", "a+slope", "b+slope", "a+b+slope"]       # (a, b, slope) of w2e_affine_act_fwd
_OPS3B = ["-", "y", "a", "slope", "y+a", "y+slope", "a+slope", "y+a+slope"]      # (y, a, slope) of w2e_affine_act_bwd
_FWD_RUN = {("float4", "a+b"), ("scalar", "a+b")}                                  # BatchNorm in front of a conv; at 7^2 = 49 the scalar kernel
_BWD_RUN = {("dense", "y+slope"), ("planar", "y+slope"), ("dense", "y+a+slope"), ("dense", "a")}  # unit s=1 / s=2, input layer, output BN
_IRSE = "test_gpu_irse.py::"
COVERAGE = {}
COVERAGE.update({("w2e_affine_act_fwd", (k, o)): ("test_affine_act_fwd_operands_on_every_kernel", "run" if (k, o) in _FWD_RUN else "ABI only")
                 for k in ("float4", "scalar", "scalar-unaligned") for o in _OPS3})
COVERAGE.update({("w2e_affine_act_bwd", (f, o)): ("test_affine_act_bwd_dense" if f == "dense" else "test_affine_act_bwd_planar",
                                                  "run" if (f, o) in _BWD_RUN else "ABI only") for f in ("dense", "planar") for o in _OPS3B})
COVERAGE.update({
    ("w2e_channel_sums", ("float4", "-")): ("test_channel_sums", "run"),                 # the SE pool at 56^2 / 28^2 / 14^2
    ("w2e_channel_sums", ("float4", "y")): ("test_channel_sums", "run"),                 # its backward: d gate = sum gout*t
    ("w2e_channel_sums", ("scalar", "-")): ("test_channel_sums", "run"),                 # 7^2 = 49
    ("w2e_channel_sums", ("scalar", "y")): ("test_channel_sums", "run"),
    ("w2e_channel_sums", ("scalar-unaligned", "-")): ("test_channel_sums_unaligned_views", "ABI only"),
    ("w2e_channel_sums", ("scalar-unaligned", "y")): ("test_channel_sums_unaligned_views", "ABI only"),
    ("w2e_channel_sums", ("refused-unaligned", "-")): ("test_channel_sums_unaligned_views", "ABI only"),
    ("w2e_channel_sums", ("refused-unaligned", "y")): ("test_channel_sums_unaligned_views", "ABI only"),
    ("w2e_se_apply_fwd", ("sc_stride 0",)): ("test_se_apply_fwd", "run"),                # a convolution's output as the shortcut
    ("w2e_se_apply_fwd", ("sc_stride 1",)): ("test_se_apply_fwd", "run"),                # MaxPool2d(1, 1): the unit's own input
    ("w2e_se_apply_fwd", ("sc_stride 2",)): ("test_se_apply_fwd", "run"),                # MaxPool2d(1, 2): the first unit (64 -> 64, stride 2)
    ("w2e_se_apply_bwd", ()): ("test_se_apply_bwd_and_channel_sums_reproduce_autograd", "run"),
    ("w2e_shortcut_add_bwd", ("dense", "stride 1")): ("test_shortcut_add_bwd_dense", "run"),
    ("w2e_shortcut_add_bwd", ("dense", "stride 2")): ("test_shortcut_add_bwd_dense", "run"),
    ("w2e_shortcut_add_bwd", ("planar", "stride 1")): ("test_shortcut_add_bwd_planar", "run"),  # the stride-2 shortcut convolution's adjoint
    ("w2e_se_gate_fwd", ()): (_IRSE + "test_se_gate_kernels_equal_the_stock_composition", "run"),
    ("w2e_se_gate_bwd", ()): (_IRSE + "test_se_gate_kernels_equal_the_stock_composition", "run"),
    # called by psp_encoders through its own door, not irse_hip.call: listed so that the table names every entry point of the file
    ("w2e_upsample_add", ()): (_IRSE + "test_upsample_add_kernel_equals_bilinear_interpolate", "ABI only"),
})
# what the planar forms and the strided forms are run on everywhere below: never square, see the module docstring
PLANAR_SIZES = [(6, 10), (12, 4), (2, 34), (228, 230)]  # (2, 34): W/2 + 1 = 18 crosses the 16-float pitch; the last: > one grid pass

U = 2.0 ** -24
SENTINEL = 1e30
GUARD = 64  # floats (256 bytes: the views below keep the alignment the offset asks for)
B, C = 2, 5
# stream_grid (csrc/common.h) caps a launch at 2048 blocks of 256 threads = 524288 elements per pass of the grid-stride loop.  The
# smallest non-square totals above it at B*C = 10 planes: 227 x 231 (524370 elements, hw % 4 = 1, 2.1 MB) for the scalar kernels,
# 228 x 230 (524400, even sizes) for the planar forms and 456 x 460 (2097600 = 4 * 524400, 8.4 MB) for the float4 kernel, which
# strides over quads.  None is a multiple of 256.  w2e_channel_sums is no stream_grid kernel: it launches one block per 4 planes with
# no cap and each wave walks its own plane, so "more than one pass of the grid" has no meaning for it; its long planes (56^2, 57 x 55)
# are what make a lane loop more than once.  At the sizes past one pass only two operand sets are run where the small sizes run all
# eight -- the fullest set the backbone passes to that form and a sparse one -- to keep a case within a few seconds (the float64
# reference on the CPU is what costs); the operand handling does not depend on the size, the index arithmetic does.
GRID_PASS = 2048 * 256
SMALL = [(6, 10), (7, 9), (10, 6)]      # hw = 60 (% 4 == 0, fewer elements than a wave has lanes), 63, and H > W; totals 600 / 630: no multiple of 256
BIG_SCALAR, BIG_FLOAT4 = (227, 231), (456, 460)


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else None


def _gen(*key):
    return torch.Generator().manual_seed(2000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def _lib():
    from where2edit_amd import _lib as L
    return L


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def guarded(t, off=0, fill=SENTINEL):
    """A copy of t on the GPU that starts GUARD + off floats into a buffer of `fill`: (buffer, view)."""
    buf = torch.full((GUARD + off + t.numel() + GUARD,), fill, device=DEV, dtype=torch.float32)
    v = buf[GUARD + off:GUARD + off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return buf, v


def guards_intact(buf, off, numel, fill=SENTINEL):
    return bool((buf[:GUARD + off] == fill).all()) and bool((buf[GUARD + off + numel:] == fill).all())


def assert_elementwise(got, ref, scale, what, roundings=4):
    """Every element within `roundings` fp32 roundings of the float64 reference, relative to ITS OWN term scale; then the global norm."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) < 1e-10 * SENTINEL, f"{what}: a sentinel was read"
    ratio = (got - ref).abs() / (U * scale).clamp_min(1e-300)  # (scale == 0: the result must be exact)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: worst element {worst:.3f} x 2^-24 of its term scale (bound {roundings})")
    assert worst <= roundings, f"{what}: element {int(ratio.argmax())} is {worst:.3f} x 2^-24 of its term scale from float64 (bound {roundings})"
    assert_close(got, ref, 1e-6, what)


def pick(names, **operands):
    """The operands named in `names` ("a+slope", "-"), None for the rest."""
    on = set(names.split("+")) - {"-"}
    assert on <= set(operands), (names, list(operands))
    return {k: (v if k in on else None) for k, v in operands.items()}


# ---------------------------------------------------------------------------------------------- w2e_affine_act_fwd
def affine_act_into(x, a, b, slope, y):
    L = _lib()
    L.call("w2e_affine_act_fwd", L.ptr(x), L.ptr(a), L.ptr(b), L.ptr(slope), L.ptr(y), x.shape[0], x.shape[1], x.shape[2] * x.shape[3],
           L.stream_ptr())


@pytest.mark.parametrize("kernel,hw", [("float4", SMALL[0]), ("scalar", SMALL[1]), ("scalar-unaligned", SMALL[0])])
def test_affine_act_fwd_operands_on_every_kernel(kernel, hw):
    """All eight NULL / non-NULL combinations of (a, b, slope) on the float4 kernel (hw = 60, aligned), the scalar kernel (hw = 63) and
    the scalar fallback for hw % 4 == 0 behind pointers one float off a 16-byte boundary: the fallback's result equals the aligned one
    bit for bit, and the floats in front of and behind the output view keep their sentinel.  Negative a in every second channel."""
    from where2edit_amd import irse_hip as I
    g = _gen(*hw, 1)
    a, b, slope = R.channel_params(g, C)
    x = R.kink_free_inputs(g, (B, C) + hw, a, b)
    for ops in _OPS3:
        p = pick(ops, a=a, b=b, slope=slope)
        ref, scale = R.affine_act(x, **p), R.affine_act_scale(x, **p)
        d = {k: dev(v) for k, v in p.items()}
        y = I.affine_act(dev(x), d["a"], d["b"], d["slope"])
        if kernel == "scalar-unaligned":
            (_, xv), (ybuf, yv) = guarded(x, 1), guarded(torch.zeros_like(x), 1)
            affine_act_into(xv, d["a"], d["b"], d["slope"], yv)
            assert torch.equal(yv, y), f"({ops}) the unaligned fallback differs from the float4 kernel"
            assert guards_intact(ybuf, 1, x.numel()), f"({ops}) wrote outside the output view"
            y = yv
        assert_elementwise(y, ref, scale, f"affine_act_fwd {kernel} ({ops})")


@pytest.mark.parametrize("kernel,hw", [("float4", BIG_FLOAT4), ("scalar", BIG_SCALAR), ("scalar-unaligned", BIG_FLOAT4)])
def test_affine_act_fwd_past_one_pass_of_the_grid(kernel, hw):
    """Totals above what one pass of the grid covers (the float4 kernel counts quads), no multiple of 256; PReLU and ReLU slopes."""
    g = _gen(*hw, 2)
    shape = (B, C) + hw
    assert (shape[0] * shape[1] * hw[0] * hw[1] >> (0 if kernel == "scalar" else 2)) > GRID_PASS and (hw[0] * hw[1] % 4 == 0) == (kernel != "scalar")
    for slope_zero in (False, True):
        a, b, slope = R.channel_params(g, C, slope_zero)
        x = R.kink_free_inputs(g, shape, a, b)
        off = 1 if kernel == "scalar-unaligned" else 0
        (_, xv), (ybuf, yv) = guarded(x, off), guarded(torch.zeros_like(x), off)
        affine_act_into(xv, dev(a), dev(b), dev(slope), yv)
        assert guards_intact(ybuf, off, x.numel())
        assert_elementwise(yv, R.affine_act(x, a, b, slope), R.affine_act_scale(x, a, b, slope), f"affine_act_fwd {kernel} {hw} slope_zero={slope_zero}")
        if slope_zero:
            assert bool(((yv > 0).cpu() == (R.affine_act(x, a, b) > 0)).all()), "ReLU: y > 0 must be exactly pre > 0"


# ---------------------------------------------------------------------------------------------- w2e_affine_act_bwd
def _bwd_inputs(g, shape, slope_zero):
    """gy, a forward OUTPUT y with both signs and exact +0 / -0 planted in every plane, a, slope."""
    a, _, slope = R.channel_params(g, shape[1], slope_zero)
    gy, y = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    y[:, :, 0, 0], y[:, :, -1, -1], y[:, :, 1, 2] = 0.0, -0.0, 0.0
    return gy, y, a, slope


def affine_act_bwd_into(gy, y, a, slope, gx, planar=0):
    L = _lib()
    b, c, h, w = gx.shape
    L.call("w2e_affine_act_bwd", L.ptr(gy), L.ptr(y), L.ptr(a), L.ptr(slope), L.ptr(gx), b, c, h, w, planar, L.stream_ptr())


@pytest.mark.parametrize("hw", SMALL + [BIG_SCALAR], ids=_id)
@pytest.mark.parametrize("slope_zero", [False, True])
def test_affine_act_bwd_dense(hw, slope_zero):
    """gx = a * gy * (y > 0 ? 1 : slope) for every combination of (y, a, slope), PReLU slopes in (0.05, 0.55) and the ReLU's 0; an output
    of exactly 0 (either sign) takes the slope branch; a negative a flips no mask (the mask comes from y)."""
    from where2edit_amd import irse_hip as I
    shape = (B, C) + hw
    g = _gen(*hw, slope_zero, 3)
    gy, y, a, slope = _bwd_inputs(g, shape, slope_zero)
    for ops in (_OPS3B if hw != BIG_SCALAR else ["y+a+slope", "a"]):
        p = pick(ops, y=y, a=a, slope=slope)
        gx = I.affine_act_bwd(dev(gy), dev(p["y"]), dev(p["a"]), dev(p["slope"]), *shape)
        assert_elementwise(gx, R.affine_act_bwd(gy, **p), R.affine_act_bwd_scale(gy, **p), f"affine_act_bwd dense {hw} ({ops})")
        if p["y"] is not None and p["slope"] is not None:
            zero = (y == 0)
            want = (gy * (p["a"].view(1, -1, 1, 1) if p["a"] is not None else 1.0)) * slope.view(1, -1, 1, 1)  # fp32: the same two products
            assert int(zero.sum()) == 3 * B * C and torch.equal(gx.cpu()[zero], want[zero]), f"({ops}) y == 0 must take the slope branch"


@pytest.mark.parametrize("hw", PLANAR_SIZES, ids=_id)
def test_affine_act_bwd_planar(hw):
    """gy read through the (+1,+1) crop of a phase-planar T [B,C,2,2,H/2+1,WP] at H != W, the layout's padding full of 1e30: the result
    is bit for bit the dense form on the cropped image, for every combination of (y, a, slope), and meets the float64 bound."""
    from where2edit_amd import irse_hip as I
    h, w = hw
    shape = (B, C, h, w)
    g = _gen(*hw, 4)
    _, y, a, slope = _bwd_inputs(g, shape, False)
    dense = torch.randn(B, C, h + 1, w + 1, generator=g)
    t = R.to_planar(dense, SENTINEL)
    crop = dense[:, :, 1:, 1:].contiguous()
    assert torch.equal(R.planar_crop(t, h, w), crop) and int((t == SENTINEL).sum()) > 0
    for ops in (_OPS3B if h * w < 1000 else ["y+slope", "-"]):
        p = pick(ops, y=y, a=a, slope=slope)
        d = {k: dev(v) for k, v in p.items()}
        gx = I.affine_act_bwd(dev(t), d["y"], d["a"], d["slope"], *shape, planar=True)
        assert_elementwise(gx, R.affine_act_bwd(crop, **p), R.affine_act_bwd_scale(crop, **p), f"affine_act_bwd planar {hw} ({ops})")
        assert torch.equal(gx, I.affine_act_bwd(dev(crop), d["y"], d["a"], d["slope"], *shape)), f"({ops}) planar != dense on the crop"
        if ops == "-":
            assert torch.equal(gx.cpu(), crop), "no operand: the planar form is the crop itself"


@pytest.mark.parametrize("entry", ["w2e_affine_act_bwd", "w2e_shortcut_add_bwd"])
def test_planar_forms_refuse_odd_sizes_and_foreign_pitches(entry):
    """An odd height, an odd width, a row pitch that is not planar_pitch(W/2) and -- w2e_shortcut_add_bwd -- the planar form with
    stride 2: the library's RuntimeError, and gx keeps every bit (nothing was launched).  The buffers are large enough for any of
    these readings, so that a refusal that did not happen shows as a wrong number."""
    from where2edit_amd import functional as K
    L = _lib()
    g = _gen(5, len(entry))
    t = dev(torch.randn(B, C, 2, 2, 8, 64, generator=g))
    gx0 = torch.randn(B, C, 8, 10, generator=g)

    def run(h, w, pitch, stride=1, refusal=None):
        """True if gx changed.  With `refusal`: the call must raise the library's error with that message."""
        gx = dev(gx0)[:, :, :h, :w].contiguous()
        before = gx.clone()
        args = (L.ptr(t), None, None, None, L.ptr(gx), B, C, h, w, pitch) if entry == "w2e_affine_act_bwd" else \
               (L.ptr(gx), L.ptr(t), B, C, h, w, stride, pitch)
        if refusal is None:
            L.call(entry, *args, L.stream_ptr())
        else:
            with pytest.raises(RuntimeError, match=refusal):
                L.call(entry, *args, L.stream_ptr())
        return not torch.equal(gx, before)

    pitch = K.planar_pitch(5)
    assert pitch == 16
    assert not run(7, 10, pitch, refusal="even sizes"), "refused (odd height), but gx changed"
    assert not run(8, 9, pitch, refusal="even sizes"), "refused (odd width), but gx changed"
    assert not run(8, 10, 32, refusal="row pitch of 32 floats"), "refused (pitch 32), but gx changed"
    assert not run(8, 10, 8, refusal="row pitch of 8 floats"), "refused (pitch 8), but gx changed"
    if entry == "w2e_shortcut_add_bwd":
        assert not run(4, 4, K.planar_pitch(2), stride=2, refusal="stride 1"), "refused (planar with stride 2), but gx changed"
    assert run(8, 10, pitch), "the same buffers with the right arguments are accepted, and gx changes"


# ---------------------------------------------------------------------------------------------- w2e_channel_sums
CHANNEL_SUMS_SHAPES = [(2, 5, 6, 10), (2, 5, 7, 9), (2, 5, 7, 7), (1, 3, 56, 56), (3, 4, 14, 14), (1, 3, 57, 55)]


def assert_sums(got, x, y, what):
    """Every plane within (8 + log2(hw)) * 2^-24 * sum|x*y| of float64 (derivation: test_channel_sums), then the global norm."""
    hw = x.shape[2] * x.shape[3]
    ref, scale = R.channel_sums(x, y), R.channel_sums_scale(x, y)
    got = got.detach().double().cpu()
    assert got.shape == ref.shape
    bound = 8 + torch.log2(torch.tensor(float(hw))).item()
    ratio = (got - ref).abs() / (U * scale).clamp_min(1e-300)
    print(f"{what}: worst plane {float(ratio.max()):.3f} x 2^-24 of its sum|x*y| (bound {bound:.2f})")
    assert float(ratio.max()) <= bound, f"{what}: plane {int(ratio.argmax())} is {float(ratio.max()):.3f} x 2^-24 of its sum|x*y| from float64 (bound {bound:.2f})"
    assert_close(got, ref, 1e-5, what)


@pytest.mark.parametrize("shape", CHANNEL_SUMS_SHAPES, ids=_id)
@pytest.mark.parametrize("with_y", [False, True])
def test_channel_sums(shape, with_y):
    """sums[b,c] = sum_p x*(y or 1) with and without y: hw = 60 (below the 64 lanes, % 4 == 0), 63, 49 (IR-SE50's last stage), one
    long plane of 56^2 on the float4 path and one of 57 x 55 on the scalar one; plane counts of 10 and 3 (no multiple of the 4 planes a
    block holds) and 12.  Two calls agree bit for bit (the header promises a fixed reduction order).  (One block per 4 planes, no
    cap on the grid: there is no second pass of a grid to test here, see GRID_PASS.)

    The bound, (8 + log2(hw)) * 2^-24 * sum_p |x*y| per plane: a term reaches the result through the product (one rounding, none with
    an FMA), the pairwise sum of its float4 (2 additions; 0 on the scalar path), the lane's running sum over ceil(hw / 256) quads (or
    ceil(hw / 64) scalars) and the 6 levels of the 64-lane butterfly; each addition adds at most 2^-24 of the partial sum's terms.  For
    hw <= 64 that is 7 roundings, for hw = 63 / 49 one term per lane; for hw <= 2048 on the float4 path at most 1 + 2 + 8 + 6 = 17 <=
    8 + log2(hw) holds in the worst case too.  For the long planes the running sum is 13 (56^2) / 49 (57 x 55) additions deep, so the
    strict worst case, 22 / 56 roundings, lies above the bound of 19.6: there the bound relies on roundings not all pointing one way
    (their sum grows like the square root of the depth: a few 2^-24), which is the level a wrong reduction would have to hide in."""
    from where2edit_amd import irse_hip as I
    g = _gen(*shape, with_y, 6)
    x = torch.randn(shape, generator=g) + 0.25  # a mean: the plain sum does not cancel to nothing
    y = torch.randn(shape, generator=g) if with_y else None
    got = I.channel_sums(dev(x), dev(y))
    assert_sums(got, x, y, f"channel_sums {shape} y={with_y}")
    assert torch.equal(got, I.channel_sums(dev(x), dev(y))), "two calls differ: the reduction order is not fixed"


def test_channel_sums_unaligned_views():
    """Pointers one float off a 16-byte boundary: with hw % 4 != 0 the scalar path takes them (same bits as the aligned call); with
    hw % 4 == 0 the call is refused -- x alone, y alone -- and `sums` keeps its sentinel."""
    from where2edit_amd import irse_hip as I
    L = _lib()
    g = _gen(7)
    for hw, ok in ((SMALL[1], True), (SMALL[0], False)):
        x, y = torch.randn((B, C) + hw, generator=g), torch.randn((B, C) + hw, generator=g)
        (_, xv), (_, yv) = guarded(x, 1), guarded(y, 1)
        for xx, yy in ((xv, None), (xv, yv), (dev(x), yv), (xv, dev(y))):
            if ok:
                got = I.channel_sums(xx, yy)
                assert torch.equal(got, I.channel_sums(dev(x), None if yy is None else dev(y)))
                assert_sums(got, x, None if yy is None else y, f"channel_sums unaligned {hw}")
            else:
                sums = torch.full((B, C), SENTINEL, device=DEV)
                with pytest.raises(RuntimeError, match="16-byte aligned"):
                    L.call("w2e_channel_sums", L.ptr(xx), L.ptr(yy), L.ptr(sums), B, C, hw[0] * hw[1], L.stream_ptr())
                assert bool((sums == SENTINEL).all()), "refused, but sums changed"


# ---------------------------------------------------------------------------------------------- w2e_se_apply_fwd / _bwd
def _gates(g):
    gate = torch.rand(B, C, generator=g) * 0.9 + 0.05
    assert len(set(gate.flatten().tolist())) == B * C  # differ between channels AND between samples
    return gate


@pytest.mark.parametrize("hw", SMALL + [BIG_SCALAR], ids=_id)
@pytest.mark.parametrize("sc_stride", [0, 1, 2])
def test_se_apply_fwd(hw, sc_stride):
    """out = t*gate[b,c] + shortcut, the shortcut a [B,C,H,W] tensor (sc_stride 0) or the strided samples of a non-square
    [B,C,s*H,s*W] one (1, 2) whose unread positions hold 1e30; the output view's neighbours keep their sentinel."""
    L = _lib()
    h, w = hw
    g = _gen(*hw, sc_stride, 8)
    t, gate = torch.randn(B, C, h, w, generator=g), _gates(g)
    s = max(sc_stride, 1)
    sc = torch.full((B, C, s * h, s * w), SENTINEL)
    sc[:, :, ::s, ::s] = torch.randn(B, C, h, w, generator=g)
    assert int((sc == SENTINEL).sum()) == B * C * h * w * (s * s - 1)
    obuf, out = guarded(torch.zeros_like(t))
    td, gd, sd = dev(t), dev(gate), dev(sc)  # (named: a temporary's block is handed to the next allocation once ptr() returns)
    L.call("w2e_se_apply_fwd", L.ptr(td), L.ptr(gd), L.ptr(sd), sc_stride, L.ptr(out), B, C, h, w, L.stream_ptr())
    assert guards_intact(obuf, 0, t.numel())
    assert_elementwise(out, R.se_apply(t, gate, sc, sc_stride), R.se_apply_scale(t, gate, sc, sc_stride), f"se_apply_fwd {hw} sc_stride {sc_stride}")


@pytest.mark.parametrize("hw", SMALL + [BIG_SCALAR], ids=_id)
def test_se_apply_bwd_and_channel_sums_reproduce_autograd(hw):
    """g_t = gout*gate + gpool on its own, and together with w2e_channel_sums(gout, t) the two gradients of
    sum(gout * (t*gate + shortcut)) + sum(r * mean_p t) that float64 autograd gives (gpool = r / hw)."""
    from where2edit_amd import irse_hip as I
    L = _lib()
    h, w = hw
    g = _gen(*hw, 9)
    t, gout, sc = (torch.randn(B, C, h, w, generator=g) for _ in range(3))
    gate, r = _gates(g), torch.randn(B, C, generator=g)
    gpool = (r.double() / (h * w)).float()
    gbuf, g_t = guarded(torch.zeros_like(t))
    gout_d, gate_d, gpool_d = dev(gout), dev(gate), dev(gpool)
    L.call("w2e_se_apply_bwd", L.ptr(gout_d), L.ptr(gate_d), L.ptr(gpool_d), L.ptr(g_t), B, C, h * w, L.stream_ptr())
    assert guards_intact(gbuf, 0, t.numel())
    assert_elementwise(g_t, R.se_apply_bwd(gout, gate, gpool), R.se_apply_bwd_scale(gout, gate, gpool), f"se_apply_bwd {hw}")
    td, gd = t.double().requires_grad_(True), gate.double().requires_grad_(True)
    loss = ((td * gd[:, :, None, None] + sc.double()) * gout.double()).sum() + (td.mean((2, 3)) * gpool.double() * (h * w)).sum()
    ref_t, ref_gate = torch.autograd.grad(loss, [td, gd])
    assert_elementwise(g_t, ref_t, R.se_apply_bwd_scale(gout, gate, gpool), f"se_apply_bwd {hw} vs autograd")
    dgate = I.channel_sums(dev(gout), dev(t))
    assert_sums(dgate, gout, t, f"d gate {hw}")
    assert_close(dgate, ref_gate, 1e-5, "d gate vs autograd")


# ---------------------------------------------------------------------------------------------- w2e_shortcut_add_bwd
@pytest.mark.parametrize("hw", SMALL + [BIG_SCALAR], ids=_id)
@pytest.mark.parametrize("stride", [1, 2])
def test_shortcut_add_bwd_dense(hw, stride):
    """gx [B,C,s*H,s*W] (random, non-square) += g [B,C,H,W] at the strided positions: those hold the correctly rounded fp32 sum, every
    other position and the buffer around gx keep every bit."""
    L = _lib()
    h, w = hw
    g = _gen(*hw, stride, 10)
    gx0, gin = torch.randn(B, C, stride * h, stride * w, generator=g), torch.randn(B, C, h, w, generator=g)
    buf, gx = guarded(gx0)
    gin_d = dev(gin)
    L.call("w2e_shortcut_add_bwd", L.ptr(gx), L.ptr(gin_d), B, C, h, w, stride, 0, L.stream_ptr())
    assert guards_intact(buf, 0, gx0.numel())
    want = gx0.clone()
    want[:, :, ::stride, ::stride] += gin  # fp32: one rounding, the kernel's own
    assert torch.equal(gx.cpu(), want), f"{int((gx.cpu() != want).sum())} elements differ from the fp32 sum"
    scale = gx0.double().abs()
    scale[:, :, ::stride, ::stride] += gin.double().abs()
    assert_elementwise(gx, R.shortcut_add_bwd(gx0, gin, stride), scale, f"shortcut_add_bwd {hw} stride {stride}")


@pytest.mark.parametrize("hw", PLANAR_SIZES, ids=_id)
def test_shortcut_add_bwd_planar(hw):
    """gx += T[y+1][x+1] of a phase-planar T at H != W with 1e30 in its padding."""
    L = _lib()
    h, w = hw
    g = _gen(*hw, 11)
    gx0, dense = torch.randn(B, C, h, w, generator=g), torch.randn(B, C, h + 1, w + 1, generator=g)
    t = R.to_planar(dense, SENTINEL)
    buf, gx = guarded(gx0)
    t_d = dev(t)
    L.call("w2e_shortcut_add_bwd", L.ptr(gx), L.ptr(t_d), B, C, h, w, 1, t.shape[-1], L.stream_ptr())
    assert guards_intact(buf, 0, gx0.numel())
    crop = dense[:, :, 1:, 1:]
    assert torch.equal(gx.cpu(), gx0 + crop), f"{int((gx.cpu() != gx0 + crop).sum())} elements differ from the fp32 sum gx + T[1:,1:]"
    assert_elementwise(gx, R.shortcut_add_bwd(gx0, R.planar_crop(t, h, w), 1), gx0.double().abs() + crop.double().abs(), f"shortcut_add_bwd planar {hw}")


# ---------------------------------------------------------------------------------------------- the stride-2 convolution, non-square
@pytest.mark.parametrize("b,k,n,h,w", [(2, 24, 40, 9, 14), (1, 24, 40, 7, 20)])
def test_conv3x3_stride2_pad1_and_its_adjoint_non_square(b, k, n, h, w):
    """test_gpu_irse.py::test_conv3x3_stride2_pad1_and_its_adjoint on a [b,k,2h,2w] input with h != w: DOWN with down_pad =
    nn.Conv2d(k, n, 3, 2, 1); UP + the (+1,+1) crop of w2e_affine_act_bwd(planar) = its input gradient; the centre-tap pack = the 1x1
    stride-2 shortcut convolution, and its adjoint through w2e_shortcut_add_bwd(planar)."""
    from where2edit_amd import functional as K
    from where2edit_amd import irse_hip as I
    L = _lib()
    g = torch.Generator().manual_seed(k + n + 3 * h + w)
    wt = torch.randn(n, k, 3, 3, generator=g) * (k * 9) ** -0.5
    x = torch.randn(b, k, 2 * h, 2 * w, generator=g)
    a, bias = torch.rand(n, generator=g) + 0.5, torch.randn(n, generator=g)
    a_rep = a.to(DEV)[None].repeat(b, 1).contiguous()
    xd = x.double().requires_grad_(True)
    ref = F.conv2d(xd, wt.double(), stride=2, padding=1) * a.double()[None, :, None, None] + bias.double()[None, :, None, None]
    y = I.conv3x3(x.to(DEV), K.conv_pack(wt.to(DEV), 1.0, False, False), n, h, w, mode=K.MODE_DOWN, down_pad=1, out_scale=a_rep, bias=bias.to(DEV))
    assert_close(y, ref, 1e-4, "stride-2 pad-1 conv + BN")
    gy = torch.randn(b, n, h, w, generator=g)
    (gref,) = torch.autograd.grad(ref, xd, gy.double())
    tt = I.conv3x3(gy.to(DEV), K.conv_pack(wt.to(DEV), 1.0, True, False), k, h, w, mode=K.MODE_UP, in_scale=a_rep)
    assert tt.shape == (b, k, 2, 2, h + 1, K.planar_pitch(w))
    gx = I.affine_act_bwd(tt, None, None, None, b, k, 2 * h, 2 * w, planar=True)
    assert_close(gx, gref, 1e-4, "input gradient of the stride-2 conv")
    # centre-tap pack = the 1x1 stride-2 shortcut convolution (helpers.py:103-106)
    w1 = torch.randn(n, k, 1, 1, generator=g) * k ** -0.5
    w9 = torch.zeros(n, k, 3, 3)
    w9[:, :, 1, 1] = w1[:, :, 0, 0]
    x1 = x.double().requires_grad_(True)
    ref1 = F.conv2d(x1, w1.double(), stride=2)
    y = I.conv3x3(x.to(DEV), K.conv_pack(w9.to(DEV), 1.0, False, False), n, h, w, mode=K.MODE_DOWN, down_pad=1)
    assert_close(y, ref1, 1e-4, "1x1 stride-2 shortcut")
    (gref1,) = torch.autograd.grad(ref1, x1, gy.double())
    ts = I.conv3x3(gy.to(DEV), K.conv_pack(w9.to(DEV), 1.0, True, False), k, h, w, mode=K.MODE_UP)
    acc = gx.clone()
    L.call("w2e_shortcut_add_bwd", L.ptr(acc), L.ptr(ts), b, k, 2 * h, 2 * w, 1, ts.shape[-1], L.stream_ptr())
    assert_close(acc, gref + gref1, 1e-4, "main + shortcut input gradient")


# ---------------------------------------------------------------------------------------------- the census
def irse_entry_points():
    """The extern "C" entry points csrc/irse.hip defines, read from the source."""
    src = open(os.path.join(ROOT, "where2edit_amd", "csrc", "irse.hip")).read()
    return sorted(set(re.findall(r"^int (w2e_\w+)\(", src, re.M)))


def path_class(name, args):
    """The path class of one call of an irse.hip entry point, from the arguments irse_hip.call hands to the library."""
    def addr(p):
        v = getattr(p, "value", p)
        return 0 if v is None else int(v)

    def ops(**named):
        return "+".join(k for k, p in named.items() if addr(p)) or "-"

    def dim(v):
        return int(getattr(v, "value", v))

    if name == "w2e_affine_act_fwd":
        x, a, b, slope, y, _, _, hw = args[:8]
        aligned = ((addr(x) | addr(y)) & 15) == 0
        return ("float4" if dim(hw) % 4 == 0 and aligned else ("scalar" if dim(hw) % 4 else "scalar-unaligned"), ops(a=a, b=b, slope=slope))
    if name == "w2e_affine_act_bwd":
        _, y, a, slope = args[:4]
        return ("planar" if dim(args[9]) else "dense", ops(y=y, a=a, slope=slope))
    if name == "w2e_channel_sums":
        x, y, _, _, _, hw = args[:6]
        aligned = ((addr(x) | addr(y)) & 15) == 0
        kernel = "scalar" if dim(hw) % 4 else "float4"
        if not aligned:
            kernel = "scalar-unaligned" if dim(hw) % 4 else "refused-unaligned"
        return (kernel, ops(y=y))
    if name == "w2e_se_apply_fwd":
        return (f"sc_stride {dim(args[3])}",)
    if name == "w2e_shortcut_add_bwd":
        return ("planar" if dim(args[7]) else "dense", f"stride {dim(args[6])}")
    return ()


def test_path_class_reads_the_arguments_the_wrappers_pass():
    """path_class on argument lists built like irse_hip's own: what the census records is what the dispatch looks at."""
    L = _lib()
    x = torch.zeros(GUARD + 8, device=DEV)
    al, un, null, s = L.ptr(x), L.ptr(x[1:]), L.ptr(None), L.stream_ptr()
    assert path_class("w2e_affine_act_fwd", (al, al, al, null, al, 2, 5, 60, s)) == ("float4", "a+b")
    assert path_class("w2e_affine_act_fwd", (al, null, null, null, al, 2, 5, 49, s)) == ("scalar", "-")
    assert path_class("w2e_affine_act_fwd", (un, null, null, al, al, 2, 5, 60, s)) == ("scalar-unaligned", "slope")
    assert path_class("w2e_affine_act_bwd", (al, al, null, al, al, 2, 5, 6, 10, 16, s)) == ("planar", "y+slope")
    assert path_class("w2e_affine_act_bwd", (al, null, al, null, al, 2, 5, 6, 10, 0, s)) == ("dense", "a")
    assert path_class("w2e_channel_sums", (al, null, al, 2, 5, 49, s)) == ("scalar", "-")
    assert path_class("w2e_channel_sums", (al, un, al, 2, 5, 60, s)) == ("refused-unaligned", "y")
    assert path_class("w2e_se_apply_fwd", (al, al, al, 2, al, 2, 5, 6, 10, s)) == ("sc_stride 2",)
    assert path_class("w2e_shortcut_add_bwd", (al, al, 2, 5, 6, 10, 1, 16, s)) == ("planar", "stride 1")
    assert path_class("w2e_se_apply_bwd", (al, al, al, al, 2, 5, 60, s)) == ()


def test_coverage_table_names_every_entry_point_and_existing_tests():
    import test_gpu_irse
    assert sorted({name for name, _ in COVERAGE}) == irse_entry_points()
    for (name, cls), (test, reach) in COVERAGE.items():
        assert reach in ("run", "ABI only"), (name, cls, reach)
        where, fn = (test_gpu_irse, test[len(_IRSE):]) if test.startswith(_IRSE) else (None, test)
        assert callable(getattr(where, fn) if where else globals().get(fn)), f"{name} {cls}: no test named {test}"
    own = {name for (name, _), (test, _) in COVERAGE.items() if not test.startswith(_IRSE)}
    assert own == {"w2e_affine_act_fwd", "w2e_affine_act_bwd", "w2e_channel_sums", "w2e_se_apply_fwd", "w2e_se_apply_bwd", "w2e_shortcut_add_bwd"}


def test_census_of_the_paths_real_runs_take(monkeypatch):
    """One IR-SE50 Backbone forward + backward at batch 2, one IDLoss forward + backward on [y_hat; y] at 256^2 and one
    Encoder4Editing forward, with irse_hip.call recording (entry point, path class) of every call: each pair is a row of COVERAGE,
    the pairs seen are exactly the rows marked "run" that go through irse_hip.call (so neither label can be wrong, and a refactor
    that routes the calls past irse_hip.call fails here instead of passing on an empty record), and every irse.hip entry point that
    ran has a test.  The six entry points this file tests must each have been recorded; w2e_se_gate_fwd / _bwd are accepted on the
    strength of their kernel-level test in test_gpu_irse.py (the `_IRSE` rows), which this file does not repeat."""
    import types

    import make_golden_e4e as ME
    import seeded
    from where2edit_amd import irse_hip as I
    from where2edit_amd.id_loss import Backbone, IDLoss
    from where2edit_amd.psp_encoders import Encoder4Editing
    entries = set(irse_entry_points())
    seen = {}
    real_call = I.call

    def recording(name, *args):
        if name in entries:
            key = (name, path_class(name, args))
            seen[key] = seen.get(key, 0) + 1
        return real_call(name, *args)

    monkeypatch.setattr(I, "call", recording)
    net = Backbone(112, 50, drop_ratio=0.6, mode="ir_se").eval()
    net.load_state_dict(seeded.irse_fill(net.state_dict()), strict=True)
    net = net.to(DEV).requires_grad_(False)
    xg = seeded.tensor("irse.x", (2, 3, 112, 112), 0.5).to(DEV).requires_grad_(True)
    y = net(xg)
    assert hasattr(net, "_plan"), "the HIP path did not run"
    torch.autograd.grad((y * seeded.tensor("irse.r", (2, 512)).to(DEV)).sum(), xg)
    mod = IDLoss(types.SimpleNamespace(ir_se50_weights=None))
    mod.facenet.load_state_dict(seeded.irse_fill(mod.facenet.state_dict()), strict=True)
    mod = mod.to(DEV)
    img = seeded.tensor("id.y256", (2, 3, 256, 256), 0.5)
    yh = (img + 0.2 * seeded.tensor("id.d256", (2, 3, 256, 256))).to(DEV).requires_grad_(True)
    loss, _ = mod(yh, img.to(DEV))
    torch.autograd.grad(loss, yh)
    enc = Encoder4Editing(50, "ir_se", types.SimpleNamespace(stylegan_size=1024)).eval()
    enc.load_state_dict(ME.encoder_state_dict(enc.state_dict()), strict=True)
    enc = enc.to(DEV).requires_grad_(False)
    with torch.no_grad():
        enc(seeded.tensor("e4e.x", (1, 3, 256, 256), 0.5).to(DEV))
    torch.cuda.synchronize()
    for key in sorted(seen):
        print(f"census: {seen[key]:4d} x {key[0]} {key[1]}")
    unknown = sorted(k for k in seen if k not in COVERAGE)
    assert not unknown, f"paths real runs take that COVERAGE has no test for: {unknown}"
    assert {name for name, _ in seen} <= {name for name, _ in COVERAGE}
    abi_only = sorted(k for k in seen if COVERAGE[k][1] == "ABI only")
    assert not abi_only, f"COVERAGE lists as ABI only what real runs do reach: {abi_only}"
    own = {"w2e_affine_act_fwd", "w2e_affine_act_bwd", "w2e_channel_sums", "w2e_se_apply_fwd", "w2e_se_apply_bwd", "w2e_shortcut_add_bwd"}
    assert own <= {name for name, _ in seen}, f"never recorded: {sorted(own - {name for name, _ in seen})} (do the calls still go through irse_hip.call?)"
    unreached = sorted(k for k, v in COVERAGE.items() if v[1] == "run" and k not in seen)
    assert not unreached, f"COVERAGE lists as run what these three runs never reach: {unreached}"
