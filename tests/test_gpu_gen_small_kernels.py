"""The generator's small kernels one by one against the float64 restatement of tests/gen_small_ref.py (held to oracle/ and to autograd
by tests/test_gen_small_ref_host.py): the seven ToRGB entry points of csrc/torgb.hip and w2e_bias_act_*, w2e_demod_*, w2e_style_affine_*,
w2e_mask_blend_* of csrc/elementwise.hip, called through the C ABI.  Never square; sizes that reach every dispatch class of the host
code (TORGB_TABLE); channel counts that are ragged against the kernels' block shapes; every optional operand NULL and given; a
non-separable, non-symmetric 4x4 up-sampling kernel; every backward in default mode and with "deterministic" = 1, against the same
reference.  Outputs are pre-filled with NaN, inputs and outputs sit between sentinels that must survive.  A census of what a 64^2
generator pass, a mapper step and a region-attention blend really call is held against the COVERAGE table.

How the error is judged.  Every ELEMENT against its own term scale (gen_small_ref.*_scale: the formula on absolute values), beside the
global helpers.assert_close: |got - ref| <= N * 2^-24 * scale, N = the number of dependent fp32 roundings on the longest chain the
kernel uses for that output, counted from the kernel source beside each test.  (A rounding of a LOCAL term -- a product, a float4's own
sum -- is relative to that term alone; over all terms these add up to one 2^-24 * scale per such step, not one per term.)  No element is
excluded anywhere.  `-s` prints the worst ratio of every comparison; the last test prints the table DESIGN.md quotes."""
import math
import os
import re

import pytest
import torch

import gen_small_ref as R
from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
SENTINEL = 1e30
GUARD = 64  # floats
SLOPE, GAIN = 0.2, math.sqrt(2.0)
ACTS = [(SLOPE, GAIN), (0.35, 1.0)]
RSQRT_ULP = 2  # assumed: no statement of device rsqrtf's error was found in the ROCm headers / documents
WORST = {}     # what -> worst measured ratio (in 2^-24 of the term scale) and the bound it was held to
EXERCISED = set()  # (entry point, path class) of every call this file's tests made


# ---------------------------------------------------------------------------------------------- the host dispatch, restated
def torgb_fwd_class(h, w):
    """(CG, V) of torgb_fwd_impl: V = 4 if hw % 4 == 0; channel groups 16 / 4 / 1 by the number of pixel groups."""
    hw = h * w
    v = 4 if hw % 4 == 0 else 1
    groups = -(-hw // v)
    return (1 if groups >= 16384 else (4 if groups >= 1024 else 16)), v


def torgb_bwd_class(h, w, batch, cin, det):
    """(V, splits, per_split) of torgb_bwd_impl."""
    hw, waves, splits = h * w, batch * cin, 1
    if waves < 8192 and not det:
        splits = min(-(-8192 // waves), -(-hw // 4096))
    per = (-(-hw // splits) + 255) & ~255
    return (4 if hw % 4 == 0 else 1), -(-hw // per), per


def reduce_splits(rows, inner, det):
    """The splits of a row in w2e_bias_act_bwd_reduce."""
    return 1 if (rows >= 2048 or det) else max(1, min(-(-2048 // rows), -(-inner // 1024)))


# h x w -> (forward (CG, V), backward at batch 2, cin 5: (V, splits, per_split, pixels of the last split))
TORGB_TABLE = {
    (6, 10): ((16, 4), (4, 1, 256, 60)),        # a float4 spans two rows (W % 4 = 2); fewer quads than lanes
    (10, 6): ((16, 4), (4, 1, 256, 60)),
    (7, 9): ((16, 1), (1, 1, 256, 63)),         # hw odd: no skip possible
    (66, 70): ((4, 4), (4, 2, 2560, 2060)),     # 1155 quad groups; the last split is short
    (127, 131): ((1, 1), (1, 5, 3328, 3325)),
    (256, 260): ((1, 4), (4, 17, 4096, 1024)),
}
TORGB_SMALL, TORGB_BIG = [(6, 10), (10, 6), (7, 9)], [(66, 70), (127, 131), (256, 260)]
TORGB_CASES = [(h, w, cin) for (h, w) in TORGB_SMALL for cin in (3, 5, 20, 300)] + [(h, w, 5) for (h, w) in TORGB_BIG]
BATCH = 2


def _det():
    from where2edit_amd import _lib as L
    return bool(L.get_option("deterministic"))


def path_class(name, args):
    """The path class of one call, from the arguments handed to the library: what the host dispatch looks at."""
    def addr(p):
        v = getattr(p, "value", p)
        return 0 if v is None else int(v)

    def ops(**named):
        return "+".join(k for k, p in named.items() if addr(p)) or "-"

    def dim(v):
        return int(getattr(v, "value", v))

    if name in ("w2e_torgb_fwd", "w2e_torgb_styled_fwd"):
        o = 1 if name == "w2e_torgb_styled_fwd" else 0
        cg, v = torgb_fwd_class(dim(args[8 + o]), dim(args[9 + o]))
        return (f"CG{cg}", f"V{v}", ops(bias=args[2 + o], skip=args[3 + o]))
    if name in ("w2e_torgb_bwd", "w2e_torgb_bwd_acc", "w2e_torgb_styled_bwd", "w2e_torgb_bwd_actbwd"):
        first_dim = {"w2e_torgb_bwd": 5, "w2e_torgb_bwd_acc": 6, "w2e_torgb_styled_bwd": 7, "w2e_torgb_bwd_actbwd": 9}[name]
        b, cin, h, w = (dim(a) for a in args[first_dim:first_dim + 4])
        v, splits, _ = torgb_bwd_class(h, w, b, cin, _det())
        named = {"w2e_torgb_bwd": {}, "w2e_torgb_bwd_acc": dict(acc=args[3]), "w2e_torgb_styled_bwd": dict(acc=args[4]),
                 "w2e_torgb_bwd_actbwd": dict(style=args[2], acc=args[4], noise=args[5])}[name]
        return (f"V{v}", "split" if splits > 1 else "one", ops(**named))
    if name == "w2e_bias_act_fwd":
        _, bias, noise, _, _, _, c, inner = args[:8]
        c, inner = dim(c), dim(inner)
        branch = "float4" if inner % 4 == 0 else ("float4-bias" if inner == 1 and c % 4 == 0 and not addr(noise) else "scalar")
        return (branch, ops(bias=bias, noise=noise))
    if name == "w2e_bias_act_bwd":
        return ("float4" if dim(args[3]) % 4 == 0 else "scalar",)
    if name == "w2e_bias_act_bwd_reduce":
        rows, inner = dim(args[5]) * dim(args[6]), dim(args[7])
        splits = reduce_splits(rows, inner, _det())
        return ("float4" if inner % 4 == 0 else "scalar", "split" if splits > 1 else "one", ops(noise=args[2]))
    if name == "w2e_demod_bwd":
        sums, _, nw, bias = args[:4]
        cout = dim(args[11])
        walk = ("serial" if cout > 32 else "one-slice") if _det() else "slices"
        return ("sums" if addr(sums) else "dz", walk, ops(noise_w=nw, bias=bias, gd=args[8]))
    if name == "w2e_style_affine_fwd":
        return (ops(bias=args[2]),)
    if name == "w2e_style_affine_bwd":
        return (("serial" if dim(args[7]) > 32 else "one-block") if _det() else "blocks",)
    if name == "w2e_mask_blend_bwd":
        w = dim(args[10])
        return (f"{256 if w >= 256 else (128 if w >= 128 else 64)} threads", ops(gb=args[5], gmask=args[6]))
    return ()


# ---------------------------------------------------------------------------------------------- the table the census is held to
# (entry point, path class) -> (the test that covers it, "run" = a class the census runs reach | "ABI only").
_FWD_OPS = ["-", "bias", "skip", "bias+skip"]
_ACT_OPS = ["-", "style", "acc", "noise", "style+acc", "style+noise", "acc+noise", "style+acc+noise"]
_BA_OPS = ["-", "bias", "noise", "bias+noise"]
_DM_OPS = ["-", "noise_w", "bias", "gd", "noise_w+bias", "noise_w+gd", "bias+gd", "noise_w+bias+gd"]
RUN = {
    # what the four census runs reach, as recorded on an MI355X (batch 2, 512 channels at every resolution of the 64^2 generator, frozen
    # decoder: the styled forms)
    ("w2e_torgb_styled_fwd", ("CG16", "V4", "bias")),            # to_rgb1 at 4^2
    ("w2e_torgb_styled_fwd", ("CG16", "V4", "bias+skip")),       # 8^2 ... 32^2
    ("w2e_torgb_styled_fwd", ("CG4", "V4", "bias+skip")),        # 64^2: 1024 quad groups
    ("w2e_torgb_bwd_actbwd", ("V4", "one", "style+acc+noise")),  # pass-through ToRGB behind a fused StyledConv (2 * 512 waves, hw <= 4096: one split)
    ("w2e_torgb_bwd_actbwd", ("V4", "one", "style+noise")),      # the last ToRGB: sole consumer, nothing to fold in
    ("w2e_torgb_styled_bwd", ("V4", "one", "-")),                # the ToRGB behind the blended layer (hooked: plain form)
    ("w2e_bias_act_bwd_reduce", ("float4", "one", "noise")),     # up-sampling StyledConvs below 256 wide (and the hooked layer)
    ("w2e_bias_act_bwd_reduce", ("float4", "split", "noise")),   # 64^2: 1024 rows of 4096
    ("w2e_demod_all_fwd", ()),                                   # the passes whose modulation layers are frozen (mapper step, blend under no_grad): one launch
    ("w2e_demod_fwd", ()),                                       # 9 layers x the three passes that go layer by layer (modulation trainable)
    ("w2e_demod_bwd", ("sums", "slices", "noise_w+bias")),
    ("w2e_demod_bwd", ("sums", "serial", "noise_w+bias")),       # deterministic mode, cout = 512
    ("w2e_style_affine_fwd", ("bias",)),
    ("w2e_style_affine_bwd", ("blocks",)),                       # the mapper step; the two generator passes (one deterministic) go layer by layer
    ("w2e_mask_blend_fwd", ()),
    ("w2e_mask_blend_bwd", ("64 threads", "gmask")),             # features 8 x 8 at layer 4: the cached features carry no gradient
    ("w2e_clip_preproc_fwd", ()),                                # the mapper step's CLIP loss (outside this file's subject, see below)
    ("w2e_clip_preproc_bwd", ()),
}
COVERAGE = {}


def _rows(name, classes, test):
    COVERAGE.update({(name, c): (test, "run" if (name, c) in RUN else "ABI only") for c in classes})


_rows("w2e_torgb_fwd", [(f"CG{cg}", f"V{v}", o) for cg in (1, 4, 16) for v in (1, 4) for o in _FWD_OPS if v == 4 or "skip" not in o], "test_torgb_forward")
_rows("w2e_torgb_styled_fwd", [(f"CG{cg}", f"V{v}", o) for cg in (1, 4, 16) for v in (1, 4) for o in _FWD_OPS if v == 4 or "skip" not in o], "test_torgb_forward")
_rows("w2e_torgb_bwd", [(v, s, "-") for v in ("V1", "V4") for s in ("one", "split")], "test_torgb_backward")
_rows("w2e_torgb_bwd_acc", [(v, s, o) for v in ("V1", "V4") for s in ("one", "split") for o in ("-", "acc")], "test_torgb_backward")
_rows("w2e_torgb_styled_bwd", [(v, s, o) for v in ("V1", "V4") for s in ("one", "split") for o in ("-", "acc")], "test_torgb_backward")
_rows("w2e_torgb_bwd_actbwd", [(v, s, o) for v in ("V1", "V4") for s in ("one", "split") for o in _ACT_OPS], "test_torgb_backward_with_activation_backward")
_rows("w2e_bias_act_fwd", [(b, o) for b in ("float4", "scalar") for o in _BA_OPS] + [("float4-bias", "-"), ("float4-bias", "bias")], "test_bias_act_forward")
_rows("w2e_bias_act_bwd", [("float4",), ("scalar",)], "test_bias_act_backward")
# w2e_bias_act_bwd_reduce: its float4 form with more than one split is the baseline tests/test_gpu_fir_variants.py measures (printed, not
# asserted); here it is held to float64 itself, with the scalar form and the deterministic single split that file does not run
_rows("w2e_bias_act_bwd_reduce", [(k, s, o) for k in ("float4", "scalar") for s in ("one", "split") for o in ("-", "noise")], "test_bias_act_backward_reduce")
_rows("w2e_demod_fwd", [()], "test_demod_forward")
_rows("w2e_demod_all_fwd", [()], "test_demod_all_forward")
_rows("w2e_demod_bwd", [(f, wk, o) for f in ("sums", "dz") for wk in ("slices", "one-slice", "serial") for o in _DM_OPS
                        if f == "sums" or not ({"noise_w", "bias"} & set(o.split("+")))], "test_demod_backward")
_rows("w2e_style_affine_fwd", [("-",), ("bias",)], "test_style_affine")
_rows("w2e_style_affine_bwd", [("blocks",), ("serial",), ("one-block",)], "test_style_affine")
_rows("w2e_mask_blend_fwd", [()], "test_mask_blend")
_rows("w2e_mask_blend_bwd", [(f"{t} threads", o) for t in (64, 128, 256) for o in ("-", "gb", "gmask", "gb+gmask")], "test_mask_blend")
# entry points of csrc/elementwise.hip outside this file's subject: listed so that the table names every entry point of the two files
for _n, _t in (("w2e_clip_preproc_fwd", "test_clip_preprocess_golden"), ("w2e_clip_preproc_bwd", "test_clip_preprocess_golden"),
               ("w2e_id_preproc_fwd", "test_id_preprocess_golden_and_adjoint"), ("w2e_id_preproc_bwd", "test_id_preprocess_golden_and_adjoint")):
    COVERAGE[(_n, ())] = ("test_gpu_parity.py::" + _t, "run" if (_n, ()) in RUN else "ABI only")
OWN = sorted({n for (n, _), (t, _) in COVERAGE.items() if "::" not in t})
# classes the table lists for completeness of the operand grid that no call can form: none -- every row above is reachable


# ---------------------------------------------------------------------------------------------- buffers and judging
@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A kernel fault surfaces at the next synchronisation: end the session there instead of launching more work on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error after this test, nothing more is launched: {e}", returncode=3)


def _lib():
    from where2edit_amd import _lib as L
    return L


def kcall(name, *args):
    L = _lib()
    EXERCISED.add((name, path_class(name, args)))
    L.call(name, *args, L.stream_ptr())


def P(t):
    return _lib().ptr(t)


def _gen(*key):
    return torch.Generator().manual_seed(4000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def rnd(g, *shape):
    return torch.randn(*shape, generator=g)


class Buf:
    """A tensor on the GPU between two runs of GUARD sentinels.  Buf(t): a copy of the CPU tensor t (an input);
    Buf(shape=...): an output, pre-filled with NaN."""

    def __init__(self, t=None, shape=None, fill=float("nan")):
        shape = tuple(t.shape) if t is not None else tuple(shape)
        n = math.prod(shape)
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
        self.v = self.buf[GUARD:GUARD + n].view(shape)
        self.v.copy_(t) if t is not None else self.v.fill_(fill)
        self.n, self.before = n, None
        assert self.v.data_ptr() % 16 == 0 and self.v.is_contiguous()

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        """An output nothing was launched for: still all NaN, guards intact."""
        return self.intact() and bool(torch.isnan(self.v).all())


def inp(t):
    return None if t is None else Buf(t)


def ptr_of(b):
    return None if b is None else P(b.v)


def judge(out, ref, scale, what, bound, tol=1e-5):
    """Every element within `bound` fp32 roundings of float64, relative to ITS OWN term scale; the guards intact; the global norm."""
    assert out.intact(), f"{what}: wrote outside the output"
    got = out.v.detach().double().cpu()
    ref, scale = ref.reshape(got.shape), scale.reshape(got.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written (NaN left) or not finite"
    assert float(got.abs().max()) < 1e-10 * SENTINEL, f"{what}: a sentinel was read"
    ratio = (got - ref).abs() / (U * scale).clamp_min(1e-300)  # (scale == 0: the result must be exact)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = what.split(" [")[0]
    if worst >= WORST.get(key, (-1.0, 0))[0]:
        WORST[key] = (worst, bound)
    print(f"{what}: worst element {worst:.3f} x 2^-24 of its term scale (bound {bound})")
    assert worst <= bound, f"{what}: element {int(ratio.argmax())} is {worst:.3f} x 2^-24 of its term scale from float64 (bound {bound})"
    assert_close(got, ref, tol, what)


def upk4(g):
    """fir_kernel(gain 4) + 0.05 randn: neither separable nor symmetric, so the tap flip and the ky / kx roles show."""
    import seeded
    k = seeded.fir_kernel(gain=4.0) + 0.05 * rnd(g, 4, 4)
    assert not torch.allclose(k, k.t()) and not torch.allclose(k, torch.flip(k, (0, 1))) and torch.linalg.matrix_rank(k) > 1
    return k


def plant_zeros(x):
    """Exact +0 / -0 at a few places of every plane of x [B,C,h,w] (in place): `> 0` against `>= 0`."""
    x[:, :, 0, 0], x[:, :, -1, -1], x[:, :, 1, 2], x[:, :, -2, 1] = 0.0, -0.0, 0.0, -0.0
    return x


def test_torgb_table_is_the_host_arithmetic():
    """TORGB_TABLE (the sizes chosen to reach each dispatch class) equals what torgb_fwd_impl / torgb_bwd_impl compute, and the sizes
    reach every (CG, V) the forward has but <4,1> -- no hw gives 1024 <= hw < 16384 with hw % 4 != 0 AND a different index path from
    <16,1> / <1,1>; (34, 37) below adds it -- and both V with one and with several splits."""
    for (h, w), (fwd, (v, splits, per, last)) in TORGB_TABLE.items():
        assert torgb_fwd_class(h, w) == fwd, (h, w)
        assert torgb_bwd_class(h, w, BATCH, 5, False) == (v, splits, per) and h * w - (splits - 1) * per == last, (h, w)
        assert torgb_bwd_class(h, w, BATCH, 5, True)[1] == 1
    assert torgb_fwd_class(34, 37) == (4, 1)
    assert {f for f, _ in TORGB_TABLE.values()} | {(4, 1)} == {(cg, v) for cg in (1, 4, 16) for v in (1, 4)}
    assert 3 * 300 > 256  # cin = 300: the forward's weight staging loop runs more than once


# ---------------------------------------------------------------------------------------------- ToRGB forward
def _torgb_data(g, h, w, cin):
    x = rnd(g, BATCH, cin, h, w)
    wmod, wsc, style = rnd(g, BATCH, 3, cin) * 0.3, rnd(g, 3, cin) * 0.3, rnd(g, BATCH, cin) + 1.0
    assert not torch.equal(x[0], x[1]) and not torch.equal(wmod[0], wmod[1])
    return x, wmod, wsc, style


@pytest.mark.parametrize("h,w,cin", TORGB_CASES + [(34, 37, 5)], ids=lambda v: str(v))
def test_torgb_forward(h, w, cin):
    """w2e_torgb_fwd and w2e_torgb_styled_fwd: bias NULL / given x skip NULL / given (even h and w).
    Roundings of a pixel: ceil(cin / CG) FMAs of the thread's channel loop + CG - 1 additions of the groups' partial sums + the
    bias + 4 taps of the skip + its addition (+ the product wsc * style of the styled form) <= ceil(cin / CG) + CG + 6."""
    g = _gen(h, w, cin, 1)
    x, wmod, wsc, style = _torgb_data(g, h, w, cin)
    bias, k = rnd(g, 3), upk4(g)
    even = h % 2 == 0 and w % 2 == 0
    skip = rnd(g, BATCH, 3, h // 2, w // 2) if even else None
    cg, v = torgb_fwd_class(h, w)
    bound = -(-cin // cg) + cg + 6
    xb, wb, wscb, stb, bb, kb, sb = inp(x), inp(wmod), inp(wsc), inp(style), inp(bias), inp(k), inp(skip)
    for styled in (False, True):
        for use_bias in (False, True):
            for use_skip in ((False, True) if even else (False,)):
                bi, sk = (bias if use_bias else None), (skip if use_skip else None)
                y = Buf(shape=(BATCH, 3, h, w))
                tail = (ptr_of(bb) if use_bias else None, ptr_of(sb) if use_skip else None, ptr_of(kb) if use_skip else None, P(y.v), BATCH, cin, h, w)
                if styled:
                    kcall("w2e_torgb_styled_fwd", P(xb.v), P(wscb.v), P(stb.v), *tail)
                else:
                    kcall("w2e_torgb_fwd", P(xb.v), P(wb.v), *tail)
                a = (x, wsc if styled else wmod, bi, sk, k, style if styled else None)
                judge(y, R.torgb_fwd(*a), R.torgb_fwd_scale(*a), f"torgb_fwd<{cg},{v}> [{h}x{w} cin {cin} styled {styled} bias {use_bias} skip {use_skip}]", bound)
    assert all(b.intact() for b in (xb, wb, wscb, stb, bb, kb) + ((sb,) if sb else ()))


# ---------------------------------------------------------------------------------------------- ToRGB backward
def _gw_bound(h, w, cin, det, extra=0):
    """ceil(per_split / 64 / V) * V accumulations of a lane + 6 levels of the wave's butterfly + one atomic per split (+ extra)."""
    v, splits, per = torgb_bwd_class(h, w, BATCH, cin, det)
    return -(-per // (64 * v)) * v + 6 + splits + extra


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("h,w,cin", TORGB_CASES, ids=lambda v: str(v))
def test_torgb_backward(h, w, cin, det, w2e_opt):
    """w2e_torgb_bwd, w2e_torgb_bwd_acc and w2e_torgb_styled_bwd with gx_acc NULL / given, in default mode (memset + fp32 atomics
    when the pixels are split) and with "deterministic" = 1 (one split), against the same float64 reference.
    gx: w0*a + w1*b + w2*c is 3 roundings, + gx_acc 1, + the product wsc*style 1 <= 5.  gwmod: _gw_bound; the style gradient
    wsc0*s0 + wsc1*s1 + wsc2*s2 adds 3."""
    w2e_opt("deterministic", str(det))
    g = _gen(h, w, cin, 2)
    x, wmod, wsc, style = _torgb_data(g, h, w, cin)
    gy, acc = rnd(g, BATCH, 3, h, w), rnd(g, BATCH, cin, h, w)
    xb, wb, wscb, stb, gyb, accb = inp(x), inp(wmod), inp(wsc), inp(style), inp(gy), inp(acc)
    v, splits, per = torgb_bwd_class(h, w, BATCH, cin, det)
    for entry in ("w2e_torgb_bwd", "w2e_torgb_bwd_acc", "w2e_torgb_styled_bwd"):
        styled = entry == "w2e_torgb_styled_bwd"
        for use_acc in ((False,) if entry == "w2e_torgb_bwd" else (False, True)):
            gx, gw = Buf(shape=x.shape), Buf(shape=(BATCH, cin) if styled else (BATCH, 3, cin))
            a_ptr = ptr_of(accb) if use_acc else None
            if entry == "w2e_torgb_bwd":
                kcall(entry, P(xb.v), P(wb.v), P(gyb.v), P(gx.v), P(gw.v), BATCH, cin, h, w)
            elif entry == "w2e_torgb_bwd_acc":
                kcall(entry, P(xb.v), P(wb.v), P(gyb.v), a_ptr, P(gx.v), P(gw.v), BATCH, cin, h, w)
            else:
                kcall(entry, P(xb.v), P(wscb.v), P(stb.v), P(gyb.v), a_ptr, P(gx.v), P(gw.v), BATCH, cin, h, w)
            a = (x, wsc if styled else wmod, gy, acc if use_acc else None, style if styled else None)
            (rx, rw), (sx, sw) = R.torgb_bwd(*a), R.torgb_bwd_scale(*a)
            what = f"[{h}x{w} cin {cin} acc {use_acc} det {det}]"
            judge(gx, rx, sx, f"{entry} gx<V{v}> {what}", 5)
            judge(gw, rw, sw, f"{entry} gw<V{v}, {'split' if splits > 1 else 'one'}> {what}", _gw_bound(h, w, cin, det, 3 if styled else 0))
    assert all(b.intact() for b in (xb, wb, wscb, stb, gyb, accb))


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("h,w,cin", [c for c in TORGB_CASES if c[2] in (5, 300) and c[:2] != (10, 6)], ids=lambda v: str(v))
def test_torgb_backward_with_activation_backward(h, w, cin, det, w2e_opt):
    """w2e_torgb_bwd_actbwd: style NULL / given x gx_acc NULL / given x noise NULL / given, two (slope, gain) pairs, exact zeros
    of both signs planted in x (they take the slope).  gpre: the 5 of gx + * gain + * slope = 7.  gw: as w2e_torgb_bwd (x itself).
    sums3: _gw_bound + the 7 of gpre + xval * inv (1) + inv_pos / inv_neg (2: gain * slope, its reciprocal) = + 10."""
    w2e_opt("deterministic", str(det))
    g = _gen(h, w, cin, 3)
    x, wmod, wsc, style = _torgb_data(g, h, w, cin)
    x = plant_zeros(x)
    gy, acc, noise = rnd(g, BATCH, 3, h, w), rnd(g, BATCH, cin, h, w), rnd(g, h * w)
    xb, wb, wscb, stb, gyb, accb, nzb = inp(x), inp(wmod), inp(wsc), inp(style), inp(gy), inp(acc), inp(noise)
    v, splits, per = torgb_bwd_class(h, w, BATCH, cin, det)
    n = 0
    for styled in (False, True):
        for use_acc in (False, True):
            for use_noise in (False, True):
                slope, gain = ACTS[n % 2] if h * w < 1000 else ACTS[0]
                n += 1
                gpre, gw, s3 = Buf(shape=x.shape), Buf(shape=(BATCH, cin) if styled else (BATCH, 3, cin)), Buf(shape=(BATCH, cin, 3))
                kcall("w2e_torgb_bwd_actbwd", P(xb.v), P(wscb.v if styled else wb.v), P(stb.v) if styled else None, P(gyb.v),
                      P(accb.v) if use_acc else None, P(nzb.v) if use_noise else None, P(gpre.v), P(gw.v), P(s3.v), BATCH, cin, h, w, slope, gain)
                a = (x, wsc if styled else wmod, style if styled else None, gy, acc if use_acc else None, noise if use_noise else None, slope, gain)
                refs, scales = R.torgb_bwd_actbwd(*a), R.torgb_bwd_actbwd_scale(*a)
                what = f"[{h}x{w} cin {cin} styled {styled} acc {use_acc} noise {use_noise} slope {slope} det {det}]"
                judge(gpre, refs[0], scales[0], f"w2e_torgb_bwd_actbwd gpre<V{v}> {what}", 7)
                judge(gw, refs[1], scales[1], f"w2e_torgb_bwd_actbwd gw<V{v}> {what}", _gw_bound(h, w, cin, det, 3 if styled else 0))
                judge(s3, refs[2], scales[2], f"w2e_torgb_bwd_actbwd sums3<V{v}> {what}", _gw_bound(h, w, cin, det, 10))
                zero = (x == 0)
                assert int(zero.sum()) == 4 * BATCH * cin
                assert_close(gpre.v.cpu()[zero], refs[0][zero], 1e-6, "x == 0 must take the slope branch")
    assert all(b.intact() for b in (xb, wb, wscb, stb, gyb, accb, nzb))


def test_torgb_refusals_leave_the_outputs_untouched():
    """skip with an odd h, skip without the 4x4 kernel, NULL sums3, slope <= 0: RuntimeError, and nothing was written."""
    g = _gen(9)
    cin = 5
    x, wmod, _, _ = _torgb_data(g, 8, 10, cin)
    xb, wb, kb, sb, gyb = inp(x), inp(wmod), inp(upk4(g)), inp(rnd(g, BATCH, 3, 4, 5)), inp(rnd(g, BATCH, 3, 8, 10))
    y = Buf(shape=(BATCH, 3, 8, 10))
    with pytest.raises(RuntimeError, match="even h,w"):
        kcall("w2e_torgb_fwd", P(xb.v), P(wb.v), None, P(sb.v), P(kb.v), P(y.v), BATCH, cin, 7, 10)
    with pytest.raises(RuntimeError, match="even h,w"):
        kcall("w2e_torgb_fwd", P(xb.v), P(wb.v), None, P(sb.v), P(kb.v), P(y.v), BATCH, cin, 8, 9)
    with pytest.raises(RuntimeError, match="4x4 kernel"):
        kcall("w2e_torgb_fwd", P(xb.v), P(wb.v), None, P(sb.v), None, P(y.v), BATCH, cin, 8, 10)
    assert y.untouched()
    gpre, gw, s3 = Buf(shape=x.shape), Buf(shape=(BATCH, 3, cin)), Buf(shape=(BATCH, cin, 3))
    with pytest.raises(RuntimeError, match="null sums"):
        kcall("w2e_torgb_bwd_actbwd", P(xb.v), P(wb.v), None, P(gyb.v), None, None, P(gpre.v), P(gw.v), None, BATCH, cin, 8, 10, SLOPE, GAIN)
    for slope in (0.0, -0.2):
        with pytest.raises(RuntimeError, match="must be positive"):
            kcall("w2e_torgb_bwd_actbwd", P(xb.v), P(wb.v), None, P(gyb.v), None, None, P(gpre.v), P(gw.v), P(s3.v), BATCH, cin, 8, 10, slope, GAIN)
    assert gpre.untouched() and gw.untouched() and s3.untouched()
    kcall("w2e_torgb_fwd", P(xb.v), P(wb.v), None, P(sb.v), P(kb.v), P(y.v), BATCH, cin, 8, 10)
    assert bool(torch.isfinite(y.v).all()), "the same buffers with the right arguments are accepted"


# ---------------------------------------------------------------------------------------------- bias + noise + LeakyReLU * gain
GRID_PASS = 2048 * 256  # stream_grid (csrc/common.h): elements (quads for the float4 kernels) one pass of the grid covers
# (outer, C, inner), branch
BIAS_ACT_CASES = [((2, 5, 60), "float4"), ((2, 5, 456 * 460), "float4"), ((3, 8, 1), "float4-bias"), ((3, 512, 1), "float4-bias"),
                  ((3, 5, 1), "scalar"), ((2, 5, 63), "scalar"), ((2, 5, 227 * 231), "scalar")]


def _kink_free(g, shape, bias, noise, nw):
    """x such that x + bias + nw*noise is at least 0.05 from 0: the activation's branch is the same in fp32 and float64 (the mask of
    the FORWARD comes from a rounded sum; nothing is excluded, the inputs just hold no sum within rounding of the kink)."""
    v = rnd(g, *shape)
    v = torch.where(v.abs() < 0.05, torch.full_like(v, 0.05) * torch.where(v < 0, -1.0, 1.0), v)
    if bias is not None:
        v = v - bias.reshape(1, -1, 1)
    if noise is not None:
        v = v - (nw.double() * noise.double()).float().reshape(1, 1, -1)
    return v


@pytest.mark.parametrize("shape,branch", BIAS_ACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_bias_act_forward(shape, branch):
    """w2e_bias_act_fwd on its three branches -- float4 over inner (6x10; 456x460 x 10 planes = 2097600 elements: more than one pass of
    the grid over quads), the float4 bias load for inner == 1, C % 4 == 0 without noise (C = 8, 512), scalar (inner 1 with noise or
    C = 5; inner 63; 227x231 x 10 planes: more than one pass) -- with bias / noise NULL or given and two (slope, gain) pairs.
    Roundings: x + bias, * slope, * gain = 3; with noise the FMA nw * noise + (.) is one more = 4."""
    outer, c, inner = shape
    g = _gen(*shape, 4)
    big = outer * c * inner > 100000
    assert not big or (outer * c * inner >> (2 if branch == "float4" else 0)) > GRID_PASS
    bias, noise, nw = rnd(g, c), rnd(g, inner), rnd(g, 1) * 0.5 + 1.0
    bb, nb, nwb = inp(bias), inp(noise), inp(nw)
    for ops in (["bias+noise", "-"] if big else _BA_OPS):
        bi, nz = (bias if "bias" in ops else None), (noise if "noise" in ops else None)
        x = _kink_free(g, shape, bi, nz, nw)
        xb = inp(x)
        for slope, gain in (ACTS[:1] if big else ACTS):
            y = Buf(shape=shape)
            kcall("w2e_bias_act_fwd", P(xb.v), P(bb.v) if bi is not None else None, P(nb.v) if nz is not None else None,
                  P(nwb.v) if nz is not None else None, P(y.v), outer, c, inner, slope, gain)
            got = path_class("w2e_bias_act_fwd", (None, bi is not None, nz is not None, None, None, outer, c, inner))[0]
            want = branch if not (branch == "float4-bias" and nz is not None) else "scalar"
            assert got == want, (got, want)
            a = (x, bi, nz, nw if nz is not None else None, slope, gain)
            judge(y, R.bias_act_fwd(*a), R.bias_act_fwd_scale(*a), f"w2e_bias_act_fwd {want} [{shape} ({ops}) slope {slope}]", 4 if nz is not None else 3)
        assert xb.intact()
    assert bb.intact() and nb.intact() and nwb.intact()


@pytest.mark.parametrize("n", [60, 61, 2097600, 524369])
def test_bias_act_backward(n):
    """w2e_bias_act_bwd at n % 4 == 0 (float4) and == 1 (scalar), below and above one pass of the grid; zeros of both signs in y take
    the slope.  Roundings: gy * gain, * (1 | slope) = 2 <= 3."""
    g = _gen(n, 5)
    gy, y = rnd(g, n), rnd(g, n)
    y[0], y[n // 2], y[-1], y[7] = 0.0, -0.0, 0.0, -0.0
    gyb, yb = inp(gy), inp(y)
    for slope, gain in ACTS:
        gx = Buf(shape=(n,))
        kcall("w2e_bias_act_bwd", P(gyb.v), P(yb.v), P(gx.v), n, slope, gain)
        judge(gx, R.bias_act_bwd(gy, y, slope, gain), R.bias_act_bwd_scale(gy, y, slope, gain), f"w2e_bias_act_bwd [{n} slope {slope}]", 3)
        assert int((y == 0).sum()) == 4  # (judged with the rest: the reference gives them the slope, a factor 1 / slope away from the other branch)
    assert gyb.intact() and yb.intact()


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("inner", [63, 2051, 66 * 70])
def test_bias_act_backward_reduce(inner, det, w2e_opt):
    """w2e_bias_act_bwd_reduce at [2, 5, inner]: the scalar form with one split (inner 63) and with 3 (2051, the last one short), the
    float4 form with 5 splits of a row (4620), and the single split of the deterministic mode -- the cases tests/test_gpu_fir_variants.py does not hold to float64
    (test_actbwd_stream_against_float64 there measures the float4 form at w >= 256 as the fused kernel's baseline, printed only).
    sums: ceil(per / 256 / V) * V accumulations of a thread + 6 (butterfly) + 3 (the four waves) + splits + the 10 local roundings
    of w2e_torgb_bwd_actbwd's sums (there 7 of gpre; here 2: the rest is slack of the same formula)."""
    w2e_opt("deterministic", str(det))
    g = _gen(inner, 6)
    shape = (2, 5, inner)
    gy, y, noise = rnd(g, *shape), rnd(g, *shape), rnd(g, inner)
    y[:, :, 0], y[:, :, -1] = 0.0, -0.0
    gyb, yb, nb = inp(gy), inp(y), inp(noise)
    cls = path_class("w2e_bias_act_bwd_reduce", (None, None, None, None, None, 2, 5, inner))
    splits = reduce_splits(10, inner, det)
    assert splits == (1 if det else {63: 1, 2051: 3, 4620: 5}[inner])
    assert cls[:2] == ("float4" if inner % 4 == 0 else "scalar", "split" if splits > 1 else "one")
    v = 4 if inner % 4 == 0 else 1
    per = (-(-inner // splits) + 3) & ~3
    bound = -(-per // (256 * v)) * v + 6 + 3 + splits + 10
    for use_noise in (False, True):
        gx, sums = Buf(shape=shape), Buf(shape=(2, 5, 3))
        kcall("w2e_bias_act_bwd_reduce", P(gyb.v), P(yb.v), P(nb.v) if use_noise else None, P(gx.v), P(sums.v), 2, 5, inner, SLOPE, GAIN)
        a = (gy, y, noise if use_noise else None, SLOPE, GAIN)
        (rx, rs), (sx, ss) = R.bias_act_bwd_reduce(*a), R.bias_act_bwd_reduce_scale(*a)
        judge(gx, rx, sx, f"w2e_bias_act_bwd_reduce gx [{inner} noise {use_noise} det {det}]", 3)
        judge(sums, rs, ss, f"w2e_bias_act_bwd_reduce sums [{inner} noise {use_noise} det {det}]", bound)
    assert gyb.intact() and yb.intact() and nb.intact()


# ---------------------------------------------------------------------------------------------- demodulation
DEMOD_SHAPES = [(5, 5), (64, 32), (65, 33), (300, 70), (257, 96)]  # (cin, cout): ragged against 64 lanes, 32-channel slices, 256-channel blocks
DB = 3
EPS = 1e-8


def _demod_inputs(g, cin, cout):
    s = rnd(g, DB, cin) + 1.0
    wsq = (rnd(g, cout, cin, 9) * (cin * 9) ** -0.5).pow(2).sum(2)
    return s, wsq


def _demod_bound(cin):
    """The sum: ceil(cin / 64) FMAs of a lane + 6 levels of the butterfly (+ v*v and + eps: 2), all terms >= 0, so its relative
    error is at most that many 2^-24; rsqrt halves a relative error; device rsqrtf itself: RSQRT_ULP ulp = 2 * RSQRT_ULP * 2^-24."""
    return (-(-cin // 64) + 6 + 2) / 2 + 2 * RSQRT_ULP


@pytest.mark.parametrize("cin,cout", DEMOD_SHAPES)
def test_demod_forward(cin, cout):
    g = _gen(cin, cout, 7)
    s, wsq = _demod_inputs(g, cin, cout)
    sb, wb, d = inp(s), inp(wsq), Buf(shape=(DB, cout))
    kcall("w2e_demod_fwd", P(sb.v), P(wb.v), P(d.v), DB, cin, cout, EPS)
    judge(d, R.demod_fwd(s, wsq, EPS), R.demod_fwd_scale(s, wsq, EPS), f"w2e_demod_fwd [{cin}->{cout}]", _demod_bound(cin))
    assert sb.intact() and wb.intact()


@pytest.mark.parametrize("n_layers", [1, 3, 32])
def test_demod_all_forward(n_layers):
    """1, 3 and 32 layers of DIFFERENT cout in one launch (the grid is sized by the widest: the rows past a narrow layer's end must
    return); each d between its own sentinels.  33 layers are refused and nothing is written."""
    L = _lib()
    g = _gen(n_layers, 8)
    shapes = [DEMOD_SHAPES[(j + 2) % len(DEMOD_SHAPES)] for j in range(n_layers)]
    assert n_layers == 1 or len({c for _, c in shapes}) > 1
    data = [_demod_inputs(g, cin, cout) for cin, cout in shapes]
    bufs = [(inp(s), inp(wsq), Buf(shape=(DB, cout))) for (s, wsq), (_, cout) in zip(data, shapes)]

    def descs(n):
        arr = (L.DemodLayer * n)()
        for j in range(n):
            sb, wb, d = bufs[j % n_layers]
            cin, cout = shapes[j % n_layers]
            arr[j].s, arr[j].wsq, arr[j].d, arr[j].cin, arr[j].cout = P(sb.v).value, P(wb.v).value, P(d.v).value, cin, cout
        return arr

    if n_layers == 32:
        with pytest.raises(RuntimeError, match="n_layers"):
            kcall("w2e_demod_all_fwd", descs(33), 33, DB, EPS)
        assert all(d.untouched() for _, _, d in bufs)
    kcall("w2e_demod_all_fwd", descs(n_layers), n_layers, DB, EPS)
    for (s, wsq), (cin, cout), (sb, wb, d) in zip(data, shapes, bufs):
        judge(d, R.demod_fwd(s, wsq, EPS), R.demod_fwd_scale(s, wsq, EPS), f"w2e_demod_all_fwd [{n_layers} layers, {cin}->{cout}]", _demod_bound(cin))
        assert sb.intact() and wb.intact()


@pytest.mark.parametrize("det", [0, 1], ids=["default", "deterministic"])
@pytest.mark.parametrize("cin,cout", DEMOD_SHAPES)
def test_demod_backward(cin, cout, det, w2e_opt):
    """w2e_demod_bwd: the `sums` form with noise_w / bias NULL or given and the `dz` form, gd NULL / given, gs holding a non-zero
    direct part on entry that is added onto; default mode (one block per 32 output channels, atomics) and deterministic mode (cout
    <= 32: the one slice; cout >= 33: the serial walk over the slices).  Both or neither of sums / dz: refused, gs keeps every bit.
    gs: dz from the sums 4 + dz*d*d 2 + min(cout, 32) FMAs of a slice + (-s * acc) 1 + one addition per slice onto gs
    (ceil(cout / 32); the serial walk: the same number onto `total`, + 1) <= min(cout, 32) + ceil(cout / 32) + 8.  gd: dz 4 + the division 1."""
    w2e_opt("deterministic", str(det))
    g = _gen(cin, cout, 9)
    s, wsq = _demod_inputs(g, cin, cout)
    d = R.demod_fwd(s, wsq, EPS).float()
    sums, dz, nw, bias, gs0 = rnd(g, DB, cout, 3), rnd(g, DB, cout), rnd(g, 1), rnd(g, cout), rnd(g, DB, cin)
    sb, wb, db, sumb, dzb, nwb, bb = inp(s), inp(wsq), inp(d), inp(sums), inp(dz), inp(nw), inp(bias)
    bound = min(cout, 32) + -(-cout // 32) + 8
    for form, use_nw, use_bias in (("sums", False, False), ("sums", True, False), ("sums", False, True), ("sums", True, True), ("dz", False, False)):
        for use_gd in (False, True):
            gs, gd = Buf(gs0), Buf(shape=(DB, cout))
            kcall("w2e_demod_bwd", P(sumb.v) if form == "sums" else None, P(dzb.v) if form == "dz" else None, P(nwb.v) if use_nw else None,
                  P(bb.v) if use_bias else None, P(db.v), P(sb.v), P(wb.v), P(gs.v), P(gd.v) if use_gd else None, DB, cin, cout)
            a = (sums if form == "sums" else None, dz if form == "dz" else None, nw if use_nw else None, bias if use_bias else None, d, s, wsq, gs0)
            (rs, rd), (ss, sd) = R.demod_bwd(*a), R.demod_bwd_scale(*a)
            what = f"[{cin}->{cout} {form} noise_w {use_nw} bias {use_bias} det {det}]"
            judge(gs, rs, ss, f"w2e_demod_bwd gs {what}", bound)
            if use_gd:
                judge(gd, rd, sd, f"w2e_demod_bwd gd {what}", 5)
            else:
                assert gd.untouched()
    gs = Buf(gs0)
    for both in ((P(sumb.v), P(dzb.v)), (None, None)):
        with pytest.raises(RuntimeError, match="exactly one of sums / dz"):
            kcall("w2e_demod_bwd", *both, None, None, P(db.v), P(sb.v), P(wb.v), P(gs.v), None, DB, cin, cout)
    assert torch.equal(gs.v.cpu(), gs0) and gs.intact()
    assert all(b.intact() for b in (sb, wb, db, sumb, dzb, nwb, bb))


# ---------------------------------------------------------------------------------------------- the stacked style affines
LAYERS = [(0, 32), (2, 64), (2, 32), (3, 96)]  # (W+ index, width): index 2 is shared (the gradients add), index 1 is used by no layer
N_LATENT = 4


def _meta(layers):
    rows, off = [], 0
    for widx, cw in layers:
        rows += [[widx, off, cw, r] for r in range(cw)]
        off += cw
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dim", [8, 260, 512])
@pytest.mark.parametrize("layers", [LAYERS, [(1, 32)]], ids=["4 layers", "1 layer"])
def test_style_affine(layers, dim, batch, w2e_opt):
    """w2e_style_affine_fwd / _bwd on four stacked layers (224 rows) and on one layer of 32 rows (in deterministic mode: the one block
    that is no serial walk): dim 8 (fewer than one pass of 64 lanes x 4), 260 (lane 0 takes
    a second pass) and 512; bias NULL / given; the backward in both modes, glatent pre-filled with NaN (the kernel zeroes it), the
    rows of the unused W+ index exactly 0.
    fwd: ceil(dim / 256) passes of (4 roundings of the float4's products and sum + 1 accumulation) + 6 (butterfly) + bias.
    bwd: 32 FMAs over the rows of a group + one addition per group of the W+ index (at most 224 / 32 = 7)."""
    import ctypes
    g = _gen(dim, batch, 10)
    LAYERS = layers
    rows = sum(cw for _, cw in LAYERS)
    latent, w, bias = rnd(g, batch, N_LATENT, dim), rnd(g, rows, dim) * dim ** -0.5, rnd(g, rows)
    meta = _meta(LAYERS).to(DEV)
    mp = ctypes.c_void_p(meta.data_ptr())
    lb, wb, bb = inp(latent), inp(w), inp(bias)
    for use_bias in (False, True):
        out = Buf(shape=(batch * rows,))
        kcall("w2e_style_affine_fwd", P(lb.v), P(wb.v), P(bb.v) if use_bias else None, mp, P(out.v), batch, N_LATENT, dim, rows)
        a = (latent, w, bias if use_bias else None, LAYERS)
        ref = torch.cat([t.reshape(-1) for t in R.style_affine_fwd(*a)])
        scale = torch.cat([t.reshape(-1) for t in R.style_affine_fwd_scale(*a)])
        judge(out, ref, scale, f"w2e_style_affine_fwd [{len(LAYERS)} layers dim {dim} batch {batch} bias {use_bias}]", 5 * -(-dim // 256) + 7)
    gouts = [rnd(g, batch, cw) for _, cw in LAYERS]
    gb = inp(torch.cat([t.reshape(-1) for t in gouts]))
    ref, scale = R.style_affine_bwd(gouts, w, LAYERS, N_LATENT), R.style_affine_bwd_scale(gouts, w, LAYERS, N_LATENT)
    for det in (0, 1):
        w2e_opt("deterministic", str(det))
        gl = Buf(shape=(batch, N_LATENT, dim))
        kcall("w2e_style_affine_bwd", P(gb.v), P(wb.v), mp, P(gl.v), batch, N_LATENT, dim, rows)
        judge(gl, ref, scale, f"w2e_style_affine_bwd [{len(LAYERS)} layers dim {dim} batch {batch} det {det}]", 32 + rows // 32)
        unused = sorted(set(range(N_LATENT)) - {widx for widx, _ in LAYERS})
        assert unused and bool((gl.v[:, unused] == 0).all()), "a W+ index no layer uses must have an exactly zero gradient"
    assert lb.intact() and wb.intact() and bb.intact() and gb.intact()


# ---------------------------------------------------------------------------------------------- region-attention blend
MASK_CASES = [(6, 10, 5), (10, 6, 3), (12, 20, 4), (5, 7, 9), (8, 130, 8), (4, 260, 4)]  # non-integer ratios, a mask larger than the features, 64 / 128 / 256 threads


@pytest.mark.parametrize("c", [1, 5])
@pytest.mark.parametrize("h,w,ms", MASK_CASES)
def test_mask_blend(h, w, ms, c):
    """w2e_mask_blend_fwd / _bwd with gb / gmask NULL or given.  The nearest index is min(floor(dst * fp32(ms / size)), ms - 1) as torch
    computes it; the reference builds it the same way (gen_small_ref.nearest_index: fp32 scale).  Cells no pixel maps to are exactly 0.
    out: m*a, 1 - m, FMA = 3.  ga / gb: 1 / 2.  gmask: a - b (1) + C FMAs + one atomic per pixel of the cell."""
    g = _gen(h, w, ms, c, 11)
    a, b, gout = (rnd(g, BATCH, c, h, w) for _ in range(3))
    mask = torch.rand(BATCH, 1, ms, ms, generator=g)
    ab, bb, mb, gob = inp(a), inp(b), inp(mask), inp(gout)
    out = Buf(shape=a.shape)
    kcall("w2e_mask_blend_fwd", P(ab.v), P(bb.v), P(mb.v), P(out.v), BATCH, c, h, w, ms)
    judge(out, R.mask_blend_fwd(a, b, mask), R.mask_blend_fwd_scale(a, b, mask), f"w2e_mask_blend_fwd [{h}x{w} ms {ms} C {c}]", 3)
    refs, scales = R.mask_blend_bwd(gout, a, b, mask), R.mask_blend_bwd_scale(gout, a, b, mask)
    cells = R.pixels_per_cell(h, ms)[:, None] * R.pixels_per_cell(w, ms)[None, :]
    for use_gb in (False, True):
        for use_gm in (False, True):
            ga, gb, gm = Buf(shape=a.shape), Buf(shape=a.shape), Buf(shape=mask.shape)
            kcall("w2e_mask_blend_bwd", P(gob.v), P(ab.v), P(bb.v), P(mb.v), P(ga.v), P(gb.v) if use_gb else None, P(gm.v) if use_gm else None,
                  BATCH, c, h, w, ms)
            what = f"[{h}x{w} ms {ms} C {c} gb {use_gb} gmask {use_gm}]"
            judge(ga, refs[0], scales[0], f"w2e_mask_blend_bwd ga {what}", 3)
            if use_gb:
                judge(gb, refs[1], scales[1], f"w2e_mask_blend_bwd gb {what}", 3)
            else:
                assert gb.untouched()
            if use_gm:
                judge(gm, refs[2], scales[2], f"w2e_mask_blend_bwd gmask {what}", 1 + c + int(cells.max()))
                assert bool((gm.v.cpu()[:, 0][:, cells == 0] == 0).all()), "a cell no pixel maps to must be exactly 0"
            else:
                assert gm.untouched()
    assert all(x.intact() for x in (ab, bb, mb, gob))


def test_mask_blend_in_deterministic_mode(w2e_opt):
    """"deterministic" = 1: h == w == ms (one add per cell) is accepted and meets the reference; another geometry is refused when gmask
    is asked for (nothing written) and still runs when it is not."""
    w2e_opt("deterministic", "1")
    g = _gen(12)
    c = 5
    for h, w, ms in ((7, 7, 7), (6, 10, 5)):
        a, b, gout = (rnd(g, BATCH, c, h, w) for _ in range(3))
        mask = torch.rand(BATCH, 1, ms, ms, generator=g)
        ab, bb, mb, gob = inp(a), inp(b), inp(mask), inp(gout)
        refs, scales = R.mask_blend_bwd(gout, a, b, mask), R.mask_blend_bwd_scale(gout, a, b, mask)
        ga, gb, gm = Buf(shape=a.shape), Buf(shape=a.shape), Buf(shape=mask.shape)
        args = lambda gmask: (P(gob.v), P(ab.v), P(bb.v), P(mb.v), P(ga.v), P(gb.v), gmask, BATCH, c, h, w, ms)
        if h == w == ms:
            kcall("w2e_mask_blend_bwd", *args(P(gm.v)))
            judge(gm, refs[2], scales[2], f"w2e_mask_blend_bwd gmask [deterministic {h}x{w} ms {ms}]", 1 + c + 1)
        else:
            with pytest.raises(RuntimeError, match="deterministic mode needs the mask at the feature resolution"):
                kcall("w2e_mask_blend_bwd", *args(P(gm.v)))
            assert ga.untouched() and gb.untouched() and gm.untouched(), "a refused call wrote (gmask was once zeroed before the refusal)"
            kcall("w2e_mask_blend_bwd", *args(None))
            assert gm.untouched()
        judge(ga, refs[0], scales[0], f"w2e_mask_blend_bwd ga [deterministic {h}x{w} ms {ms}]", 3)
        judge(gb, refs[1], scales[1], f"w2e_mask_blend_bwd gb [deterministic {h}x{w} ms {ms}]", 3)


# ---------------------------------------------------------------------------------------------- the census
def entry_points():
    """The extern "C" entry points csrc/torgb.hip and csrc/elementwise.hip define, read from the sources."""
    names = set()
    for f in ("torgb.hip", "elementwise.hip"):
        src = open(os.path.join(ROOT, "where2edit_amd", "csrc", f)).read()
        names |= set(re.findall(r"^(?:extern \"C\" )?int (w2e_\w+)\(", src, re.M))
    return sorted(names)


def test_path_class_reads_the_arguments_the_wrappers_pass():
    L = _lib()
    x = torch.zeros(64, device=DEV)
    p, null = L.ptr(x), L.ptr(None)
    assert path_class("w2e_torgb_fwd", (p, p, p, null, null, p, 2, 5, 66, 70)) == ("CG4", "V4", "bias")
    assert path_class("w2e_torgb_styled_fwd", (p, p, p, null, p, p, p, 2, 5, 256, 260)) == ("CG1", "V4", "skip")
    assert path_class("w2e_torgb_bwd", (p, p, p, p, p, 2, 5, 127, 131)) == ("V1", "split", "-")
    assert path_class("w2e_torgb_bwd_acc", (p, p, p, p, p, p, 2, 5, 6, 10)) == ("V4", "one", "acc")
    assert path_class("w2e_torgb_styled_bwd", (p, p, p, p, null, p, p, 2, 5, 66, 70)) == ("V4", "split", "-")
    assert path_class("w2e_torgb_bwd_actbwd", (p, p, p, p, null, p, p, p, p, 2, 5, 7, 9, 0.2, 1.4)) == ("V1", "one", "style+noise")
    assert path_class("w2e_bias_act_fwd", (p, p, null, null, p, 3, 8, 1, 0.2, 1.4)) == ("float4-bias", "bias")
    assert path_class("w2e_bias_act_fwd", (p, p, p, p, p, 3, 8, 1, 0.2, 1.4)) == ("scalar", "bias+noise")
    assert path_class("w2e_bias_act_bwd", (p, p, p, 61, 0.2, 1.4)) == ("scalar",)
    assert path_class("w2e_demod_bwd", (p, null, p, null, p, p, p, p, p, 3, 65, 33)) == ("sums", "slices", "noise_w+gd")
    assert path_class("w2e_style_affine_bwd", (p, p, p, p, 3, 4, 8, 224)) == ("blocks",)
    assert path_class("w2e_mask_blend_bwd", (p, p, p, p, p, null, p, 2, 5, 8, 130, 8)) == ("128 threads", "gmask")


def test_coverage_table_names_every_entry_point_and_existing_tests():
    import test_gpu_fir_variants  # noqa: F401  (named in the docstrings as what covers the fused FIR forms)
    import test_gpu_parity
    assert sorted({name for name, _ in COVERAGE}) == entry_points()
    for (name, cls), (test, reach) in COVERAGE.items():
        assert reach in ("run", "ABI only"), (name, cls, reach)
        where, fn = (test_gpu_parity, test.split("::")[1]) if "::" in test else (None, test)
        assert callable(getattr(where, fn) if where else globals().get(fn)), f"{name} {cls}: no test named {test}"
    assert not [k for k in RUN if k not in COVERAGE], "RUN names a class the table does not have"


def test_census_of_the_paths_real_runs_take(monkeypatch, w2e_opt):
    """Four runs with every call of the library recorded as (entry point, path class): (1) one 64^2 generator forward + backward
    (frozen decoder: ToRGB pass-through and ActLink), (2) the same with "deterministic" = 1, (3) one mapper step as
    tests/test_gpu_step.py builds it at 64^2, (4) one region-attention blend forward + backward through the attention generator.
    Every recorded pair is a COVERAGE row marked "run", every "run" row was recorded, and every entry point this file tests was seen
    at least once -- so an empty record (calls routed past where2edit_amd._lib.call) fails."""
    import sys

    import seeded
    import test_gpu_parity as TP
    import test_gpu_step as TS
    from oracle import stylegan2 as OG
    from where2edit_amd import _lib as L
    from where2edit_amd.attention_model import Generator as AttGenerator
    names = set(entry_points())
    seen = {}
    real_call = L.call

    def recording(name, *args):
        if name in names:
            key = (name, path_class(name, args))
            seen[key] = seen.get(key, 0) + 1
        return real_call(name, *args)

    # where2edit_amd._lib.call, and the name every module of the package bound it to at import (`from ._lib import call`)
    monkeypatch.setattr(L, "call", recording)
    for mod in list(sys.modules.values()):
        if getattr(mod, "__name__", "").startswith("where2edit_amd") and getattr(mod, "call", None) is real_call:
            monkeypatch.setattr(mod, "call", recording)

    def generator_pass():
        gen = TP._gen(64)
        w = seeded.wplus_latents(2, gen.n_latent, salt=3).to(DEV).requires_grad_(True)
        img, _ = gen([w], input_is_latent=True, randomize_noise=False)
        torch.autograd.grad((img * seeded.tensor("g64.r", img.shape).to(DEV)).sum(), w)

    generator_pass()
    w2e_opt("deterministic", "1")
    generator_pass()
    w2e_opt("deterministic", "0")
    coach, _, _ = TS._coach(TS._opts())
    coach.train_step(seeded.wplus_latents(2, OG.n_latent(64), salt=21).to(DEV))
    ga = TP._gen(64, AttGenerator)
    w = seeded.wplus_latents(2, ga.n_latent, salt=5).to(DEV)
    with torch.no_grad():
        _, _, _, feats = ga([w], input_is_latent=True, randomize_noise=False, return_features=True)
    w2 = (w + 0.2 * seeded.tensor("census.dw", w.shape).to(DEV)).requires_grad_(True)
    mask = torch.rand(2, 1, 8, 8, generator=torch.Generator().manual_seed(3)).to(DEV).requires_grad_(True)
    img = ga([w2], input_is_latent=True, randomize_noise=False, return_features=True, attention_layer=4, attention_map=mask, feature_map=feats)[0]
    torch.autograd.grad((img * seeded.tensor("g64.r", img.shape).to(DEV)).sum(), (w2, mask))
    torch.cuda.synchronize()
    for key in sorted(seen):
        print(f"census: {seen[key]:4d} x {key[0]} {key[1]}")
    unknown = sorted(k for k in seen if k not in COVERAGE)
    assert not unknown, f"paths real runs take that COVERAGE has no test for: {unknown}"
    abi_only = sorted(k for k in seen if COVERAGE[k][1] == "ABI only")
    assert not abi_only, f"COVERAGE lists as ABI only what real runs do reach: {abi_only}"
    unreached = sorted(k for k, v in COVERAGE.items() if v[1] == "run" and k not in seen)
    assert not unreached, f"COVERAGE lists as run what these four runs never reach: {unreached}"
    assert seen, "nothing was recorded: do the calls still go through where2edit_amd._lib.call?"


def test_zz_every_coverage_row_was_exercised_and_worst_ratios(request):
    """After the tests above (file order): every COVERAGE row that names a test of this file was really called with that path class by
    this file's tests -- checked when the whole file ran -- and the table of worst measured ratios (DESIGN.md quotes it)."""
    for key in sorted(WORST):
        print(f"worst: {WORST[key][0]:8.3f} of {WORST[key][1]:<7} {key}")
    whole_file = not request.config.getoption("keyword") and not any("::" in a for a in request.config.args)
    if whole_file:
        missing = sorted(k for k, (t, _) in COVERAGE.items() if "::" not in t and k not in EXERCISED)
        assert not missing, f"COVERAGE rows no test of this file exercised: {missing}"
