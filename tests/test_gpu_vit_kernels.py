"""The CLIP transformer kernels one by one against the float64 restatement of tests/vit_ref.py (held to oracle/clip_model.py and to
autograd by tests/test_vit_ref_host.py): w2e_gemm_ex, w2e_layernorm_*, w2e_attn_* of csrc/vit.hip, the slab consumers and the MFMA
attention of csrc/vit2.hip, the packings and register-fed GEMMs of csrc/vit3.hip, called through the C ABI at the smallest shapes at
which each tiling can still go wrong.  All inputs come from seeded CPU generators, in three families (vit_ref.family): plain, clip-like
(peaked logits, a head with K = 0, a row of mean 50, a constant row, massive channels) and qgelu-wide.  Outputs are pre-filled with
NaN and sit between sentinels; row gaps (lda / ldb > k, slab strides) hold NaN that must never be read, output gaps (ldc > n, the padded
rows of a packed output) hold sentinels that must survive.  A census of what the towers really launch is held against EXERCISED.

How the error is judged.  Every ELEMENT against its own term scale (vit_ref.*_scale): |got - ref| <= N * 2^-24 * scale with N =
vit_ref.*_bound, counted from the kernel source (the header of tests/test_gpu_gen_small_kernels.py describes the counting; N is a
tensor where the count depends on the data).  No element is excluded.  Beside it the global helpers.assert_close at the tolerance
tests/test_gpu_clip.py holds the same kernel to -- on the plain family only: on the other two the element bound is the statement
(a tolerance on max |a - b| / max |b| there would have to come from the measured values).  `-s` prints every comparison; the last test
prints the table of worst ratios that DESIGN.md quotes."""
import ctypes
import math

import pytest
import torch

import vit_ref as R
from helpers import assert_close
from test_gpu_gen_small_kernels import GUARD, SENTINEL, Buf, P, _stop_after_a_gpu_fault, inp, ptr_of  # noqa: F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
EPS = float(torch.tensor(1e-5, dtype=torch.float32))  # the float the ABI receives
PAD = 777.0    # what the padded rows of a packed output hold before the launch
WORST = {}     # what -> (worst measured ratio in 2^-24 of the term scale, the bound at that element, its share of the bound)
EXERCISED = set()  # (entry point, path class) of every call this file's tests made
GEMM_CLASSES = {}  # (trans_b, a_gelu, aux) -> the set of {"split", "single"} the c_is_zero constant showed
CENSUS = {}    # (entry point, path class) -> calls, of the towers' own passes (test_census_of_the_paths_the_towers_take)
TUNE = [0]     # the "tune_gemm_s" the tests set (the library has no getter for it)
FAMS = ["plain", "clip-like"]


def _lib():
    from where2edit_amd import _lib as L
    return L


def _gen(*key):
    return torch.Generator().manual_seed(9000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


# ---------------------------------------------------------------------------------------------- the host dispatch, restated
def _addr(p):
    v = getattr(p, "value", p)
    return 0 if v is None else int(v)


def _int(v):
    return int(getattr(v, "value", v))


def gemm_splits(m, n, k, ldc, det, tune):
    """The slice count of w2e_gemm_ex: the cost model (ldc == n only), "tune_gemm_s", "deterministic", then the 128-multiple clip."""
    want = 1
    if ldc == n:
        want = tune if tune > 0 else R.gemm_cost_splits(m, n, k)
        want = 1 if det else want
    return R.gemm_split(k, want)[0]


def path_class(name, args):
    """The path class of one call, from the arguments handed to the library: what the host dispatch looks at."""
    al = lambda *ps: all(_addr(p) % 16 == 0 for p in ps)  # noqa: E731
    vec = lambda dim, *ps: "vector" if _int(dim) in (512, 768, 1024) and al(*ps) else "generic"  # noqa: E731
    pk = lambda v: "packed" if _addr(v) else "row-major"  # noqa: E731
    if name in ("w2e_gemm_ex", "w2e_gemm"):
        m, n, k, _, _, ldc, trans_b, a_gelu = (_int(v) for v in args[3:11])
        ciz = _int(args[14]) if name == "w2e_gemm_ex" else 0
        sp = gemm_splits(m, n, k, ldc, bool(_lib().get_option("deterministic")), TUNE[0])
        return (trans_b, a_gelu, "aux" if _addr(args[13]) else "-", "split" if sp > 1 else "single", int(bool(ciz)))
    if name == "w2e_layernorm_fwd":
        return (vec(args[7], args[0], args[3], args[1], args[2]),)
    if name == "w2e_layernorm_bwd":
        return (vec(args[7], args[0], args[1], args[2], args[5]), "-")
    if name == "w2e_layernorm_bwd_add":
        return (vec(args[8], args[0], args[1], args[2], args[6], args[5]), "add" if _addr(args[5]) else "-")
    if name == "w2e_reduce_ln_fwd":
        return ("no y" if not _addr(args[8]) else pk(args[14]),)
    if name == "w2e_layernorm_bwd_part":
        return (pk(args[11]),)
    if name == "w2e_reduce_gelu":
        return (_int(args[9]), pk(args[10]))
    if name in ("w2e_attn2_fwd", "w2e_attn_causal_fwd"):
        return (pk(args[8]),)
    if name == "w2e_attn2_bwd":
        return (pk(args[11]),)
    if name in ("w2e_pack_kq", "w2e_pack_kq_h"):
        return ("transposed" if _int(args[6]) else "plain",)
    return ()


OWN = ["w2e_gemm_ex", "w2e_layernorm_fwd", "w2e_layernorm_bwd", "w2e_layernorm_bwd_add", "w2e_attn_fwd", "w2e_attn_bwd", "w2e_reduce_gelu",
       "w2e_reduce_ln_fwd", "w2e_layernorm_bwd_part", "w2e_attn2_fwd", "w2e_attn2_bwd", "w2e_attn_causal_fwd", "w2e_pack_kq", "w2e_gemm_pk",
       "w2e_pack_kq_h", "w2e_gemm_pk_h"]
# entry points of the towers that other files hold to float64 one by one: the census lists them, this file does not call them
ELSEWHERE = {"w2e_text_embed": "test_gpu_clip_text.py", "w2e_text_pool": "test_gpu_clip_text.py", "w2e_clip_logits_fwd": "test_gpu_clip.py",
             "w2e_clip_logits_bwd": "test_gpu_clip.py", "w2e_step_loss_fwd": "test_gpu_clip.py", "w2e_step_loss_bwd": "test_gpu_clip.py"}


def kcall(name, *args):
    L = _lib()
    L.call(name, *args, L.stream_ptr())
    EXERCISED.add((name, path_class(name, args)))  # (after the call: a refused call exercises nothing)


def raw(t):
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------- buffers and judging
def judge(got, ref, scale, bound, what, bufs=(), tol=None):
    """Every element within `bound` (a number or a tensor) fp32 roundings of float64, relative to ITS OWN term scale; the guards of
    `bufs` intact; tol: the global criterion beside it."""
    for b in bufs:
        assert b is None or b.intact(), f"{what}: wrote outside a buffer"
    got = got.detach().double().cpu()
    ref, scale = R.D(ref).reshape(got.shape), R.D(scale).reshape(got.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(got.shape) if torch.is_tensor(bound) else torch.full(got.shape, float(bound), dtype=torch.float64)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written (NaN left) or not finite"
    if got.numel() == 0:
        return
    assert float(got.abs().max()) < 1e-10 * SENTINEL, f"{what}: a sentinel was read"
    ratio = (got - ref).abs() / (U * scale)
    share = ratio / bound
    i = int(share.argmax())
    r, n, s = float(ratio.reshape(-1)[i]), float(bound.reshape(-1)[i]), float(share.reshape(-1)[i])
    key = what.split(" [")[0]
    if s >= WORST.get(key, (0.0, 0.0, -1.0))[2]:
        WORST[key] = (r, n, s)
    print(f"{what}: worst element {r:.3f} x 2^-24 of its term scale (bound there {n:.1f})")
    assert s <= 1.0, f"{what}: element {i} is {r:.3f} x 2^-24 of its term scale from float64 (bound {n:.1f})"
    if tol is not None:
        assert_close(got, ref, tol, what)


def padded(t, ld):
    """t [rows, cols] in a buffer of row stride ld >= cols, the gap filled with NaN (None stays None)."""
    if t is None:
        return None
    b = Buf(shape=(t.shape[0], ld))
    b.v[:, :t.shape[1]].copy_(t)
    return b


def obuf(t=None, shape=None, off=0):
    """A tensor `off` floats past a 16-byte boundary (off = 0: aligned), 4 floats of NaN slack around it inside the guards:
    (Buf, the view).  t: an input, copied in; shape: an output, NaN."""
    shape = tuple(t.shape) if t is not None else tuple(shape)
    n = math.prod(shape)
    b = Buf(shape=(n + 4,))
    v = b.v[off:off + n].view(shape)
    if t is not None:
        v.copy_(t)
    b.slack = lambda: bool(torch.isnan(b.v[:off]).all()) and bool(torch.isnan(b.v[off + n:]).all()) and b.intact()
    return b, v


def slab_buf(slabs, gap=8):
    """[S, rows, ld] -> (Buf [S, rows * ld + gap] with NaN in the gaps, the slab stride in elements)."""
    s, n = slabs.shape[0], slabs[0].numel()
    b = Buf(shape=(s, n + gap))
    b.v[:, :n].copy_(slabs.reshape(s, n))
    return b, n + gap


def packed_out(cols, m):
    """A K-quad-major output [cols / 4, mpad, 4] with 32 padded rows at least, pre-filled with PAD."""
    mpad = -(-m // 32) * 32 + 32
    return Buf(shape=(cols // 4, mpad, 4), fill=PAD), mpad


def unpacked(pb, m, what):
    """The rows < m of a packed output as [m, cols]; the padded rows must still hold PAD."""
    assert pb.intact(), f"{what}: wrote outside the packed output"
    full = pb.v.permute(1, 0, 2).reshape(pb.v.shape[1], -1)
    assert bool((full[m:] == PAD).all()), f"{what}: a padded row of the packed output was written"
    return full[:m]


def dev(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------------------------- w2e_gemm_ex
_CORES = {}


def _gemm_case(fam, m, n, k, trans_b, a_gelu=False):
    key = (fam, m, n, k, trans_b, a_gelu)
    if key not in _CORES:
        g = _gen(m, n, k, trans_b, len(fam))
        a = R.family("qgelu-wide" if a_gelu else ("plain" if fam == "qgelu-wide" else fam), g, m, k)
        w = R.family_weight(fam, g, n, k)
        b = w if trans_b else w.t().contiguous()
        bias, res = torch.randn(n, generator=g), R.family("plain", g, m, n)
        aux = R.family("qgelu-wide" if fam == "qgelu-wide" else "plain", g, m, n)
        if len(_CORES) > 16:
            _CORES.clear()
        _CORES[key] = (a, b, bias, res, aux, R.gemm_core(a, b, trans_b, a_gelu))
    return _CORES[key]


def run_gemm(a, b, trans_b, a_gelu=False, bias=None, residual=None, aux=None, c_is_zero=0, strided=False, prefill=float("nan")):
    """One w2e_gemm_ex launch.  strided: lda = k + 4, ldb = its row + 8, ldc = n + 5; residual and aux at stride ldc (what the kernel
    reads: w2e_vit.h); the input gaps hold NaN, C's gaps sentinels.  Returns (C[:, :n], the buffers whose guards must be intact)."""
    m, k = a.shape
    n = b.shape[0] if trans_b else b.shape[1]
    lda, ldb, ldc = k + (4 if strided else 0), b.shape[1] + (8 if strided else 0), n + (5 if strided else 0)
    ab, bb, bi, rb, xb = padded(a, lda), padded(b, ldb), inp(bias), padded(residual, ldc), padded(aux, ldc)
    c = Buf(shape=(m, ldc), fill=prefill)
    c.v[:, n:] = SENTINEL
    kcall("w2e_gemm_ex", P(ab.v), P(bb.v), P(c.v), m, n, k, lda, ldb, ldc, int(trans_b), int(a_gelu), ptr_of(bi), ptr_of(rb), ptr_of(xb), int(c_is_zero))
    assert bool((c.v[:, n:] == SENTINEL).all()), "the gap between C's rows was written"
    return c.v[:, :n], [c, ab, bb, bi, rb, xb]


def _epi(epi, bias, res, aux):
    return dict(bias=bias if "bias" in epi else None, residual=res if "residual" in epi else None, aux=aux if "aux" in epi else None)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("trans_b,m,n,k", [(t, *s) for t in (1, 0) for s in R.GEMM_SHAPES[t]])
def test_gemm_shapes_epilogues_and_strides(trans_b, m, n, k, fam):
    """Every shape x {none, bias, residual, aux, all} x {contiguous, lda > k & ldb > k & ldc > n}.  ldc > n pins the stride at which
    residual / gelu_grad_aux are read (ldc) and keeps the launch single-slice; the contiguous launch takes what the cost model picks."""
    a, b, bias, res, aux, core = _gemm_case(fam, m, n, k, trans_b)
    for strided in (False, True):
        sp = gemm_splits(m, n, k, n + (5 if strided else 0), False, 0)
        for epi in R.GEMM_EPILOGUES:
            kw = _epi(epi, bias, res, aux)
            got, bufs = run_gemm(a, b, trans_b, strided=strided, **kw)
            judge(got, R.gemm(core, **kw), R.gemm_scale(core, **kw), R.gemm_bound(core, k, sp, kw["aux"]),
                  f"w2e_gemm_ex trans_b {trans_b} [{m}x{n}x{k} {fam} {'+'.join(epi) or '-'} strided {strided}]", bufs, max(1e-5, 2e-6 * k ** 0.5) if fam == "plain" else None)


@pytest.mark.parametrize("m,n,k", R.GEMM_SHAPES[1])
def test_gemm_quickgelu_prologue_with_wide_arguments(m, n, k):
    """a_gelu = 1 on the [N,K] shapes, A spread over [-100, 100] with exact zeros of both signs; alone, with a wide aux, and with all."""
    a, b, bias, res, aux, core = _gemm_case("qgelu-wide", m, n, k, 1, True)
    for strided in (False, True):
        sp = gemm_splits(m, n, k, n + (5 if strided else 0), False, 0)
        for epi in ((), ("aux",), ("bias", "residual", "aux")):
            kw = _epi(epi, bias, res, aux)
            got, bufs = run_gemm(a, b, 1, a_gelu=True, strided=strided, **kw)
            judge(got, R.gemm(core, **kw), R.gemm_scale(core, **kw), R.gemm_bound(core, k, sp, kw["aux"]),
                  f"w2e_gemm_ex a_gelu [{m}x{n}x{k} {'+'.join(epi) or '-'} strided {strided}]", bufs)


GEMM_VARIANTS = [(1, 0, "-"), (1, 1, "-"), (0, 0, "-"), (0, 0, "aux"), (1, 0, "aux")]  # (trans_b, a_gelu, aux): what the towers launch, and aux on [N,K]
C0 = 0.5  # what C holds before a c_is_zero launch


@pytest.mark.parametrize("tune", R.GEMM_TUNE)
@pytest.mark.parametrize("m,n,k", R.GEMM_SPLIT_SHAPES)
def test_gemm_split_classes(m, n, k, tune, w2e_opt):
    """"tune_gemm_s" = 2, 3, 16 and the cost model (0) at K = 256 (two exact slices), 260 (a last slice 4 deep), 3072, and 132 (16
    requested: clipped to 2), bias + residual given (they belong to slice 0 alone).  With c_is_zero = 1 and C holding C0 a split
    launch returns ref + C0 and a single-slice launch ref: the test reads the class from that, holds it against the restated
    dispatch, and judges the values; with c_is_zero = 0 C starts as NaN (a split launch zero-fills it itself)."""
    if tune:
        w2e_opt("tune_gemm_s", str(tune))
    TUNE[0] = tune
    try:
        sp = gemm_splits(m, n, k, n, False, tune)
        for trans_b, a_gelu, ax in GEMM_VARIANTS:
            a, b, bias, res, aux, core = _gemm_case("qgelu-wide" if a_gelu else "clip-like", m, n, k, trans_b, bool(a_gelu))
            kw = _epi(("bias", "residual") + (("aux",) if ax == "aux" else ()), bias, res, aux)
            ref, scale, bound = R.gemm(core, **kw), R.gemm_scale(core, **kw), R.gemm_bound(core, k, sp, kw["aux"])
            what = f"w2e_gemm_ex {'split' if sp > 1 else 'single'} [{m}x{n}x{k} tune {tune} trans_b {trans_b} a_gelu {a_gelu} {ax}"
            got, bufs = run_gemm(a, b, trans_b, a_gelu=bool(a_gelu), **kw)
            judge(got, ref, scale, bound, what + " c_is_zero 0]", bufs)
            got, bufs = run_gemm(a, b, trans_b, a_gelu=bool(a_gelu), c_is_zero=1, prefill=C0, **kw)
            seen = "split" if float((got.double().cpu() - ref).median()) > C0 / 2 else "single"
            assert seen == ("split" if sp > 1 else "single"), f"{what}]: C0 shows a {seen} launch, the restated dispatch says {sp} slices"
            GEMM_CLASSES.setdefault((trans_b, a_gelu, ax), set()).add(seen)
            judge(got, ref + (C0 if sp > 1 else 0.0), scale + (C0 if sp > 1 else 0.0), bound + 1, what + " c_is_zero 1]", bufs)
    finally:
        TUNE[0] = 0


def test_gemm_split_table_is_the_host_arithmetic():
    assert [R.gemm_split(256, w) for w in (2, 3, 16)] == [(2, 128), (2, 128), (2, 128)]
    assert [R.gemm_split(260, w) for w in (2, 3, 16)] == [(2, 256), (3, 128), (3, 128)] and 260 - 2 * 128 == 4 == 260 - 256
    assert [R.gemm_split(3072, w) for w in (2, 3, 16)] == [(2, 1536), (3, 1024), (12, 256)]
    assert R.gemm_split(132, 16) == (2, 128) and R.gemm_split(128, 16) == (1, 128)
    assert R.gemm_cost_splits(70, 132, 256) == 1 and R.gemm_cost_splits(200, 768, 3072) > 1


@pytest.mark.parametrize("m,n,k", [(70, 132, 260), (200, 768, 3072)])
def test_gemm_deterministic_is_one_slice_and_bit_reproducible(m, n, k, w2e_opt):
    w2e_opt("deterministic", "1")
    w2e_opt("tune_gemm_s", "3")
    a, b, bias, res, aux, core = _gemm_case("clip-like", m, n, k, 1)
    kw = _epi(("bias", "residual"), bias, res, aux)
    got, bufs = run_gemm(a, b, 1, c_is_zero=1, prefill=C0, **kw)
    again, _ = run_gemm(a, b, 1, c_is_zero=1, prefill=C0, **kw)
    assert torch.equal(got, again), "two deterministic launches differ"
    judge(got, R.gemm(core, **kw), R.gemm_scale(core, **kw), R.gemm_bound(core, k, 1), f"w2e_gemm_ex deterministic [{m}x{n}x{k}]", bufs)


def test_gemm_refusals_leave_c_untouched():
    g = _gen(1)
    a, b, bn = inp(torch.randn(8, 16, generator=g)), inp(torch.randn(12, 16, generator=g)), inp(torch.randn(16, 12, generator=g))
    c = Buf(shape=(8, 12))
    tail = (None, None, None, 0)
    with pytest.raises(RuntimeError, match="QuickGELU prologue"):
        kcall("w2e_gemm_ex", P(a.v), P(bn.v), P(c.v), 8, 12, 16, 16, 12, 12, 0, 1, *tail)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        kcall("w2e_gemm_ex", P(a.v), P(b.v), P(c.v), 8, 12, 14, 16, 16, 12, 1, 0, *tail)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        kcall("w2e_gemm_ex", P(a.v), P(bn.v), P(c.v), 8, 10, 16, 16, 12, 10, 0, 0, *tail)
    off = P(a.buf[GUARD + 1:GUARD + 1 + 64])
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        kcall("w2e_gemm_ex", off, P(b.v), P(c.v), 4, 12, 16, 16, 16, 12, 1, 0, *tail)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        kcall("w2e_gemm_ex", P(a.v), off, P(c.v), 8, 4, 16, 16, 16, 4, 1, 0, *tail)
    kcall("w2e_gemm_ex", P(a.v), P(b.v), P(c.v), 0, 12, 16, 16, 16, 12, 1, 0, *tail)  # m = 0: returns 0, launches nothing
    assert c.untouched()
    kcall("w2e_gemm_ex", P(a.v), P(b.v), P(c.v), 8, 12, 16, 16, 16, 12, 1, 0, *tail)
    assert bool(torch.isfinite(c.v).all()), "the same buffers with the right arguments are accepted"


# ---------------------------------------------------------------------------------------------- LayerNorm
def _ln_offsets(dim):
    """(name, which tensor sits one float past a 16-byte boundary): at 512 / 768 / 1024 each sends the call to the generic kernel
    (gy and add exist in the backward only: with them the forward stays on the vector kernel)."""
    vec = [("aligned", None), ("x", "x"), ("y", "y"), ("gamma", "gamma"), ("gy", "gy"), ("add", "add")]
    return vec if dim in R.LN_VEC_DIMS else [("aligned", None), ("x", "x")]


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dim", R.LN_VEC_DIMS + R.LN_GENERIC_DIMS)
def test_layernorm_forward_and_backward(dim, fam):
    """w2e_layernorm_fwd (y, mean, rstd judged) and its input gradient through w2e_layernorm_bwd and w2e_layernorm_bwd_add (add NULL
    and given), rows 1, 4, 5, 7 (the generic kernel packs four rows per workgroup), aligned and with x, then y / gx, then gamma, then
    gy, then add one float off.  The backward takes the mean / rstd the forward saved (fp32) as its inputs, and so does its reference."""
    for rows in R.LN_ROWS:
        g = _gen(dim, rows, len(fam))
        x, gy, add = R.family(fam, g, rows, dim), R.family("plain", g, rows, dim), R.family("plain", g, rows, dim)
        gamma, beta = 1 + 0.2 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g)
        refs, scales, bounds = R.ln_fwd(x, gamma, beta, EPS), R.ln_fwd_scale(x, gamma, beta, EPS), R.ln_fwd_bound(x, EPS)
        betab = inp(beta)
        for oname, off in _ln_offsets(dim):
            (gyb, gyv), (addb, addv) = obuf(gy, off=int(off == "gy")), obuf(add, off=int(off == "add"))
            (xb, xv), (gb, gv) = obuf(x, off=int(off == "x")), obuf(gamma, off=int(off == "gamma"))
            (yb, yv), mean, rstd = obuf(shape=(rows, dim), off=int(off == "y")), Buf(shape=(rows,)), Buf(shape=(rows,))
            kcall("w2e_layernorm_fwd", P(xv), P(gv), P(betab.v), P(yv), P(mean.v), P(rstd.v), rows, dim, EPS)
            kind = path_class("w2e_layernorm_fwd", (P(xv), P(gv), P(betab.v), P(yv), 0, 0, rows, dim))[0]
            assert kind == ("vector" if dim in R.LN_VEC_DIMS and off in (None, "gy", "add") else "generic")
            what = f"[{rows}x{dim} {fam} off {oname}]"
            assert yb.slack() and xb.slack() and gb.slack(), f"{what}: wrote around y / into an input"
            for got, r, s, n, nm in zip((yv, mean.v, rstd.v), refs, scales, bounds, ("y", "mean", "rstd")):
                judge(got, r, s, n, f"w2e_layernorm_fwd {kind} {nm} {what}", (mean, rstd), 1e-5 if fam == "plain" and nm == "y" else None)
            const = [i for i in range(rows) if float(x[i].max()) == float(x[i].min())]
            assert const or not (fam == "clip-like" and rows > 2 or dim == 1)
            for i in const:  # a constant row: variance exactly 0, rstd = eps^-1/2 within rsqrtf's own error, y = beta exactly
                assert abs(float(rstd.v[i]) - EPS ** -0.5) <= (2 * R.RSQRT_ULP + 1) * U * EPS ** -0.5, (what, i, float(rstd.v[i]))
                assert torch.equal(yv[i].cpu(), beta), f"{what}: y of the constant row {i} is not beta"
            m32, r32 = mean.v.cpu(), rstd.v.cpu()
            for entry, ad in (("w2e_layernorm_bwd", None), ("w2e_layernorm_bwd_add", None), ("w2e_layernorm_bwd_add", add)):
                gxb, gxv = obuf(shape=(rows, dim), off=int(off == "y"))
                args = (P(gyv), P(xv), P(gv), P(mean.v), P(rstd.v), *(() if entry == "w2e_layernorm_bwd" else (P(addv) if ad is not None else None,)),
                        P(gxv), rows, dim)
                kcall(entry, *args)
                bkind = path_class(entry, args)[0]
                misaligned = off in ("x", "y", "gamma", "gy") or (off == "add" and ad is not None)
                assert bkind == ("vector" if dim in R.LN_VEC_DIMS and not misaligned else "generic"), (entry, oname, bkind)
                assert gxb.slack() and gyb.slack() and addb.slack(), f"{what}: wrote around gx / into an input"
                judge(gxv, R.ln_bwd(gy, x, gamma, m32, r32, ad), R.ln_bwd_scale(gy, x, gamma, m32, r32, ad), R.ln_bwd_bound(dim),
                      f"{entry} {bkind} {what[:-1]} add {ad is not None}]", (), 1e-5 if fam == "plain" else None)


def test_layernorm_refuses_dim_2049():
    x, y, s = inp(torch.zeros(2, 2049)), Buf(shape=(2, 2049)), Buf(shape=(2,))
    with pytest.raises(RuntimeError, match="unsupported"):
        kcall("w2e_layernorm_fwd", P(x.v), P(x.v), P(x.v), P(y.v), P(s.v), P(s.v), 2, 2049, EPS)
    with pytest.raises(RuntimeError, match="unsupported"):
        kcall("w2e_layernorm_bwd_add", P(x.v), P(x.v), P(x.v), P(s.v), P(s.v), None, P(y.v), 2, 2049)
    assert y.untouched() and s.untouched()


# ---------------------------------------------------------------------------------------------- attention
# (nsplit, gsplit): the loaders take 3 slabs of qkv and 6 of gout per pass
ATTN2_SPLITS = [(ns, gs) for ns in R.ATTN2_NSPLIT for gs in R.ATTN2_GSPLIT]


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("seq", R.ATTN_SEQ)
def test_attention_first_generation(seq, fam):
    """w2e_attn_fwd / w2e_attn_bwd on the packed [B, L, 3, H, 64] tensor."""
    for b, h in R.ATTN_BH:
        g = _gen(seq, b, h, len(fam))
        slabs, bias = R.family_qkv(fam, g, 1, b, seq, h)
        qkv, go = (slabs[0] + bias).reshape(b, seq, 3 * h * 64), torch.randn(b, seq, h * 64, generator=g)
        qb, gob, out, gq = inp(qkv), inp(go), Buf(shape=(b, seq, h * 64)), Buf(shape=(b, seq, 3 * h * 64))
        what = f"[L {seq} B {b} H {h} {fam}]"
        kcall("w2e_attn_fwd", P(qb.v), P(out.v), b, seq, h)
        judge(out.v, R.attn_fwd(qkv), R.attn_fwd_scale(qkv), R.attn_bound(seq), f"w2e_attn_fwd {what}", (out, qb), 1e-5 if fam == "plain" else None)
        kcall("w2e_attn_bwd", P(qb.v), P(gob.v), P(gq.v), b, seq, h)
        judge(gq.v.view(b, seq, 3, h, 64), R.attn_bwd(qkv, go), R.attn_bwd_scale(qkv, go), R.attn_bwd_bound(seq, h), f"w2e_attn_bwd {what}",
              (gq, qb, gob), 2e-5 if fam == "plain" else None)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("seq", R.ATTN_SEQ)
def test_attention_on_mfma(seq, fam):
    """w2e_attn2_fwd / _bwd: qkv as 1, 3, 4, 7 slabs and gout as 1, 6, 7, slab strides larger than the slab with NaN in the gap, bias
    NULL and given, row-major and packed: the packed tensor holds the same bits and its padded rows keep what they held."""
    for b, h in R.ATTN_BH:
        m, d = b * seq, h * 64
        for nsplit, gsplit in ATTN2_SPLITS:
            g = _gen(seq, b, h, nsplit, gsplit, len(fam))
            slabs, bias = R.family_qkv(fam, g, nsplit, b, seq, h)
            gs = torch.randn(gsplit, m, d, generator=g) / gsplit
            (sb, stride), (gsb, gstride) = slab_buf(slabs), slab_buf(gs)
            gr, gss, n_g = R.slab_sum(gs).reshape(b, seq, d), R.slab_sum_scale(gs).reshape(b, seq, d), R.slab_sum_bound(gsplit)
            for bi in (None, bias):
                bb = inp(bi)
                qr, qs = R.slab_sum(slabs, bi).reshape(b, seq, 3 * d), R.slab_sum_scale(slabs, bi).reshape(b, seq, 3 * d)
                n_in = R.slab_sum_bound(nsplit, bi is not None)
                what = f"[L {seq} B {b} H {h} {fam} slabs {nsplit}/{gsplit} bias {bi is not None}]"
                out, (outp, mpad) = Buf(shape=(m, d)), packed_out(d, m)
                kcall("w2e_attn2_fwd", P(sb.v), nsplit, stride, ptr_of(bb), P(out.v), b, seq, h, 0)
                kcall("w2e_attn2_fwd", P(sb.v), nsplit, stride, ptr_of(bb), P(outp.v), b, seq, h, mpad)
                judge(out.v, R.attn_fwd(qr), R.attn_fwd_scale(qr, qs, n_in), R.attn_bound(seq, n_in), f"w2e_attn2_fwd {what}", (out, sb, bb),
                      1e-5 if fam == "plain" else None)
                assert torch.equal(unpacked(outp, m, what), out.v), f"w2e_attn2_fwd {what}: packed and row-major differ"
                gq, (gqp, mpad) = Buf(shape=(m, 3 * d)), packed_out(3 * d, m)
                kcall("w2e_attn2_bwd", P(sb.v), nsplit, stride, ptr_of(bb), P(gsb.v), gsplit, gstride, P(gq.v), b, seq, h, 0)
                kcall("w2e_attn2_bwd", P(sb.v), nsplit, stride, ptr_of(bb), P(gsb.v), gsplit, gstride, P(gqp.v), b, seq, h, mpad)
                judge(gq.v.view(b, seq, 3, h, 64), R.attn_bwd(qr, gr), R.attn_bwd_scale(qr, gr, qs, gss, n_in, n_g), R.attn_bwd_bound(seq, h, n_in, n_g),
                      f"w2e_attn2_bwd {what}", (gq, sb, gsb, bb), 2e-5 if fam == "plain" else None)
                assert torch.equal(unpacked(gqp, m, what), gq.v), f"w2e_attn2_bwd {what}: packed and row-major differ"


def test_attention_refusals():
    qkv, out = inp(torch.zeros(2 * 65 * 192)), Buf(shape=(2 * 65 * 192,))
    for entry, args in (("w2e_attn_fwd", (P(qkv.v), P(out.v), 2, 65, 1)), ("w2e_attn_bwd", (P(qkv.v), P(qkv.v), P(out.v), 2, 65, 1)),
                        ("w2e_attn2_fwd", (P(qkv.v), 1, 4, None, P(out.v), 2, 65, 1, 0)),
                        ("w2e_attn2_bwd", (P(qkv.v), 1, 4, None, P(qkv.v), 1, 4, P(out.v), 2, 65, 1, 0))):
        with pytest.raises(RuntimeError, match="seq 65"):
            kcall(entry, *args)
    with pytest.raises(RuntimeError, match="out_packed_rows"):
        kcall("w2e_attn2_fwd", P(qkv.v), 1, 4, None, P(out.v), 2, 50, 1, 96)
    with pytest.raises(RuntimeError, match="g_packed_rows"):
        kcall("w2e_attn2_bwd", P(qkv.v), 1, 4, None, P(qkv.v), 1, 4, P(out.v), 2, 50, 1, 96)
    assert out.untouched()


@pytest.mark.parametrize("seq", [1, 33, 96])
def test_causal_attention_leaves_the_padding_alone(seq):
    """w2e_attn_causal_fwd (values: tests/test_gpu_clip_text.py): the packed output's padded rows keep what they held, the row-major
    output sits between intact sentinels, both hold the same bits, slab gaps with NaN are not read."""
    b, h = 2, 8
    m, d = b * seq, h * 64
    slabs, bias = R.family_qkv("plain", _gen(seq, 77), 2, b, seq, h)
    (sb, stride), bb = slab_buf(slabs), inp(bias)
    out, (outp, mpad) = Buf(shape=(m, d)), packed_out(d, m)
    kcall("w2e_attn_causal_fwd", P(sb.v), 2, stride, P(bb.v), P(out.v), b, seq, h, 0)
    kcall("w2e_attn_causal_fwd", P(sb.v), 2, stride, P(bb.v), P(outp.v), b, seq, h, mpad)
    assert out.intact() and bool(torch.isfinite(out.v).all())
    assert torch.equal(unpacked(outp, m, f"causal L {seq}"), out.v)
    assert_close(out.v.view(b, seq, d), R.attn_fwd(R.slab_sum(slabs, bias).reshape(b, seq, 3 * d), causal=True), 1e-5, f"causal L {seq}")


# ---------------------------------------------------------------------------------------------- the slab consumers
# (bias, residual, x_out, y, packed y): every combination w2e_reduce_ln_fwd admits -- bias x residual x {x_out and y, y alone (each
# row-major or packed), x_out alone}: 20; the one with everything given and a row-major y comes last (the backward below takes its outputs)
REDUCE_LN_COMBOS = sorted(((ub, ur, ux, uy, upk) for ub in (0, 1) for ur in (0, 1) for ux in (0, 1) for uy in (0, 1) for upk in (0, 1)
                           if (ux or uy) and (uy or not upk)), key=lambda c: c == (1, 1, 1, 1, 0))
assert len(REDUCE_LN_COMBOS) == 20 and REDUCE_LN_COMBOS[-1] == (1, 1, 1, 1, 0)


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("dim", R.REDUCE_DIMS)
def test_reduce_ln_and_layernorm_backward_of_slabs(dim, fam):
    """w2e_reduce_ln_fwd and w2e_layernorm_bwd_part: rows 1 and 33, 1 / 4 / 5 / 9 slabs (four per pass) a NaN gap apart, every NULL /
    given combination the entry points admit of bias, residual, x_out, y (row-major or packed) -- REDUCE_LN_COMBOS, 20 -- and of add,
    gx_packed -- 4; an output that was not asked for stays untouched."""
    for rows in R.REDUCE_ROWS:
        for nsplit in R.REDUCE_NSPLIT:
            g = _gen(dim, rows, nsplit, len(fam))
            part = torch.stack([R.family(fam, g, rows, dim) for _ in range(nsplit)]) / nsplit
            bias, res = torch.randn(dim, generator=g), R.family("plain", g, rows, dim)
            gamma, beta = 1 + 0.2 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g)
            (pb, stride), bb, rb, gb, btb = slab_buf(part), inp(bias), inp(res), inp(gamma), inp(beta)
            x32 = None
            for ub, ur, ux, uy, upk in REDUCE_LN_COMBOS:
                bi, rs = (bias if ub else None), (res if ur else None)
                xo, mean, rstd = Buf(shape=(rows, dim)), Buf(shape=(rows,)), Buf(shape=(rows,))
                y, mpad = packed_out(dim, rows) if upk else (Buf(shape=(rows, dim)), 0)
                kcall("w2e_reduce_ln_fwd", P(pb.v), nsplit, stride, ptr_of(bb) if ub else None, ptr_of(rb) if ur else None, P(xo.v) if ux else None,
                      P(gb.v), P(btb.v), P(y.v) if uy else None, P(mean.v), P(rstd.v), rows, dim, EPS, mpad)
                what = f"[{rows}x{dim} {fam} slabs {nsplit} bias {ub} res {ur} x {ux} y {uy} packed {upk}]"
                xr, xs, n_in = R.slab_sum(part, bi, rs), R.slab_sum_scale(part, bi, rs), R.slab_sum_bound(nsplit, ub, ur)
                if ux:
                    judge(xo.v, xr, xs, n_in, f"w2e_reduce_ln_fwd x {what}", (xo, pb, bb, rb), 1e-6 if fam == "plain" else None)
                    x32 = xo.v.cpu()  # (the last combination's -- everything given -- is what the backward below reads)
                else:
                    assert xo.untouched()
                if uy:
                    refs, scales, bounds = R.ln_fwd(xr, gamma, beta, EPS), R.ln_fwd_scale(xr, gamma, beta, EPS, xs, n_in), R.ln_fwd_bound(xr, EPS, xs, n_in)
                    yv = unpacked(y, rows, what) if upk else y.v
                    for got, r, s, n, nm in zip((yv, mean.v, rstd.v), refs, scales, bounds, ("y", "mean", "rstd")):
                        judge(got, r, s, n, f"w2e_reduce_ln_fwd {nm} {what}", (y, mean, rstd, gb, btb), 1e-5 if fam == "plain" and nm == "y" else None)
                    m32, r32 = mean.v.cpu(), rstd.v.cpu()
                else:
                    assert y.untouched() and mean.untouched() and rstd.untouched(), f"{what}: y = NULL wrote y / mean / rstd"
            # the backward of the (bias, residual) case: LN'(sum of the slabs) (+ add), from the x, mean, rstd that forward saved
            xb, mb, sb_ = inp(x32), inp(m32), inp(r32)
            gsum, gscale = R.slab_sum(part), R.slab_sum_scale(part)
            for ua, upk in ((0, 0), (1, 0), (0, 1), (1, 1)):
                gx, (gxp, mpad) = Buf(shape=(rows, dim)), packed_out(dim, rows)
                kcall("w2e_layernorm_bwd_part", P(pb.v), nsplit, stride, P(xb.v), P(gb.v), P(mb.v), P(sb_.v), P(rb.v) if ua else None, P(gx.v), rows, dim,
                      P(gxp.v) if upk else None, mpad if upk else 0)
                what = f"[{rows}x{dim} {fam} slabs {nsplit} add {ua} packed {upk}]"
                ad = res if ua else None
                judge(gx.v, R.ln_bwd(gsum, x32, gamma, m32, r32, ad), R.ln_bwd_scale(gscale, x32, gamma, m32, r32, ad), R.ln_bwd_bound(dim, nsplit),
                      f"w2e_layernorm_bwd_part {what}", (gx, pb, xb, mb, sb_), 1e-5 if fam == "plain" else None)
                if upk:
                    assert torch.equal(unpacked(gxp, rows, what), gx.v), f"{what}: packed and row-major differ"
                else:
                    assert bool((gxp.v == PAD).all()) and gxp.intact(), f"{what}: gx_packed = NULL wrote the packed buffer"


def test_slab_consumers_refuse_too_few_packed_rows():
    p, o, s = inp(torch.zeros(40, 512)), Buf(shape=(512 // 4, 32, 4)), Buf(shape=(40,))
    with pytest.raises(RuntimeError, match="y_packed_rows"):
        kcall("w2e_reduce_ln_fwd", P(p.v), 1, 40 * 512, None, None, None, P(p.v), P(p.v), P(o.v), P(s.v), P(s.v), 40, 512, EPS, 32)
    with pytest.raises(RuntimeError, match="packed_rows"):
        kcall("w2e_layernorm_bwd_part", P(p.v), 1, 40 * 512, P(p.v), P(p.v), P(s.v), P(s.v), None, P(p.v), 40, 512, P(o.v), 32)
    with pytest.raises(RuntimeError, match="packed_rows"):
        kcall("w2e_reduce_gelu", P(p.v), 1, 40 * 512, None, P(p.v), P(o.v), None, 40, 512, 1, 32)
    with pytest.raises(RuntimeError, match="unsupported"):
        kcall("w2e_reduce_ln_fwd", P(p.v), 1, 40 * 128, None, None, P(o.v), None, None, None, None, None, 40, 128, EPS, 0)
    assert o.untouched() and s.untouched()


GRID_PASS = 2048 * 256  # stream_grid (csrc/common.h): the float4s one pass of w2e_reduce_gelu's grid covers


@pytest.mark.parametrize("rows,n", [(1, 4), (33, 4), (1, 3072), (33, 3072), (683, 3072)])
def test_reduce_gelu(rows, n):
    """w2e_reduce_gelu, both modes, row-major and packed, on qgelu-wide sums and aux (exact zeros of both signs, +-100); 683 x 3072
    is 524544 float4s: the grid-stride loop runs twice (8.4 MB per slab: one slab only at that size)."""
    big = rows * n // 4 > GRID_PASS
    assert big == (rows == 683)
    for nsplit in ((1,) if big else R.REDUCE_NSPLIT):
        g = _gen(rows, n, nsplit)
        part = torch.stack([R.family("qgelu-wide", g, rows, n) for _ in range(nsplit)]) / nsplit
        bias, aux = torch.randn(n, generator=g), R.family("qgelu-wide", g, rows, n)
        (pb, stride), bb, ab = slab_buf(part), inp(bias), inp(aux)
        (hr, gr), (hs, gs) = R.reduce_gelu(part, bias), R.reduce_gelu_scale(part, bias)
        nh, ng = R.reduce_gelu_bound(nsplit, hr)
        r1, s1, n1 = R.reduce_gelu(part, aux=aux, mode=1), R.reduce_gelu_scale(part, aux=aux, mode=1), R.reduce_gelu_bound(nsplit, aux=aux, mode=1)
        what = f"[{rows}x{n} slabs {nsplit}]"
        h, act = Buf(shape=(rows, n)), Buf(shape=(rows, n))
        kcall("w2e_reduce_gelu", P(pb.v), nsplit, stride, P(bb.v), None, P(h.v), P(act.v), rows, n, 0, 0)
        judge(h.v, hr, hs, nh, f"w2e_reduce_gelu mode 0 h {what}", (h, pb, bb))
        judge(act.v, gr, gs, ng, f"w2e_reduce_gelu mode 0 g {what}", (act,))
        h2, (actp, mpad) = Buf(shape=(rows, n)), packed_out(n, rows)
        kcall("w2e_reduce_gelu", P(pb.v), nsplit, stride, P(bb.v), None, P(h2.v), P(actp.v), rows, n, 0, mpad)
        assert torch.equal(h2.v, h.v) and h2.intact() and torch.equal(unpacked(actp, rows, what), act.v), f"mode 0 packed {what}"
        out, unused = Buf(shape=(rows, n)), Buf(shape=(rows, n))
        kcall("w2e_reduce_gelu", P(pb.v), nsplit, stride, None, P(ab.v), P(out.v), P(unused.v), rows, n, 1, 0)
        judge(out.v, r1, s1, n1, f"w2e_reduce_gelu mode 1 {what}", (out, pb, ab))
        assert unused.untouched(), f"{what}: mode 1 wrote g"
        outp, mpad = packed_out(n, rows)
        kcall("w2e_reduce_gelu", P(pb.v), nsplit, stride, None, P(ab.v), P(outp.v), None, rows, n, 1, mpad)
        assert torch.equal(unpacked(outp, rows, what), out.v), f"mode 1 packed {what}"
        assert int((aux == 0).sum()) >= 2 or n == 4


# ---------------------------------------------------------------------------------------------- packings and the register-fed GEMMs
def _pack(x, rows_padded, transposed=False, half=False, gap=4):
    """w2e_pack_kq / w2e_pack_kq_h of X [rows, K] given row-major with ldx = K + gap (NaN in the gap), or, transposed, as X^T [K, rows]
    with ldx = rows + gap.  Returns the pack as a GPU tensor that sat between sentinels (checked)."""
    rows, k = x.shape
    src = padded(x.t().contiguous() if transposed else x, (rows if transposed else k) + gap)
    if half:
        n = (k // 8) * rows_padded * 8
        buf = torch.full((GUARD + n + GUARD,), 3e4, device=DEV, dtype=torch.float16)
        out = buf[GUARD:GUARD + n].view(k // 8, rows_padded, 8)
        out.fill_(float("nan"))
        kcall("w2e_pack_kq_h", P(src.v), raw(out), rows, rows_padded, k, src.v.shape[1], int(transposed))
        assert bool((buf[:GUARD] == 3e4).all()) and bool((buf[GUARD + n:] == 3e4).all()), "w2e_pack_kq_h wrote outside its output"
        return out
    pb = Buf(shape=(k // 4, rows_padded, 4))
    kcall("w2e_pack_kq", P(src.v), P(pb.v), rows, rows_padded, k, src.v.shape[1], int(transposed))
    assert pb.intact() and src.intact(), "w2e_pack_kq wrote outside its output"
    return pb.v


@pytest.mark.parametrize("m,n,k", R.PK_SHAPES)
def test_gemm_pk_with_the_padding_production_leaves(m, n, k):
    """w2e_pack_kq (plain and transposed, ldx larger than the row, padded rows zero, bit-exact against vit_ref.kq_pack) and w2e_gemm_pk
    at every admissible split count (the one w2e_gemm_pk_splits returns is one of them), ldc = n and ldc > n (sentinels in the gap).  Then
    the operands as production builds them: _block_fwd allocates every packed A with torch.empty and its producers write the rows < m
    only -- the padded rows of A and the padded columns of the weight pack hold NaN here: the slabs must equal the clean-padding
    result bit for bit and hold no NaN (MFMA rows and columns are independent)."""
    g = _gen(m, n, k, 8)
    a, w = R.family("clip-like", g, m, k), R.family_weight("clip-like", g, n, k)
    mpad, npad = -(-m // 32) * 32, -(-n // 64) * 64
    ap, wp, wpt = _pack(a, mpad), _pack(w, npad), _pack(w, npad, transposed=True)
    assert torch.equal(ap.cpu(), R.kq_pack(a, mpad)) and torch.equal(wp.cpu(), R.kq_pack(w, npad)), "w2e_pack_kq is not vit_ref.kq_pack"
    assert torch.equal(wpt, wp), "the transposed packing gives another operand"
    a_nan, w_nan = ap.clone(), wp.clone()
    a_nan[:, m:], w_nan[:, n:] = float("nan"), float("nan")
    core = R.gemm_core(a, w, True)
    pick = _lib().load().w2e_gemm_pk_splits(m, n, k)
    tried = 0
    for sp in range(1, k // 8 + 1):
        if not R.pk_split(k, sp)[1]:
            continue
        tried += 1
        slabs = {}
        for tag, (aa, ww, ldc) in {"clean": (ap, wp, n), "nan padding": (a_nan, w_nan, n), "ldc": (ap, wp, n + 5)}.items():
            c = Buf(shape=(sp, m, ldc))
            c.v[:, :, n:] = SENTINEL
            kcall("w2e_gemm_pk", P(aa), P(ww), P(c.v), m, n, k, mpad, npad, ldc, sp)
            assert c.intact() and bool((c.v[:, :, n:] == SENTINEL).all()), f"w2e_gemm_pk wrote between the rows of a slab ({tag})"
            slabs[tag] = c.v[:, :, :n]
        judge(slabs["clean"].double().sum(0), core[0], core[1] + R.TINY, R.gemm_pk_bound(k, sp), f"w2e_gemm_pk [{m}x{n}x{k} {sp} slabs]")
        assert bool(torch.isfinite(slabs["nan padding"]).all()), f"{sp} slabs: NaN from the padding reached a stored element"
        assert torch.equal(slabs["nan padding"], slabs["clean"]), f"{sp} slabs: the padding's contents changed stored elements"
        assert torch.equal(slabs["ldc"], slabs["clean"]), f"{sp} slabs: ldc > n changed the values"
    assert tried >= 1 and R.pk_split(k, pick)[1]
    if k >= 16:
        with pytest.raises(RuntimeError, match="empty slice|splits of"):
            kcall("w2e_gemm_pk", P(ap), P(wp), P(Buf(shape=(1,)).v), m, n, k, mpad, npad, n, k // 8 + 1)


@pytest.mark.parametrize("m,n,k", [(77, 200, kk) for kk in R.PK_H_K] + [(33, 65, 48)])
def test_gemm_pk_h_with_the_padding_production_leaves(m, n, k):
    """The fp16 form: w2e_pack_kq_h is vit_ref.kq_pack_h bit for bit (plain and transposed), w2e_gemm_pk_h against the float64 product of
    the operands rounded to fp16, every admissible split count, NaN in the padding of both operands."""
    g = _gen(m, n, k, 16)
    a, w = R.family("clip-like", g, m, k), R.family_weight("clip-like", g, n, k) * k ** -0.5
    mpad, npad = -(-m // 32) * 32, -(-n // 64) * 64
    ap, wh, wht = _pack(a, mpad), _pack(w, npad, half=True), _pack(w, npad, transposed=True, half=True)
    assert torch.equal(wh.cpu(), R.kq_pack_h(w, npad)), "w2e_pack_kq_h is not vit_ref.kq_pack_h"
    assert torch.equal(wht, wh), "the transposed fp16 packing gives another operand"
    a_nan, w_nan = ap.clone(), wh.clone()
    a_nan[:, m:], w_nan[:, n:] = float("nan"), float("nan")
    core = R.gemm_core(a.half(), w.half(), True)
    pick = _lib().load().w2e_gemm_pk_h_splits(m, n, k)
    tried = 0
    for sp in range(1, k // 16 + 1):
        if not R.pk_split(k, sp, 16)[1]:
            continue
        tried += 1
        slabs = {}
        for tag, (aa, ww, ldc) in {"clean": (ap, wh, n), "nan padding": (a_nan, w_nan, n), "ldc": (ap, wh, n + 5)}.items():
            c = Buf(shape=(sp, m, ldc))
            c.v[:, :, n:] = SENTINEL
            kcall("w2e_gemm_pk_h", P(aa), raw(ww), P(c.v), m, n, k, mpad, npad, ldc, sp)
            assert c.intact() and bool((c.v[:, :, n:] == SENTINEL).all()), f"w2e_gemm_pk_h wrote between the rows of a slab ({tag})"
            slabs[tag] = c.v[:, :, :n]
        judge(slabs["clean"].double().sum(0), core[0], core[1] + R.TINY, R.gemm_pk_bound(k, sp, 16), f"w2e_gemm_pk_h [{m}x{n}x{k} {sp} slabs]")
        assert bool(torch.isfinite(slabs["nan padding"]).all()), f"{sp} slabs: NaN from the padding reached a stored element"
        assert torch.equal(slabs["nan padding"], slabs["clean"]) and torch.equal(slabs["ldc"], slabs["clean"])
    assert tried >= 1 and R.pk_split(k, pick, 16)[1]


# ---------------------------------------------------------------------------------------------- the census
def test_path_class_reads_the_arguments_the_wrappers_pass():
    x = torch.zeros(64, device=DEV)
    p, q, null = P(x), P(x[1:]), None
    assert path_class("w2e_gemm_ex", (p, p, p, 200, 768, 3072, 3072, 3072, 768, 1, 1, p, p, null, 1)) == (1, 1, "-", "split", 1)
    assert path_class("w2e_gemm_ex", (p, p, p, 200, 768, 3072, 3072, 768, 773, 0, 0, null, null, p, 0)) == (0, 0, "aux", "single", 0)
    assert path_class("w2e_layernorm_fwd", (p, p, p, p, p, p, 5, 768, EPS)) == ("vector",)
    assert path_class("w2e_layernorm_fwd", (p, p, p, q, p, p, 5, 768, EPS)) == ("generic",) == path_class("w2e_layernorm_fwd", (p, p, p, p, p, p, 5, 128, EPS))
    assert path_class("w2e_layernorm_bwd", (p, p, p, p, p, p, 5, 512)) == ("vector", "-")
    assert path_class("w2e_layernorm_bwd_add", (p, p, p, p, p, q, p, 5, 512)) == ("generic", "add")
    assert path_class("w2e_reduce_ln_fwd", (p, 1, 4, null, null, p, null, null, null, null, null, 5, 512, EPS, 0)) == ("no y",)
    assert path_class("w2e_reduce_ln_fwd", (p, 1, 4, null, null, p, p, p, p, p, p, 5, 512, EPS, 32)) == ("packed",)
    assert path_class("w2e_layernorm_bwd_part", (p, 1, 4, p, p, p, p, null, p, 5, 512, p, 32)) == ("packed",)
    assert path_class("w2e_reduce_gelu", (p, 1, 4, null, p, p, null, 5, 512, 1, 32)) == (1, "packed")
    assert path_class("w2e_attn2_bwd", (p, 1, 4, p, p, 1, 4, p, 1, 50, 12, 0)) == ("row-major",)
    assert path_class("w2e_pack_kq", (p, p, 5, 32, 8, 8, 1)) == ("transposed",)


def test_census_of_the_paths_the_towers_take(monkeypatch):
    """One forward + backward of (a) the tiny tower (width 128: the first-generation path), (b) a one-layer 768-wide tower at batch 1 and
    4, fp32 and set_precision("f16"), (c) one forward of a one-layer 512-wide text tower at L = 77, (d) the loss tail (clip_logits,
    step_loss), with every call of the library -- through where2edit_amd._lib.call and through the name vit_hip bound at import --
    recorded as (entry point, path class).  Every recorded pair of an entry point this file tests must have been exercised by its
    tests (checked by the last test when the whole file ran); the rest of what the towers call is listed with the file that tests it."""
    import sys

    import seeded
    import test_gpu_clip as TC
    import test_gpu_clip_text as TT
    from make_golden import CLIP_TINY
    from where2edit_amd import vit_hip as V
    L = _lib()
    real_call = L.call

    def recording(name, *args):
        key = (name, path_class(name, args))
        CENSUS[key] = CENSUS.get(key, 0) + 1
        return real_call(name, *args)

    assert V.call is real_call
    monkeypatch.setattr(L, "call", recording)
    for mod in list(sys.modules.values()):
        if getattr(mod, "__name__", "").startswith("where2edit_amd") and getattr(mod, "call", None) is real_call:
            monkeypatch.setattr(mod, "call", recording)
    assert V.call is recording

    def image_pass(model, batch, key):
        img = seeded.tensor(key, (batch, 3, 224, 224), 0.5).to(DEV).requires_grad_(True)
        f = model.encode_image(img)
        torch.autograd.grad((f * seeded.tensor(key + ".r", tuple(f.shape)).to(DEV)).sum(), img)
        return f

    tiny, _ = TC._model(CLIP_TINY)
    image_pass(tiny, 3, "census.tiny")
    cfg = dict(embed_dim=512, image_resolution=224, vision_layers=1, vision_width=768, vision_patch=32, context_length=8, vocab_size=64,
               text_width=64, text_layers=1)
    wide, _ = TC._model(cfg)
    for batch in (1, 4):
        image_pass(wide, batch, f"census.wide{batch}")
        wide.set_precision("f16")
        try:
            feat = image_pass(wide, batch, f"census.wide{batch}")
        finally:
            wide.set_precision("f32")
    text, _ = TT._clip(layers=1, vocab=1000)
    tf = text.encode_text(TT._tokens(2, vocab=1000).to(DEV))
    assert tf.shape == (2, 512)
    fd = feat.detach().requires_grad_(True)
    sim = V.clip_logits(fd, tf, torch.tensor(2.6593, device=DEV), similarity=True)
    w = seeded.tensor("census.w", (4, 18, 512)).to(DEV)
    loss, _, _ = V.step_loss(sim, (w + 0.1).requires_grad_(True), w, 1.0, 0.8)
    loss.backward()
    torch.cuda.synchronize()
    for key in sorted(CENSUS, key=str):
        where = "" if key[0] in OWN else f"   (tested in {ELSEWHERE.get(key[0], 'another file')})"
        print(f"census: {CENSUS[key]:4d} x {key[0]} {key[1]}{where}")
    unseen = [n for n in OWN if not any(k[0] == n for k in CENSUS)]
    assert CENSUS and not unseen, f"entry points the census never saw (do the calls still go through vit_hip.call?): {unseen}"


def test_zz_census_pairs_were_exercised_and_worst_ratios(request):
    """After the tests above (file order): both GEMM classes occurred for every variant, every (entry point, path class) the census
    recorded for an entry point of this file was called with that class by this file's tests -- checked when the whole file ran --
    and the table of worst measured ratios (DESIGN.md quotes it).  A pair only the tests reach is listed and does not fail."""
    for key in sorted(WORST):
        r, n, s = WORST[key]
        print(f"worst: {r:10.3f} of {n:10.1f} ({100 * s:5.1f} % of the bound)  {key}")
    whole_file = not request.config.getoption("keyword") and not any("::" in a for a in request.config.args)
    if whole_file:
        for v in GEMM_VARIANTS:
            assert GEMM_CLASSES.get(v) == {"split", "single"}, f"w2e_gemm_ex {v}: only {GEMM_CLASSES.get(v)} occurred"
        missing = sorted((k for k in CENSUS if k[0] in OWN and k not in EXERCISED), key=str)
        assert not missing, f"paths the towers take that no test of this file exercised: {missing}"
        for key in sorted((k for k in EXERCISED if k not in CENSUS), key=str):
            print(f"tests only: {key[0]} {key[1]}")
