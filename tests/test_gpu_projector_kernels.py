"""Every entry point of include/w2e_projector.h (csrc/projector.hip) on its own, through the C ABI, against the float64 restatement of
tests/projector_ref.py (held to autograd by tests/test_projector_ref_host.py).

How the error is judged: the error-bound form of `judge` in tests/test_gpu_gen_small_kernels.py.  Every ELEMENT against its own term
scale -- the formula on absolute values, never the cancelled result --: |got - ref| <= N * 2^-24 * scale, N = the dependent fp32
roundings on the longest chain the kernel uses for that output, derived beside each test from the reduction that was built.  Outputs are
pre-filled with NaN and sit between sentinels that must survive; inputs must come back unchanged; two runs must agree bit for bit."""
import ctypes
import math

import pytest
import torch

import projector_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SENTINEL = 1e30
GUARD = 64


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A kernel fault surfaces at the next synchronisation: end the session there instead of launching more work on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error after this test, nothing more is launched: {e}", returncode=3)


def L():
    from where2edit_amd import _lib
    return _lib


def kcall(name, *args):
    L().call(name, *args, L().stream_ptr())


def P(t):
    return None if t is None else L().ptr(t)


def pointers(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.v.data_ptr() for b in bufs])


def ints(v):
    return (ctypes.c_int * len(v))(*v)


def reg_workspace(batch, size):
    """w2e_noise_reg_workspace: the floats of the regulariser's workspace (a refusal raises)."""
    floats = ctypes.c_int64(-1)
    L().call("w2e_noise_reg_workspace", len(batch), ints(batch), ints(size), ctypes.byref(floats))
    return floats.value


class Buf:
    """A tensor on the GPU between two runs of GUARD sentinels.  Buf(t): a copy of the CPU tensor t; Buf(shape=...): pre-filled (NaN)."""

    def __init__(self, t=None, shape=None, fill=float("nan"), dtype=torch.float32):
        shape = tuple(t.shape) if t is not None else tuple(shape)
        n = math.prod(shape)
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, device=DEV, dtype=dtype)
        self.v = self.buf[GUARD:GUARD + n].view(shape)
        self.v.copy_(t) if t is not None else self.v.fill_(fill)
        self.n = n
        self.src = t.clone().to(dtype) if t is not None else None

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def unchanged(self):
        return self.intact() and torch.equal(self.v.cpu(), self.src)


def judge(out, ref, scale, what, bound):
    """Every element within `bound` fp32 roundings of float64, relative to ITS OWN term scale; the guards intact."""
    assert out.intact(), f"{what}: wrote outside the output"
    got = out.v.detach().double().cpu()
    ref, scale = ref.reshape(got.shape).double(), scale.reshape(got.shape).double()
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written (NaN left) or not finite"
    ratio = (got - ref).abs() / (U * scale).clamp_min(1e-300)
    worst = float(ratio.max())
    print(f"{what}: worst element {worst:.3f} x 2^-24 of its term scale (bound {bound})")
    assert worst <= bound, f"{what}: element {int(ratio.argmax())} is {worst:.3f} x 2^-24 of its term scale from float64 (bound {bound})"


def gen(*key):
    return torch.Generator().manual_seed(7000 + sum((i + 1) * int(k) for i, k in enumerate(key)))


def white(shape, *key):
    return torch.randn(shape, generator=gen(*key))


def smooth(shape, *key):
    """Correlated: white noise box-filtered twice along both axes (wrapping), unit variance."""
    n = white(shape, *key)
    for _ in range(2):
        n = n + torch.roll(n, 1, 2) + torch.roll(n, 1, 3) + torch.roll(n, (1, 1), (2, 3))
    return n / n.std()


# ---------------------------------------------------------------------------------------------- w2e_noise_grad
def slices(planes, pixels):
    """noise_grad_slices of csrc/projector.hip, restated: interleaved plane slices until 65536 threads or no more planes to split."""
    groups = pixels // 4 if pixels % 4 == 0 else pixels
    s = 1
    while s < 64 and 2 * s <= planes and groups * s < 65536:
        s *= 2
    return s


NOISE_GRAD_CASES = [(planes, pixels) for planes in (1, 3, 33, 512) for pixels in (16, 64, 1024)] + [(32, 256 * 256), (33, 25), (5, 4099)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("planes,pixels", NOISE_GRAD_CASES, ids=str)
def test_noise_grad(planes, pixels, accumulate):
    """g_noise (+)= noise_w * sum over planes.  Roundings of an element: a slice adds ceil(planes / S) values (the first onto 0: exact),
    the S slices are added in order (S - 1), the product with noise_w (1), the addition onto the old value when accumulating (1):
    ceil(planes / S) + S.  (33, 25) and (5, 4099): the one-pixel-per-thread form; (32, 256^2): one slice, 256 blocks."""
    S = slices(planes, pixels)
    assert L().load().w2e_noise_grad_slices(planes, pixels) == S
    assert {slices(*c) for c in NOISE_GRAD_CASES} >= {1, 2, 32, 64}
    gpre, nw, old = white((planes, pixels), planes, pixels), torch.tensor([-0.37]), white((pixels,), planes, pixels, 1)
    gb, nwb = Buf(gpre), Buf(nw)
    ref, scale = R.noise_grad(gpre.double(), float(nw.double()))
    if accumulate:
        ref, scale = ref + old.double(), scale + old.double().abs()
    runs = []
    for _ in range(2):
        out = Buf(old) if accumulate else Buf(shape=(pixels,))
        kcall("w2e_noise_grad", P(gb.v), P(nwb.v), P(out.v), planes, pixels, accumulate)
        judge(out, ref, scale, f"w2e_noise_grad [{planes} x {pixels}, S {S}, acc {accumulate}]", -(-planes // S) + S)
        runs.append(out.v.clone())
    assert torch.equal(runs[0], runs[1])
    assert gb.unchanged() and nwb.unchanged()


def test_noise_grad_refusals():
    x = torch.zeros(16, device=DEV)
    for args in [(None, P(x), P(x), 1, 16, 0), (P(x), None, P(x), 1, 16, 0), (P(x), P(x), None, 1, 16, 0), (P(x), P(x), P(x), 0, 16, 0),
                 (P(x), P(x), P(x), 1, 0, 0)]:
        with pytest.raises(RuntimeError, match="noise_grad"):
            kcall("w2e_noise_grad", *args)


# ---------------------------------------------------------------------------------------------- regulariser and normaliser: the lists
def _list(shapes, kind, key):
    make = white if kind == "white" else smooth
    return [make(s, key, i) for i, s in enumerate(shapes)]


GEN64 = [(1, 1, 4, 4)] + [(1, 1, 2 ** i, 2 ** i) for i in range(3, 7) for _ in range(2)]  # Generator(64).make_noise()
LISTS = {
    "4": [(1, 1, 4, 4)], "8": [(1, 1, 8, 8)], "16": [(1, 1, 16, 16)], "2x32": [(2, 1, 32, 32)], "256": [(1, 1, 256, 256)],
    "gen64": GEN64, "65x8": [(1, 1, 8, 8)] * 65,
}
assert len(GEN64) == 9


@pytest.mark.parametrize("kind", ["white", "smooth"])
@pytest.mark.parametrize("name", list(LISTS), ids=str)
def test_noise_regularize(name, kind):
    """Value and gradient of the whole list in one call each.  What rounds in fp32: a pooled value ((a + b) + (c + d)) * 0.25 carries two
    roundings per pyramid step, so 2 j at level j, a product of two of them 4 j; the products and their sums run in double (nothing at
    this scale), as do the means and the squares.
      value: 4 (levels - 1) for the coarsest level's products + the final double -> float: 4 (levels - 1) + 1; held to + 4.
      gradient, the term of level j: the mean 4 j and its coefficient's rounding 1; the two neighbours 2 j and their sum 1; the product 1;
        the sum of the two products 2; adding a quarter of the coarser gradient 1; then one more rounding at each of the j finer levels it
        is handed down through: 7 j + 6 <= 7 (levels - 1) + 6.
    Scales (projector_ref.noise_regularize_scales): the same sums on |n|, with the mean of |products| in place of the cancelled mean."""
    shapes = LISTS[name]
    maps = _list(shapes, kind, len(shapes))
    levels = max(len(R.levels(m)) for m in maps)
    gout = torch.tensor([1e5])
    dbl = [m.double().requires_grad_(True) for m in maps]
    ref = R.noise_regularize(dbl)
    ref_grads = torch.autograd.grad(ref, dbl)
    scales = [R.noise_regularize_scales(m.double()) for m in maps]
    bufs, gb = [Buf(m) for m in maps], Buf(gout)
    batch, size = ints([s[0] for s in shapes]), ints([s[2] for s in shapes])
    floats = reg_workspace([s[0] for s in shapes], [s[2] for s in shapes])
    assert floats > 0
    runs = []
    for _ in range(2):
        ws, loss, grads = Buf(shape=(floats,)), Buf(shape=(1,)), [Buf(shape=s) for s in shapes]
        assert ws.v.data_ptr() % 8 == 0
        kcall("w2e_noise_reg_fwd", len(maps), pointers(bufs), batch, size, P(ws.v), floats, P(loss.v))
        judge(loss, ref.detach(), sum(s[0] for s in scales), f"w2e_noise_reg_fwd [{name} {kind}]", 4 * (levels - 1) + 4)
        kcall("w2e_noise_reg_bwd", len(maps), pointers(bufs), batch, size, P(ws.v), floats, P(gb.v), pointers(grads), 0)
        for i, (g, rg, sc) in enumerate(zip(grads, ref_grads, scales)):
            judge(g, rg * 1e5, sc[1] * 1e5, f"w2e_noise_reg_bwd [{name} {kind} map {i}]", 7 * (levels - 1) + 6)
        assert ws.intact()
        runs.append([loss.v.clone()] + [g.v.clone() for g in grads])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # accumulate: added onto what the gradients hold (one more rounding)
    first = Buf(maps[0] * 1e-3)
    others = [Buf(shape=s, fill=0.0) for s in shapes[1:]]
    kcall("w2e_noise_reg_bwd", len(maps), pointers(bufs), batch, size, P(ws.v), floats, P(gb.v), pointers([first] + others), 1)
    judge(first, ref_grads[0] * 1e5 + maps[0].double() * 1e-3, scales[0][1] * 1e5 + maps[0].double().abs() * 1e-3,
          f"w2e_noise_reg_bwd accumulate [{name} {kind}]", 7 * (levels - 1) + 7)
    assert all(b.unchanged() for b in bufs) and gb.unchanged()


def test_noise_regularize_white_against_smooth_and_refusals():
    """The cancellation case end to end: a white 256^2 map's value is within a few 1 / N of 0 and still right to the bound above (that
    test); here that the kernel's value orders the two kinds as the reference does, and what is refused."""
    vals = {}
    for kind in ("white", "smooth"):
        m = Buf(_list([(1, 1, 256, 256)], kind, 1)[0])
        batch, size = ints([1]), ints([256])
        floats = reg_workspace([1], [256])
        ws, loss = torch.empty(floats, device=DEV), torch.empty(1, device=DEV)
        kcall("w2e_noise_reg_fwd", 1, pointers([m]), batch, size, P(ws), floats, P(loss))
        vals[kind] = float(loss)
    assert vals["white"] < 1.7 and vals["smooth"] > 0.25 and vals["smooth"] > 20 * vals["white"]
    for batch, size in (([1], [24]), ([0], [8])):  # no power of two; an empty batch
        with pytest.raises(RuntimeError, match="noise_reg_workspace"):
            reg_workspace(batch, size)
    x, one = torch.zeros(64, device=DEV), torch.zeros(1, device=DEV)
    small_ws = torch.empty(8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        kcall("w2e_noise_reg_fwd", 1, (ctypes.c_void_p * 1)(x.data_ptr()), ints([1]), ints([8]), P(small_ws), 8, P(one))
    with pytest.raises(RuntimeError, match="power-of-two"):
        kcall("w2e_noise_reg_fwd", 1, (ctypes.c_void_p * 1)(x.data_ptr()), ints([1]), ints([6]), P(small_ws), 8, P(one))


@pytest.mark.parametrize("kind", ["white", "smooth"])
@pytest.mark.parametrize("name", list(LISTS), ids=str)
def test_noise_normalize(name, kind):
    """n <- (n - mean) / std (unbiased) in place.  The moments are summed in double and every element is formed in double and rounded
    once: 1 rounding of |n - mean| / std; held to 2.  Then, in float64, of the fp32 result y: |mean(y)| <= 2^-24 mean|y| (every element's
    one rounding, all the same way at worst) and |std(y) - 1| <= 2 * 2^-24 * rms(y) / std(y) (the same perturbation of the norm)."""
    shapes = LISTS[name]
    maps = [m * (1.5 + i) + (0.5 - 0.25 * i) for i, m in enumerate(_list(shapes, kind, 50 + len(shapes)))]
    bufs = [Buf(m) for m in maps]
    numel = (ctypes.c_int64 * len(maps))(*[m.numel() for m in maps])
    floats = len(maps) * L().CONSTS["W2E_PROJ_SLOTS"] * 4
    ws = Buf(shape=(floats,))
    kcall("w2e_noise_normalize", len(maps), pointers(bufs), numel, P(ws.v), floats)
    assert ws.intact()
    for i, (b, m) in enumerate(zip(bufs, maps)):
        d = m.double()
        judge(b, R.noise_normalize(d), (d.abs() + d.mean().abs()) / d.std(), f"w2e_noise_normalize [{name} {kind} map {i}]", 2)
        y = b.v.double().cpu()
        assert abs(float(y.mean())) <= U * float(y.abs().mean()), (name, i, float(y.mean()))
        assert abs(float(y.std()) - 1) <= 2 * U * float(y.pow(2).mean().sqrt() / y.std()), (name, i, float(y.std()))
    again = [Buf(m) for m in maps]
    kcall("w2e_noise_normalize", len(maps), pointers(again), numel, P(ws.v), floats)
    assert all(torch.equal(a.v, b.v) for a, b in zip(again, bufs))


def test_noise_normalize_refusals():
    x, ws = torch.ones(4, device=DEV), torch.empty(256, device=DEV)
    with pytest.raises(RuntimeError, match="elements"):
        kcall("w2e_noise_normalize", 1, (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int64 * 1)(1), P(ws), 256)
    with pytest.raises(RuntimeError, match="workspace"):
        kcall("w2e_noise_normalize", 1, (ctypes.c_void_p * 1)(x.data_ptr()), (ctypes.c_int64 * 1)(4), P(ws), 255)
    assert torch.equal(x.cpu(), torch.ones(4))


# ---------------------------------------------------------------------------------------------- loss front
FRONT_CASES = [(1, 16, 1), (3, 16, 2), (1, 32, 2), (3, 32, 4), (1, 64, 4), (3, 64, 1), (1, 48, 3)]


@pytest.mark.parametrize("mse", [0.0, 0.7])
@pytest.mark.parametrize("batch,size,f", FRONT_CASES, ids=str)
def test_loss_front(batch, size, f, mse):
    """Forward: a box is summed in row order from 0 (f^2 - 1 roundings) and multiplied (1) by the fp32 1 / f^2 (itself rounded when f is
    no power of two: 1): f^2 + 1, relative to the box mean of |img|.  The partial sums: the squared differences of the kernel's OWN fp32 `small` in double, so their total is the float64 mean
    squared error of that tensor to ~1e-15.  Adjoint: coef * g_mse (1), small - target (1), their product (1), + g_small (1), times the fp32 1 / f^2 (2, as
    above): 6, relative to (|g_small| + |c| (|small| + |target|)) / f^2."""
    s = size // f
    img, target, g_small = white((batch, 3, size, size), batch, size, f), white((batch, 3, s, s), batch, size, f, 1), white((batch, 3, s, s), batch, size, f, 2)
    g_mse = torch.tensor([mse * 1.3])
    ref_small, _ = R.front(img.double(), target.double(), f)
    scale_small, _ = R.front(img.double().abs(), target.double(), f)
    ib, tb, small = Buf(img), Buf(target), Buf(shape=(batch, 3, s, s))
    blocks = L().load().w2e_proj_front_blocks(small.n)
    assert 1 <= blocks <= L().CONSTS["W2E_PROJ_FRONT_PARTIALS"] and blocks == min(1024, -(-small.n // 1024))
    partials = Buf(shape=(blocks,), dtype=torch.float64)
    kcall("w2e_proj_front_fwd", P(ib.v), P(tb.v), batch, 3, size, size, f, P(small.v), ctypes.c_void_p(partials.v.data_ptr()))
    judge(small, ref_small, scale_small, f"w2e_proj_front_fwd small [{batch} {size} f{f}]", f * f + 1)
    assert partials.intact() and bool(torch.isfinite(partials.v).all())
    own = (small.v.double().cpu() - target.double()).pow(2).sum()
    assert abs(float(partials.v.sum()) - float(own)) <= 1e-13 * float(own)
    # without a target: the same small, no partial sums
    small2 = Buf(shape=(batch, 3, s, s))
    kcall("w2e_proj_front_fwd", P(ib.v), None, batch, 3, size, size, f, P(small2.v), None)
    assert torch.equal(small2.v, small.v) and small2.intact()
    # the adjoint, on the kernel's own small
    sm = small.v.double().cpu()
    c = 2.0 / small.n * float(g_mse.double())
    gsb, gmb, g_img = Buf(g_small), Buf(g_mse), Buf(shape=(batch, 3, size, size))
    up = lambda t: t.repeat_interleave(f, 2).repeat_interleave(f, 3)  # noqa: E731
    if mse:
        kcall("w2e_proj_front_bwd", P(gsb.v), P(small.v), P(tb.v), P(gmb.v), 2.0 / small.n, batch, 3, size, size, f, P(g_img.v))
        ref = up(g_small.double() + c * (sm - target.double())) / (f * f)
        scale = up(g_small.double().abs() + abs(c) * (sm.abs() + target.double().abs())) / (f * f)
        judge(g_img, ref, scale, f"w2e_proj_front_bwd [{batch} {size} f{f} mse]", 6)
        only = Buf(shape=(batch, 3, size, size))
        kcall("w2e_proj_front_bwd", None, P(small.v), P(tb.v), P(gmb.v), 2.0 / small.n, batch, 3, size, size, f, P(only.v))
        judge(only, up(c * (sm - target.double())) / (f * f), up(abs(c) * (sm.abs() + target.double().abs())) / (f * f),
              f"w2e_proj_front_bwd [{batch} {size} f{f} mse only]", 5)
    else:
        kcall("w2e_proj_front_bwd", P(gsb.v), None, None, None, 0.0, batch, 3, size, size, f, P(g_img.v))
        judge(g_img, up(g_small.double()) / (f * f), up(g_small.double().abs()) / (f * f), f"w2e_proj_front_bwd [{batch} {size} f{f}]", 2)
    assert ib.unchanged() and tb.unchanged() and gsb.unchanged()


def test_loss_front_refusals():
    x = torch.zeros(3 * 16 * 16, device=DEV)
    with pytest.raises(RuntimeError, match="multiple"):
        kcall("w2e_proj_front_fwd", P(x), None, 1, 3, 16, 16, 3, P(x), None)
    with pytest.raises(RuntimeError, match="go together"):
        kcall("w2e_proj_front_fwd", P(x), P(x), 1, 3, 16, 16, 2, P(x), None)
    with pytest.raises(RuntimeError, match="needs small and target"):
        kcall("w2e_proj_front_bwd", P(x), None, None, P(x), 1.0, 1, 3, 16, 16, 2, P(x))
