"""The entry points of csrc/mapper.hip (K7) that tests/test_gpu_mapper_kernels.py does not hold (it holds w2e_mapper_linear), one by one
through the C ABI against the float64 restatement of tests/mapper_ref.py (held to oracle/mappers.py and to float64 autograd by
tests/test_mapper_ref_host.py): w2e_mapper_pixelnorm, w2e_mapper_wgrad, w2e_ssmapper_pixelnorm, w2e_ssmapper_gather,
w2e_ssmapper_linear (both modes), w2e_ssmapper_wgrad.

Inputs: heavy-tailed operands (normal^3); layer outputs y of both signs with one entry in eight exactly 0 and a few -0.0 (the slope
branch is y > 0); biases of order 30 (they are scaled by 0.01).  Every output is pre-filled with NaN between sentinels that must survive,
every input sits between sentinels, and what a call has no business reading is NaN: the latents of x, gy and y outside every level, the
slack around the code tensors (which sit at addresses that are 4-byte but not 16-byte aligned).  Two calls on the same inputs must give
equal bits (the header promises a fixed summation order).

How the error is judged: EVERY element, |got - ref| <= N * 2^-24 * scale, no element excluded.
  products and column sums (the two wgrads, both modes of ssmapper_linear): N = K + 8, scale = the formula on absolute values
      (mapper_ref.*_scale), K = the number of summed terms: the rows of the group (the batch) for the wgrads, the code width for the
      style-space products.  That is the worst-case bound of any correct fp32 sum of K products in any order, plus at most 8 roundings
      around it, counted from the source: gpre = gy * sqrt2f * slope (2 roundings + 0.3 + 0.25 for the two fp32 constants), the fp32
      w_scale / b_scale and its product (1.5), in the forward bias * b_scale, its addition, slope and gain (4.6).  A dropped or doubled
      term of typical size lands near 1 / K of the scale: at K = 1152 still ten times above the bound.
  PixelNorm outputs: N = (K + 2) / 2 + RSQRT_ULP + 1, scale = |h_ref|, K = the length of the mean (len of the level, dim of the code):
      the sum of K squares is all-positive, so its relative error is at most K roundings; + the division and the epsilon add; rsqrt
      halves a relative error; + device rsqrtf (RSQRT_ULP, the assumption DESIGN.md names) + the final product.
`-s` prints the worst ratio of every comparison; the last test prints the table DESIGN.md quotes.  A census of what the five mappers of
where2edit_amd/latent_mappers.py really call is held against COVERAGE."""
import ctypes
import math

import pytest
import torch

import mapper_ref as R
import seeded
from test_gpu_gen_small_kernels import GUARD, RSQRT_ULP, SENTINEL, Buf, _stop_after_a_gpu_fault, inp  # noqa: F401  (the fixture is autouse here too)
from test_gpu_mapper_kernels import CASES as LINEAR_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, U = R.D, R.U
LR_MUL = 0.01
W_SCALE, B_SCALE = LR_MUL / math.sqrt(D), LR_MUL   # EqualLinear(512, 512, lr_mul=0.01): model.py:130-164
WORST = {}         # entry point / output -> (share of the bound, ratio in 2^-24 of the term scale, the bound there)
EXERCISED = set()  # (entry point, path class) of every call this file's tests made

# name -> (batch, n_latent, levels): the cases of test_gpu_mapper_kernels.py at n_latent = 18 and the 64^2 generator's 10 latents
CASES = {name: (batch, 18, levels) for name, (batch, levels) in LINEAR_CASES.items()}
CASES["b2_n10"] = (2, 10, ((0, 4), (4, 4), (8, 2)))

REAL_DIMS = (512,) * 15 + (256,) * 3 + (128,) * 3 + (64,) * 3 + (32,) * 2          # STYLESPACE_DIMENSIONS
NO_TORGB_DIMS = tuple(d for c, d in enumerate(REAL_DIMS) if c not in range(1, 26, 3))  # WithoutToRGBStyleSpaceMapper's 17 codes
RAGGED_DIMS = (1, 3, 33, 64, 65, 100, 257, 600)   # ABI only: no multiple of 64 / 256, one wave and several, more than one 256-column block
WIDE_DIMS = (1000, 32)                            # four blocks per code in ss_linear_bwd_kernel, each staging the LDS itself
# name -> (dims, batch);  batch * max(dim) * 4 <= 64000 bytes everywhere (mode 1 stages gpre of a code in LDS)
SS_CASES = {"full_b1": (REAL_DIMS, 1), "full_b2": (REAL_DIMS, 2), "full_b16": (REAL_DIMS, 16), "no_torgb_b4": (NO_TORGB_DIMS, 4),
            "ragged_b3": (RAGGED_DIMS, 3), "ragged_b16": (RAGGED_DIMS, 16), "wide_b3": (WIDE_DIMS, 3)}
OPTIONAL = ["given", "null", "one_null"]   # an optional pointer array: every entry given, the array NULL, one entry NULL


# ---------------------------------------------------------------------------------------------- the path class of a call
def _opt_class(arr):
    """An optional array of pointers: "-" = NULL, "all" = every entry given, "some" = a NULL entry among them."""
    if arr is None:
        return "-"
    return "all" if all(v for v in list(arr)) else "some"


def _int(v):
    return int(getattr(v, "value", v))


def path_class(name, args):
    """What the host code and the kernels branch on, read from the arguments handed to the library.  (`scatter` belongs to mode 0 and
    `gathered` to mode 1 of w2e_mapper_linear -- include/w2e.h -- and mode 1 of both linears drops the bias.)"""
    if name == "w2e_mapper_pixelnorm":
        return (_int(args[4]),)
    if name == "w2e_mapper_linear":
        mode, groups = _int(args[0]), _int(args[8])
        return (0, _int(args[13]), _opt_class(args[5]), groups) if mode == 0 else (1, _int(args[14]), groups)
    if name == "w2e_mapper_wgrad":
        return (_int(args[12]), _opt_class(args[4]), _int(args[7]))
    if name == "w2e_ssmapper_pixelnorm":
        return (_int(args[3]),)
    if name == "w2e_ssmapper_gather":
        return (_opt_class(args[0]), _int(args[3]))
    if name == "w2e_ssmapper_linear":
        mode, groups = _int(args[0]), _int(args[7])
        return (0, _opt_class(args[5]), groups) if mode == 0 else (1, groups)
    if name == "w2e_ssmapper_wgrad":
        return (_opt_class(args[4]), _int(args[6]))
    raise KeyError(name)


_LEVEL_GROUPS = sorted({len(levels) for _, _, levels in CASES.values()})
_SS_GROUPS = sorted({len(dims) for dims, _ in SS_CASES.values()})
assert _LEVEL_GROUPS == [1, 2, 3, 4] and _SS_GROUPS == [2, 8, 17, 26]
# (entry point, path class) -> the test that exercises it
COVERAGE = {}
COVERAGE.update({("w2e_mapper_pixelnorm", (g,)): "test_mapper_pixelnorm" for g in _LEVEL_GROUPS})
COVERAGE.update({("w2e_mapper_wgrad", (gathered, gb, g)): "test_mapper_wgrad"
                 for gathered in (0, 1) for gb in ("all", "-", "some") for g in _LEVEL_GROUPS})
COVERAGE.update({("w2e_ssmapper_pixelnorm", (g,)): "test_ssmapper_pixelnorm" for g in _SS_GROUPS})
COVERAGE.update({("w2e_ssmapper_gather", (src, g)): "test_ssmapper_gather" for src in ("all", "some") for g in _SS_GROUPS})
COVERAGE.update({("w2e_ssmapper_linear", (0, b, g)): "test_ssmapper_linear_forward" for b in ("all", "-", "some") for g in _SS_GROUPS})
COVERAGE.update({("w2e_ssmapper_linear", (1, g)): "test_ssmapper_linear_input_gradient" for g in _SS_GROUPS})
COVERAGE.update({("w2e_ssmapper_wgrad", (gb, g)): "test_ssmapper_wgrad" for gb in ("all", "-", "some") for g in _SS_GROUPS})
# w2e_mapper_linear is held by tests/test_gpu_mapper_kernels.py, which records no set: what its parametrisation calls, as a table.
# test_forward_matches_float64: CASES x scatter {0, 1} x bias {given, NULL}; test_input_gradient_matches_float64: CASES x gathered {1, 0};
# its CASES have 1, 2, 3 and 4 groups (asserted above: the cases here are the same ones).
COVERAGE.update({("w2e_mapper_linear", (0, scatter, b, g)): "test_gpu_mapper_kernels.py::test_forward_matches_float64"
                 for scatter in (0, 1) for b in ("all", "-") for g in _LEVEL_GROUPS})
COVERAGE.update({("w2e_mapper_linear", (1, gathered, g)): "test_gpu_mapper_kernels.py::test_input_gradient_matches_float64"
                 for gathered in (0, 1) for g in _LEVEL_GROUPS})
ENTRY_POINTS = sorted({n for n, _ in COVERAGE})


# ---------------------------------------------------------------------------------------------- calling and judging
def _lib():
    from where2edit_amd import _lib as L
    return L


def kcall(name, *args):
    L = _lib()
    L.call(name, *args, L.stream_ptr())
    torch.cuda.synchronize()
    EXERCISED.add((name, path_class(name, args)))  # (after the call: a refused call exercises nothing)


def P(t):
    return _lib().ptr(t)


def ptrs(tensors):
    """A HOST array of device pointers; None entries are NULL."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def ints(values):
    return (ctypes.c_int * len(values))(*values)


def floats(values):
    return (ctypes.c_float * len(values))(*values)


def optional(bufs, mode):
    """The pointer array of an optional operand list in one of the OPTIONAL modes, and the index left NULL (or None)."""
    if mode == "null":
        return None, None
    hole = len(bufs) // 2 if mode == "one_null" else None
    return ptrs([None if i == hole else b.v for i, b in enumerate(bufs)]), hole


def judge(got, ref, scale, bound, what, quiet=False):
    """Every element of `got` within `bound` (a number or a tensor) fp32 roundings of float64, relative to ITS OWN scale; an element
    whose scale is 0 must be exact.  Returns the worst ratio to the bound (quiet: the caller prints one line for many comparisons)."""
    got = got.detach().double().cpu()
    ref, scale = R.f64(ref).reshape(got.shape), R.f64(scale).reshape(got.shape)
    bound = (R.f64(bound) if torch.is_tensor(bound) else torch.tensor(float(bound), dtype=torch.float64)).expand(got.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written (NaN left) or not finite"
    assert float(got.abs().max()) < 1e-10 * SENTINEL, f"{what}: a sentinel was read"
    share = (got - ref).abs() / (bound * U * scale).clamp_min(1e-300)
    i = int(share.argmax())
    s, n = float(share.reshape(-1)[i]), float(bound.reshape(-1)[i])
    key = what.split(" [")[0]
    if s >= WORST.get(key, (-1.0, 0.0, 0.0))[0]:
        WORST[key] = (s, s * n, n)
    if not quiet:
        print(f"{what}: worst element {s * n:.3f} x 2^-24 of its scale (bound there {n:g}): {s:.4f} of the bound")
    assert s <= 1.0, f"{what}: element {i} is {s * n:.3f} x 2^-24 of its scale from float64 (bound {n:g})"
    return s


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def heavy(key, shape, scale=1.0):
    return (seeded.tensor(key, shape) ** 3 * scale).contiguous()


def layer_output(key, shape):
    """Both signs, one entry in eight exactly 0, one in sixty-four -0.0."""
    y = heavy(key, shape)
    y.view(-1)[::8] = 0.0
    y.view(-1)[4::64] = -0.0
    assert bool((y > 0).any()) and bool((y < 0).any()) and bool(torch.signbit(y[y == 0]).any())
    return y


# ---------------------------------------------------------------------------------------------- the level mappers
def _covered(batch, n_latent, levels):
    m = torch.zeros(batch, n_latent, D, dtype=torch.bool)
    for l0, ln in levels:
        m[:, l0:l0 + ln] = True
    return m


@pytest.fixture(scope="module")
def level_case():
    """Per case: the CPU inputs, their guarded device copies and the float64 references -- made once, read-only."""
    made = {}

    def make(name):
        if name in made:
            return made[name]
        batch, n_latent, levels = CASES[name]
        rows = batch * sum(ln for _, ln in levels)
        nan_outside = lambda t: torch.where(_covered(batch, n_latent, levels), t, torch.full_like(t, float("nan")))  # noqa: E731
        x = heavy(f"maprest.{name}.x", (batch, n_latent, D))
        x[0, :, 5] = 0.0                                                           # a (sample, feature) column of zeros: h = 0, not NaN
        x[-1, :, 7] = 1e-6 * torch.where(torch.arange(n_latent) % 2 == 0, 1.0, -1.0)  # mean x^2 = 1e-12: the epsilon dominates
        x = nan_outside(x)
        gy_full = nan_outside(heavy(f"maprest.{name}.gy", (batch, n_latent, D)))
        y_full = nan_outside(layer_output(f"maprest.{name}.y", (batch, n_latent, D)))
        h_in = heavy(f"maprest.{name}.h", (rows, D))
        gy_rows, y_rows = R.gather_rows(gy_full, levels).contiguous(), R.gather_rows(y_full, levels).contiguous()
        assert not torch.isnan(gy_rows).any() and not torch.isnan(y_rows).any()
        h_ref = R.levels_pixelnorm(x, levels)
        assert h_ref.shape == (rows, D) and bool(torch.isfinite(h_ref).all())
        h_bound = torch.cat([torch.full((batch * ln, 1), (ln + 2) / 2 + RSQRT_ULP + 1, dtype=torch.float64) for _, ln in levels], 0)
        zero_col = torch.zeros(batch, n_latent, D, dtype=torch.bool)
        zero_col[0, :, 5] = True
        gp = R.split_rows(R.gpre(gy_rows, y_rows), batch, levels)
        hs = R.split_rows(h_in, batch, levels)
        made[name] = dict(batch=batch, n_latent=n_latent, levels=levels, rows=rows, x=inp(x), gy_full=inp(gy_full), y_full=inp(y_full),
                          gy_rows=inp(gy_rows), y_rows=inp(y_rows), h_in=inp(h_in), h_ref=h_ref, h_bound=h_bound,
                          zero_rows=R.gather_rows(zero_col, levels),
                          wgrad=[R.wgrad(g, h, W_SCALE, B_SCALE) + R.wgrad_scale(g, h, W_SCALE, B_SCALE) for g, h in zip(gp, hs)])
        return made[name]

    return make


def _geom(c):
    return c["batch"], c["n_latent"], len(c["levels"]), ints([lv[0] for lv in c["levels"]]), ints([lv[1] for lv in c["levels"]])


@pytest.mark.parametrize("name", list(CASES))
def test_mapper_pixelnorm(level_case, name):
    """w2e_mapper_pixelnorm.  Roundings (mapper_pixelnorm_kernel): L FMAs of the all-positive sum of squares, s / L, + 1e-8f -> at most
    L + 2 on the argument, halved by rsqrt; rsqrtf (RSQRT_ULP); x * r (1):  N = (L + 2) / 2 + RSQRT_ULP + 1, L = len of the level.
    h has exactly batch * sum(len) rows; the latents of x outside every level are NaN."""
    c = level_case(name)
    outs = []
    for _ in range(2):
        h = Buf(shape=(c["rows"], D))
        kcall("w2e_mapper_pixelnorm", P(c["x"].v), P(h.v), *_geom(c))
        assert h.intact() and c["x"].intact(), "wrote outside the output"
        outs.append(h)
    judge(outs[0].v, c["h_ref"], c["h_ref"].abs(), c["h_bound"], f"w2e_mapper_pixelnorm [{name}]")
    got = outs[0].v.cpu()
    assert bool(c["zero_rows"].any()) and bool((got[c["zero_rows"]] == 0).all()), "a column of zeros must map to 0"
    assert same_bits(outs[0].v, outs[1].v), "two calls on the same inputs differ"


@pytest.mark.parametrize("gb_mode", OPTIONAL)
@pytest.mark.parametrize("gathered", [1, 0], ids=["grouped", "ungathered"])
@pytest.mark.parametrize("name", list(CASES))
def test_mapper_wgrad(level_case, name, gathered, gb_mode):
    """w2e_mapper_wgrad: every group's gw and gb in its own guarded buffer.  Roundings (mapper_wgrad_kernel): gpre 2.6, one FMA per row
    of the group in ascending order (K = rows), the fp32 scale and its product 1.5:  N = K + 8 with K = batch * len of the group.
    b2_four_groups (2, 4, 10, 20 rows) and step_b4 (16, 16, 40) index an LDS sized by the LARGEST group with every group's own row
    count; b64_single is the 1152-row limit.  gb NULL, and gb with one NULL entry, must leave every other output as it was, bit for bit."""
    c = level_case(name)
    g = len(c["levels"])
    gy, y = (c["gy_rows"], c["y_rows"]) if gathered else (c["gy_full"], c["y_full"])

    def run(mode):
        gw, gb = [Buf(shape=(D, D)) for _ in range(g)], [Buf(shape=(D,)) for _ in range(g)]
        gb_arg, hole = optional(gb, mode)
        batch, n_latent, groups, l0, ln = _geom(c)
        kcall("w2e_mapper_wgrad", P(gy.v), P(y.v), P(c["h_in"].v), ptrs([b.v for b in gw]), gb_arg, batch, n_latent, groups, l0, ln,
              W_SCALE, B_SCALE, gathered)
        assert all(b.intact() for b in gw + gb + [gy, y, c["h_in"]]), "wrote outside an output"
        return gw, gb, [i for i in range(g) if mode != "null" and i != hole]

    gw, gb, given = run(gb_mode)
    for i, (_, ln) in enumerate(c["levels"]):
        gw_ref, gb_ref, gw_scale, gb_scale = c["wgrad"][i]
        n = c["batch"] * ln + 8
        judge(gw[i].v, gw_ref, gw_scale, n, f"w2e_mapper_wgrad gw [{name} group {i} gathered={gathered} {gb_mode}]")
        if i in given:
            judge(gb[i].v, gb_ref, gb_scale, n, f"w2e_mapper_wgrad gb [{name} group {i} gathered={gathered} {gb_mode}]")
        else:
            assert gb[i].untouched(), "a bias gradient that was not asked for was written"
    gw2, gb2, _ = run("given")   # the same bits again, and the same bits whatever gb was
    assert all(same_bits(a.v, b.v) for a, b in zip(gw, gw2)), "gw depends on gb, or two calls on the same inputs differ"
    assert all(same_bits(gb[i].v, gb2[i].v) for i in given), "gb depends on its neighbours, or two calls on the same inputs differ"


@pytest.mark.parametrize("entry", ["w2e_mapper_pixelnorm", "w2e_mapper_wgrad"])
def test_more_rows_than_the_limit_are_refused_and_nothing_is_written(entry):
    batch, levels = 65, ((0, 18),)   # 1170 rows > MAP_MAXROWS = 1152: a host-side check that returns before any launch
    rows = batch * 18
    a = torch.ones(batch, 18, D, device=DEV)
    outs = [Buf(shape=(rows, D), fill=7.0)] if entry == "w2e_mapper_pixelnorm" else [Buf(shape=(D, D), fill=7.0), Buf(shape=(D,), fill=7.0)]
    with pytest.raises(RuntimeError, match="bad groups"):
        if entry == "w2e_mapper_pixelnorm":
            kcall(entry, P(a), P(outs[0].v), batch, 18, 1, ints([0]), ints([18]))
        else:
            kcall(entry, P(a), P(a), P(a), ptrs([outs[0].v]), ptrs([outs[1].v]), batch, 18, 1, ints([0]), ints([18]), W_SCALE, B_SCALE, 1)
    torch.cuda.synchronize()
    assert all(b.intact() and bool((b.v == 7.0).all()) for b in outs)


# ---------------------------------------------------------------------------------------------- the style-space mappers
def _offset_copy(t, off):
    """A device copy of t that starts `off` floats past a 16-byte boundary, NaN slack around it inside the guards: (Buf, the view)."""
    n = t.numel()
    b = Buf(shape=(n + 4,))
    v = b.v[off:off + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == 0 and (v.data_ptr() % 16 != 0) == (off % 4 != 0)
    return b, v


def _per_code(values, batch, dims):
    """A packed vector that holds values[c] in every element of code c's block."""
    return torch.cat([torch.full((batch * d,), float(v), dtype=torch.float64) for v, d in zip(values, dims)], 0)


@pytest.fixture(scope="module")
def ss_case():
    """Per case: the CPU inputs, their guarded device copies and lazily the float64 references -- made once, read-only."""
    made = {}

    def make(name):
        if name in made:
            return made[name]
        dims, batch = SS_CASES[name]
        assert batch * max(dims) * 4 <= 64000
        g, total = len(dims), batch * sum(dims)
        xs = [heavy(f"ssrest.{name}.x{c}", (batch, d)) for c, d in enumerate(dims)]
        xs[0][0], xs[-1][0] = 0.0, 0.0      # rows of zeros: h = 0, not NaN
        xs[1][-1] = 1e-6                    # mean x^2 = 1e-12: the epsilon dominates
        w = [heavy(f"ssrest.{name}.w{c}", (d, d), 100.0 / 3.0) for c, d in enumerate(dims)]
        bias = [seeded.tensor(f"ssrest.{name}.b{c}", (d,), std=30.0) for c, d in enumerate(dims)]
        a, gy, h_in = (heavy(f"ssrest.{name}.{k}", (total,)) for k in ("a", "gy", "h"))
        y = layer_output(f"ssrest.{name}.y", (total,))
        w_scale = [LR_MUL / math.sqrt(d) for d in dims]   # differs from code to code
        gp = R.ss_unpack(R.gpre(gy, y), batch, dims)
        c = dict(dims=dims, batch=batch, groups=g, total=total, xs=xs, w_cpu=w, bias_cpu=bias, w_scale=w_scale, gp=gp,
                 a_cpu=R.ss_unpack(a, batch, dims), h_cpu=R.ss_unpack(h_in, batch, dims), gy_cpu=R.ss_unpack(gy, batch, dims),
                 a=inp(a), gy=inp(gy), y=inp(y), h_in=inp(h_in), w=[inp(t) for t in w], bias=[inp(t) for t in bias], refs={})
        made[name] = c
        return c

    return make


def _ss_geom(c):
    return c["batch"], c["groups"], ints(c["dims"])


def _inputs_intact(c):
    return all(b.intact() for b in [c["a"], c["gy"], c["y"], c["h_in"]] + c["w"] + c["bias"])


@pytest.mark.parametrize("name", list(SS_CASES))
def test_ssmapper_pixelnorm(ss_case, name):
    """w2e_ssmapper_pixelnorm.  Roundings (ss_pixelnorm_kernel): ceil(d / 64) FMAs per lane + 6 butterfly additions of the all-positive
    sum (<= d for d >= 3; at d = 1, 2 the butterfly adds zeros: exact), s / d, + 1e-8f -> at most d + 2 on the argument, halved by rsqrt;
    rsqrtf (RSQRT_ULP); x * r (1):  N = (d + 2) / 2 + RSQRT_ULP + 1, d = the code's width.  The code tensors start 1, 2 or 3 floats past
    a 16-byte boundary (the kernel uses scalar loads), NaN around them."""
    c = ss_case(name)
    dims, batch = c["dims"], c["batch"]
    held = [_offset_copy(x, 1 + k % 3) for k, x in enumerate(c["xs"])]
    ref = R.ss_pixelnorm(c["xs"])
    bound = _per_code([(d + 2) / 2 + RSQRT_ULP + 1 for d in dims], batch, dims)
    outs = []
    for _ in range(2):
        h = Buf(shape=(c["total"],))
        kcall("w2e_ssmapper_pixelnorm", ptrs([v for _, v in held]), P(h.v), *_ss_geom(c))
        assert h.intact() and all(b.intact() for b, _ in held), "wrote outside the output"
        outs.append(h)
    judge(outs[0].v, ref, ref.abs(), bound, f"w2e_ssmapper_pixelnorm [{name}]")
    got = R.ss_unpack(outs[0].v.cpu(), batch, dims)
    assert bool((got[0][0] == 0).all()) and bool((got[-1][0] == 0).all()), "a row of zeros must map to 0"
    assert same_bits(outs[0].v, outs[1].v), "two calls on the same inputs differ"


@pytest.mark.parametrize("nulls", [False, True], ids=["all", "some_null"])
@pytest.mark.parametrize("name", list(SS_CASES))
def test_ssmapper_gather(ss_case, name, nulls):
    """w2e_ssmapper_gather: the packed block of a NULL entry is exactly 0, every other block a bit copy of its source (which sits at
    an address that is not 16-byte aligned, -0.0 among its values); the floats after the last block keep the sentinel."""
    c = ss_case(name)
    dims, batch = c["dims"], c["batch"]
    src = [t.clone() for t in c["gy_cpu"]]
    for t in src:
        t.view(-1)[0] = -0.0
    null = [nulls and k % 3 == 1 for k in range(len(dims))]
    if nulls and len(dims) == 2:
        null = [True, False]   # (the first block: the offset of the second must not depend on the first's source)
    held = [None if z else _offset_copy(t, 1 + k % 3) for k, (t, z) in enumerate(zip(src, null))]
    dst = Buf(shape=(c["total"],))
    kcall("w2e_ssmapper_gather", ptrs([None if h is None else h[1] for h in held]), P(dst.v), *_ss_geom(c))
    assert dst.intact() and all(h is None or h[0].intact() for h in held), "wrote outside the packed output"
    got = R.ss_unpack(dst.v.cpu(), batch, dims)
    for k, (t, z) in enumerate(zip(src, null)):
        if z:
            assert bool((got[k] == 0).all()), f"code {k}: a NULL entry must be packed as zeros"
        else:
            assert same_bits(got[k], t), f"code {k}: not a bit copy"


def _ss_forward_ref(c, mode):
    """(ref, scale, bound) of mode 0, packed, for a bias list in one of the OPTIONAL modes -- cached."""
    if ("fwd", mode) not in c["refs"]:
        dims, batch = c["dims"], c["batch"]
        hole = len(dims) // 2 if mode == "one_null" else None
        refs, scales = [], []
        for k, d in enumerate(dims):
            b = None if (mode == "null" or k == hole) else c["bias_cpu"][k]
            refs.append(R.linear_fwd(c["a_cpu"][k], c["w_cpu"][k], b, c["w_scale"][k], B_SCALE))
            scales.append(R.linear_fwd_scale(c["a_cpu"][k], c["w_cpu"][k], b, c["w_scale"][k], B_SCALE, d + 8))
        c["refs"][("fwd", mode)] = (R.ss_pack(refs), R.ss_pack(scales), _per_code([d + 8 for d in dims], batch, dims))
    return c["refs"][("fwd", mode)]


@pytest.mark.parametrize("bias_mode", OPTIONAL)
@pytest.mark.parametrize("name", list(SS_CASES))
def test_ssmapper_linear_forward(ss_case, name, bias_mode):
    """w2e_ssmapper_linear mode 0.  Roundings (ss_linear_fwd_kernel): ceil(d / 64) FMAs per lane + 6 butterfly additions (<= d for
    d >= 3; at d = 1, 2 one product and at most one addition), then s * w_scale (1.5), bias * b_scale (1.5), their addition, slope (1.25)
    and gain (1.3):  N = K + 8 with K = d, the code's width; w_scale differs from code to code."""
    c = ss_case(name)
    ref, scale, bound = _ss_forward_ref(c, bias_mode)
    bias_arg, _ = optional(c["bias"], bias_mode)
    outs = []
    for _ in range(2):
        out = Buf(shape=(c["total"],))
        batch, groups, dims = _ss_geom(c)
        kcall("w2e_ssmapper_linear", 0, P(c["a"].v), None, P(out.v), ptrs([b.v for b in c["w"]]), bias_arg, batch, groups, dims,
              floats(c["w_scale"]), B_SCALE)
        assert out.intact() and _inputs_intact(c), "wrote outside the output"
        outs.append(out)
    judge(outs[0].v, ref, scale, bound, f"w2e_ssmapper_linear forward [{name} bias {bias_mode}]")
    assert same_bits(outs[0].v, outs[1].v), "two calls on the same inputs differ"


@pytest.mark.parametrize("name", list(SS_CASES))
def test_ssmapper_linear_input_gradient(ss_case, name):
    """w2e_ssmapper_linear mode 1.  Roundings (ss_linear_bwd_kernel): gpre 2.6, one FMA per output feature in ascending order (K = d),
    the fp32 w_scale and its product 1.5:  N = K + 8.  Codes wider than 256 take more than one block, each staging gpre in LDS itself
    (wide_b3: four blocks of code 0, the last with 232 columns); a bias handed to mode 1 is ignored."""
    c = ss_case(name)
    dims, batch = c["dims"], c["batch"]
    if "bwd" not in c["refs"]:
        c["refs"]["bwd"] = (R.ss_pack([R.linear_bwd(c["gp"][k], c["w_cpu"][k], c["w_scale"][k]) for k in range(len(dims))]),
                            R.ss_pack([R.linear_bwd_scale(c["gp"][k], c["w_cpu"][k], c["w_scale"][k]) for k in range(len(dims))]))
    ref, scale = c["refs"]["bwd"]
    outs = []
    for bias_arg in (None, ptrs([b.v for b in c["bias"]])):
        out = Buf(shape=(c["total"],))
        b_, groups, dims_c = _ss_geom(c)
        kcall("w2e_ssmapper_linear", 1, P(c["gy"].v), P(c["y"].v), P(out.v), ptrs([b.v for b in c["w"]]), bias_arg, b_, groups, dims_c,
              floats(c["w_scale"]), B_SCALE)
        assert out.intact() and _inputs_intact(c), "wrote outside the output"
        outs.append(out)
    judge(outs[0].v, ref, scale, _per_code([d + 8 for d in dims], batch, dims), f"w2e_ssmapper_linear input gradient [{name}]")
    assert same_bits(outs[0].v, outs[1].v), "two calls on the same inputs differ, or mode 1 read the bias"


@pytest.mark.parametrize("gb_mode", OPTIONAL)
@pytest.mark.parametrize("name", list(SS_CASES))
def test_ssmapper_wgrad(ss_case, name, gb_mode):
    """w2e_ssmapper_wgrad: every code's gw and gb in its own guarded buffer.  Roundings (ss_wgrad_kernel): gpre 2.6, one FMA per sample in
    ascending order (K = batch), the fp32 scale and its product 1.5:  N = K + 8 with K = batch."""
    c = ss_case(name)
    dims, batch = c["dims"], c["batch"]
    if "wgrad" not in c["refs"]:
        c["refs"]["wgrad"] = [R.wgrad(c["gp"][k], c["h_cpu"][k], c["w_scale"][k], B_SCALE) + R.wgrad_scale(c["gp"][k], c["h_cpu"][k], c["w_scale"][k], B_SCALE)
                              for k in range(len(dims))]

    def run(mode):
        gw, gb = [Buf(shape=(d, d)) for d in dims], [Buf(shape=(d,)) for d in dims]
        gb_arg, hole = optional(gb, mode)
        b_, groups, dims_c = _ss_geom(c)
        kcall("w2e_ssmapper_wgrad", P(c["gy"].v), P(c["y"].v), P(c["h_in"].v), ptrs([b.v for b in gw]), gb_arg, b_, groups, dims_c,
              floats(c["w_scale"]), B_SCALE)
        assert all(b.intact() for b in gw + gb) and _inputs_intact(c), "wrote outside an output"
        return gw, gb, [k for k in range(len(dims)) if mode != "null" and k != hole]

    gw, gb, given = run(gb_mode)
    worst_w = worst_b = 0.0
    for k in range(len(dims)):
        gw_ref, gb_ref, gw_scale, gb_scale = c["refs"]["wgrad"][k]
        worst_w = max(worst_w, judge(gw[k].v, gw_ref, gw_scale, batch + 8, f"w2e_ssmapper_wgrad gw [{name} code {k} {gb_mode}]", quiet=True))
        if k in given:
            worst_b = max(worst_b, judge(gb[k].v, gb_ref, gb_scale, batch + 8, f"w2e_ssmapper_wgrad gb [{name} code {k} {gb_mode}]", quiet=True))
        else:
            assert gb[k].untouched(), "a bias gradient that was not asked for was written"
    print(f"w2e_ssmapper_wgrad [{name} {gb_mode}]: worst element over the {len(dims)} codes {worst_w * (batch + 8):.3f} (gw), "
          f"{worst_b * (batch + 8):.3f} (gb) x 2^-24 of its scale (bound {batch + 8})")
    gw2, gb2, _ = run("given")
    assert all(same_bits(a.v, b.v) for a, b in zip(gw, gw2)), "gw depends on gb, or two calls on the same inputs differ"
    assert all(same_bits(gb[k].v, gb2[k].v) for k in given), "gb depends on its neighbours, or two calls on the same inputs differ"


SS_KINDS = ["pixelnorm", "gather", "linear0", "linear1", "wgrad"]
REFUSED = {"batch17": (17, (8, 4)), "codes33": (2, (4,) * 33), "dim0": (2, (4, 0, 4)), "dim4097": (2, (4, 4097))}


def _ss_refused_call(kind, batch, dims):
    """One call of `kind` whose buffers are as large as the geometry asks (a width of 0 gets one float), outputs holding 7.0 between
    guards: -> the outputs.  Every refusal below is a host-side argument check that returns before any launch."""
    sizes = [max(d, 1) for d in dims]
    total = batch * sum(sizes)
    act = torch.ones(total, device=DEV)
    codes = [torch.ones(batch * s, device=DEV) for s in sizes]
    geom = (batch, len(dims), ints(dims))
    ws = floats([0.5] * len(dims))
    if kind in ("pixelnorm", "gather"):
        outs = [Buf(shape=(total,), fill=7.0)]
        call = lambda: kcall(f"w2e_ssmapper_{kind}", ptrs(codes), P(outs[0].v), *geom)  # noqa: E731
    elif kind in ("linear0", "linear1"):
        outs = [Buf(shape=(total,), fill=7.0)]
        w = [torch.zeros(s * s, device=DEV) for s in sizes]
        mode = int(kind[-1])
        call = lambda: kcall("w2e_ssmapper_linear", mode, P(act), P(act) if mode else None, P(outs[0].v), ptrs(w), None, *geom, ws, B_SCALE)  # noqa: E731
    else:
        gw, gb = [Buf(shape=(s * s,), fill=7.0) for s in sizes], [Buf(shape=(s,), fill=7.0) for s in sizes]
        outs = gw + gb
        call = lambda: kcall("w2e_ssmapper_wgrad", P(act), P(act), P(act), ptrs([b.v for b in gw]), ptrs([b.v for b in gb]), *geom, ws, B_SCALE)  # noqa: E731
    return call, outs


@pytest.mark.parametrize("what", list(REFUSED))
@pytest.mark.parametrize("kind", SS_KINDS)
def test_ssmapper_refuses_what_it_cannot_serve_and_writes_nothing(kind, what):
    """batch 17 (> 16), 33 codes (> 32), a width of 0 and a width of 4097 (> 4096): ss_fill refuses each for every entry point."""
    batch, dims = REFUSED[what]
    call, outs = _ss_refused_call(kind, batch, dims)
    before = set(EXERCISED)
    with pytest.raises(RuntimeError, match=r"1\.\.32 codes, batch 1\.\.16"):
        call()
    torch.cuda.synchronize()
    assert all(b.intact() and bool((b.v == 7.0).all()) for b in outs) and EXERCISED == before


def test_ssmapper_linear_refuses_a_staged_gradient_beyond_the_lds():
    """Mode 1 stages batch x max(dim) floats of gpre in LDS: batch 16 x width 2048 = 128 KiB is refused (64 KiB); mode 0 has no such
    limit and is not called here."""
    call, outs = _ss_refused_call("linear1", 16, (2048,))
    with pytest.raises(RuntimeError, match="too large for the staged gradient"):
        call()
    torch.cuda.synchronize()
    assert all(b.intact() and bool((b.v == 7.0).all()) for b in outs)


# ---------------------------------------------------------------------------------------------- the census
def test_census_of_the_paths_the_mappers_take(monkeypatch):
    """LevelsMapper (three levels; the medium level disabled), SingleMapper, FullStyleSpaceMapper and WithoutToRGBStyleSpaceMapper,
    each forward and backward once with every call of mapper_hip recorded as (entry point, path class): every recorded pair is a
    COVERAGE row, and every entry point of csrc/mapper.hip was seen -- so an empty record fails."""
    from types import SimpleNamespace

    import where2edit_amd.mapper_hip as MH
    from where2edit_amd import latent_mappers as LM
    seen = {}
    real_call = MH.call

    def recording(name, *args):
        key = (name, path_class(name, args))
        seen[key] = seen.get(key, 0) + 1
        return real_call(name, *args)

    monkeypatch.setattr(MH, "call", recording)
    monkeypatch.delenv("W2E_MAPPER_STOCK", raising=False)
    batch = 2
    gen = torch.Generator().manual_seed(11)
    for kind in ("levels", "no_medium", "single", "full", "without_torgb"):
        opts = SimpleNamespace(no_coarse_mapper=False, no_medium_mapper=kind == "no_medium", no_fine_mapper=False)
        cls = {"levels": LM.LevelsMapper, "no_medium": LM.LevelsMapper, "single": LM.SingleMapper, "full": LM.FullStyleSpaceMapper,
               "without_torgb": LM.WithoutToRGBStyleSpaceMapper}[kind]
        torch.manual_seed(3)
        m = cls(opts).to(DEV)
        n_before = sum(seen.values())
        if kind in ("full", "without_torgb"):
            x = [torch.randn(batch, 1, d, 1, 1, generator=gen).to(DEV) for d in LM.STYLESPACE_DIMENSIONS]
            y = m(x)
            loss = sum((a * a).sum() for a in y if a.requires_grad)
        else:
            x = torch.randn(batch, 18, D, generator=gen).to(DEV)
            loss = (m(x) ** 2).sum()
        loss.backward()
        torch.cuda.synchronize()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters()), kind
        # PixelNorm, 4 forward, 4 weight-gradient and 3 input-gradient launches (+ the style-space gather)
        assert sum(seen.values()) - n_before == (13 if kind in ("full", "without_torgb") else 12), kind
    for key in sorted(seen, key=str):
        print(f"census: {seen[key]:3d} x {key[0]} {key[1]}  <- {COVERAGE.get(key, 'NOT COVERED')}")
    missing = sorted((k for k in seen if k not in COVERAGE), key=str)
    assert not missing, f"calls of the mappers in a path class no test exercises: {missing}"
    assert {n for n, _ in seen} == set(ENTRY_POINTS), "an entry point of csrc/mapper.hip the mappers never called"


def test_zz_every_coverage_row_was_exercised_and_worst_ratios(request):
    """After the tests above (file order): every COVERAGE row that names a test of this file was really called with that path class by
    this file's tests, and they called nothing else -- checked when the whole file ran -- and the table of worst ratios per output."""
    for key in sorted(WORST):
        share, ratio, bound = WORST[key]
        print(f"worst: {ratio:9.3f} of {bound:<7g} ({share:.4f} of the bound)  {key}")
    whole_file = not request.config.getoption("keyword") and not any("::" in a for a in request.config.args)
    if whole_file:
        own = {k for k, t in COVERAGE.items() if "::" not in t}
        assert sorted(own - EXERCISED, key=str) == [], "COVERAGE rows no test of this file exercised"
        assert sorted(EXERCISED - own, key=str) == [], "calls of this file's tests that COVERAGE does not list"
