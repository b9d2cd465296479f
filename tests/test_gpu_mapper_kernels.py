"""The two products of the latent mapper's EqualLinear (csrc/mapper.hip, K7) one by one: w2e_mapper_linear mode 0 (forward) and mode 1
(input gradient, the weight as stored) called through the C ABI and held, element by element, against a float64 restatement of the
formulas in include/w2e.h computed on the CPU.

Inputs: heavy-tailed operands (normal^3), layer outputs y of both signs with one entry in eight exactly 0 (the slope branch is y > 0),
biases of order 30 (they are scaled by 0.01).  Shapes: the ones at which a (16 rows x 8 features) tiling can go wrong -- CASES.

Bound, for EVERY output element:  |got - ref| <= gamma * sum|terms|,  gamma = (K + 8) * 2^-24, K = 512: the worst-case bound of any
correct fp32 sum of K products, with a few roundings for scale, bias and activation (a dropped or doubled term of typical size lands
near 1/K of sum|terms|, about 60 times above).  sum|terms| is the same formula in float64 on |a|, |W|, |bias|, times the slope the
reference took (lrelu is 1-Lipschitz times its gain, so an element whose pre-activation is within the bound of 0 is judged with
slope 1).  Outputs are pre-filled with NaN between sentinels that must survive.  `-s` prints the worst ratio of every case.

The other entry points of csrc/mapper.hip -- w2e_mapper_pixelnorm, w2e_mapper_wgrad and the style-space w2e_ssmapper_* -- are held the
same way by tests/test_gpu_mapper_rest_kernels.py, which runs CASES too and holds a census of what the mappers really call against
both files (its COVERAGE table states this file's path classes: mode 0 x scatter x bias given / NULL, mode 1 x gathered, 1-4 groups)."""
import math

import pytest
import torch

import seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, N_LATENT, K = 512, 18, 512
GAMMA = (K + 8) * 2.0 ** -24
SLOPE, GAIN = 0.2, math.sqrt(2.0)
W_SCALE, B_SCALE = 0.01 / math.sqrt(D), 0.01   # EqualLinear(512, 512, lr_mul=0.01): model.py:130-164
STEP_LEVELS = ((0, 4), (4, 4), (8, 10))
GUARD, SENTINEL = 64, 1e30

# name -> (batch, levels)
CASES = {
    "step_b4": (4, STEP_LEVELS),                            # the step's own shape: 16 / 16 / 40 rows
    "b1": (1, STEP_LEVELS),                                 # 4 / 4 / 10 rows: fewer rows than any tile
    "b3_medium_only": (3, ((4, 4),)),                       # a disabled level: uncovered latents of the scattered output stay 0
    "b3_no_medium": (3, ((0, 4), (8, 10))),                 # LevelsMapper with no_medium_mapper: two groups, 12 / 30 rows, a gap between them
    "b5_single": (5, ((0, 18),)),                           # 90 rows: no multiple of 16 or 32
    "b64_single": (64, ((0, 18),)),                         # 1152 rows = MAP_MAXROWS
    "b2_four_groups": (2, ((0, 1), (1, 2), (3, 5), (8, 10))),  # four groups, one with 2 rows
}


def _heavy(key, shape, scale=1.0):
    return (seeded.tensor(key, shape) ** 3 * scale).contiguous()


def _layer_output(key, shape):
    """Both signs, one entry in eight exactly 0."""
    y = _heavy(key, shape)
    y.view(-1)[::8] = 0.0
    return y


def _gather(t, levels):
    """[B, n_latent, 512] -> group-major rows (row r0_g + b*len_g + l = latent l0_g + l of sample b)."""
    return torch.cat([t[:, l0:l0 + ln].reshape(-1, D) for l0, ln in levels], 0)


def _scatter(rows, batch, levels):
    out = torch.zeros(batch, N_LATENT, D, dtype=rows.dtype)
    r = 0
    for l0, ln in levels:
        out[:, l0:l0 + ln] = rows[r:r + batch * ln].reshape(batch, ln, D)
        r += batch * ln
    return out


def _per_group(rows, batch, levels, fn):
    outs, r = [], 0
    for gi, (_, ln) in enumerate(levels):
        outs.append(fn(rows[r:r + batch * ln], gi))
        r += batch * ln
    return torch.cat(outs, 0)


def _guarded(shape, fill):
    """A tensor of `shape` inside a buffer with GUARD sentinel floats on either side."""
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _linear(mode, a, y_act, out, w, bias, batch, levels, scatter=0, gathered=1):
    from where2edit_amd._lib import call, ptr, stream_ptr
    from where2edit_amd.mapper_hip import _int_array, _ptr_array
    g = len(levels)
    call("w2e_mapper_linear", mode, ptr(a), ptr(y_act), ptr(out), _ptr_array(w), _ptr_array(bias) if bias is not None else None, batch,
         N_LATENT, g, _int_array([lv[0] for lv in levels]), _int_array([lv[1] for lv in levels]), W_SCALE, B_SCALE, scatter, gathered,
         stream_ptr())
    torch.cuda.synchronize()


def _worst(got, ref, terms, what):
    """max over elements of |got - ref| / (GAMMA * terms): must be <= 1."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: an output element was not written"
    ratio = ((got - ref).abs() / (GAMMA * terms).clamp_min(1e-300)).max().item()
    print(f"{what}: worst |err| / (gamma * sum|terms|) = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} x the bound"
    return ratio


@pytest.fixture(scope="module")
def operands():
    """Per case: CPU inputs, their device copies and the float64 references -- computed once, read-only."""
    made = {}

    def make(name):
        if name in made:
            return made[name]
        batch, levels = CASES[name]
        g = len(levels)
        rows = batch * sum(ln for _, ln in levels)
        a = _heavy(f"mapk.{name}.a", (rows, D))
        w = [_heavy(f"mapk.{name}.w{i}", (D, D), 100.0 / 3.0) for i in range(g)]
        bias = [seeded.tensor(f"mapk.{name}.b{i}", (D,), std=30.0) for i in range(g)]
        gy_full = _heavy(f"mapk.{name}.gy", (batch, N_LATENT, D))
        y_full = _layer_output(f"mapk.{name}.y", (batch, N_LATENT, D))
        a64, w64, b64 = a.double(), [t.double() for t in w], [t.double() for t in bias]

        def fwd(use_bias):
            pre = _per_group(a64, batch, levels, lambda r, gi: W_SCALE * r @ w64[gi].T + (B_SCALE * b64[gi] if use_bias else 0.0))
            tot = _per_group(a64.abs(), batch, levels, lambda r, gi: W_SCALE * r @ w64[gi].abs().T + (B_SCALE * b64[gi].abs() if use_bias else 0.0))
            ref = torch.where(pre > 0, pre, pre * SLOPE) * GAIN
            slope = torch.where(pre < -GAMMA * tot, torch.full_like(pre, SLOPE), torch.ones_like(pre))
            return ref, tot * slope * GAIN

        gpre = _gather(gy_full, levels).double() * GAIN * torch.where(_gather(y_full, levels) > 0, 1.0, SLOPE).double()
        bwd = _per_group(gpre, batch, levels, lambda r, gi: W_SCALE * r @ w64[gi])
        bwd_terms = _per_group(gpre.abs(), batch, levels, lambda r, gi: W_SCALE * r @ w64[gi].abs())
        made[name] = dict(batch=batch, levels=levels, rows=rows, a=a.to(DEV), w=[t.to(DEV) for t in w], bias=[t.to(DEV) for t in bias],
                          gy_full=gy_full.to(DEV), y_full=y_full.to(DEV), gy_rows=_gather(gy_full, levels).contiguous().to(DEV),
                          y_rows=_gather(y_full, levels).contiguous().to(DEV), fwd={True: fwd(True), False: fwd(False)}, bwd=(bwd, bwd_terms))
        return made[name]

    return make


@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("scatter", [0, 1], ids=["grouped", "scattered"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_float64(operands, name, scatter, use_bias):
    c = operands(name)
    batch, levels = c["batch"], c["levels"]
    ref, terms = c["fwd"][use_bias]
    if scatter:  # latents outside every level are the caller's zeros: the kernel must leave them alone
        buf, out = _guarded((batch, N_LATENT, D), 0.0)
        covered = _scatter(torch.ones(c["rows"], D), batch, levels).bool()
        out[covered.to(DEV)] = float("nan")
        ref, terms = _scatter(ref, batch, levels), _scatter(terms, batch, levels)
    else:
        buf, out = _guarded((c["rows"], D), float("nan"))
    _linear(0, c["a"], None, out, c["w"], c["bias"] if use_bias else None, batch, levels, scatter=scatter)
    assert _guards_intact(buf), "wrote outside the output"
    if scatter:
        assert bool((out.cpu()[~covered] == 0).all()), "an uncovered latent of the scattered output was written"
        terms = torch.where(covered, terms, torch.ones_like(terms))
    _worst(out, ref, terms, f"forward {name} scatter={scatter} bias={use_bias}")
    again = torch.full_like(out, float("nan")) if not scatter else torch.where(covered.to(DEV), float("nan"), 0.0).float()
    _linear(0, c["a"], None, again, c["w"], c["bias"] if use_bias else None, batch, levels, scatter=scatter)
    assert torch.equal(out, again), "two calls on the same inputs differ"


@pytest.mark.parametrize("gathered", [1, 0], ids=["grouped", "ungathered"])
@pytest.mark.parametrize("name", list(CASES))
def test_input_gradient_matches_float64(operands, name, gathered):
    c = operands(name)
    batch, levels = c["batch"], c["levels"]
    ref, terms = c["bwd"]
    buf, out = _guarded((c["rows"], D), float("nan"))
    gy, y = (c["gy_rows"], c["y_rows"]) if gathered else (c["gy_full"], c["y_full"])
    _linear(1, gy, y, out, c["w"], None, batch, levels, gathered=gathered)
    assert _guards_intact(buf), "wrote outside the output"
    _worst(out, ref, terms, f"input gradient {name} gathered={gathered}")
    again = torch.full_like(out, float("nan"))
    _linear(1, gy, y, again, c["w"], None, batch, levels, gathered=gathered)
    assert torch.equal(out, again), "two calls on the same inputs differ"


@pytest.mark.parametrize("mode", [0, 1])
def test_more_rows_than_the_limit_are_refused_and_nothing_is_written(mode):
    batch, levels = 65, ((0, 18),)   # 1170 rows > MAP_MAXROWS = 1152
    rows = batch * 18
    a = torch.ones(rows, D, device=DEV)
    w = [torch.ones(D, D, device=DEV)]
    buf, out = _guarded((rows, D), 7.0)
    with pytest.raises(RuntimeError, match="bad groups"):
        _linear(mode, a, a if mode else None, out, w, None, batch, levels)
    torch.cuda.synchronize()
    assert _guards_intact(buf) and bool((out == 7.0).all())
