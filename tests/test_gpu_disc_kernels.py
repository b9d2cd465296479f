"""The entry points of csrc/disc.hip (K8) and the finish half of csrc/wgrad.hip, one by one through the C ABI against the float64
restatement of tests/disc_ref.py (held to float64 autograd by tests/test_disc_ref_host.py): w2e_fromrgb_fwd / _bwd / _jvp,
w2e_mbstd_fwd / _bwd / _jvp / _hvp, w2e_sumsq_rows (+ _parts), w2e_modconv_wgrad_finish on hand-made slabs, w2e_modconv_wsq.

How the error is judged: EVERY element, |got - ref| <= K * 2^-24 * T, no element excluded and no norm over a tensor.  T is the element's
own term scale in float64 (disc_ref.*: the formula on absolute values; for the stddev kernels the scales that carry the conditioning
of (x - mean) / sd), K the number of fp32 roundings on the longest chain of the kernel source, counted beside each constant in
tests/disc_ref.py.  An element whose scale is 0 must be exact.

Inputs: the suite's heavy-tailed family and, for the stddev kernels, a family whose group members are well apart.  Every output and
workspace is pre-filled with NaN (7.0 where a call must refuse) between 64 sentinels on either side that must survive; every input sits
between sentinels; what a call has no business reading is NaN.  Every call is made twice and the two results must have equal bits.
`-s` prints the worst error / bound of every comparison; the last test prints the table DESIGN.md quotes.  A census of what the
Discriminator, its R1 penalty and one decoder fine-tuning backward really call is held against COVERAGE."""
import math

import pytest
import torch

import disc_ref as R
from test_gpu_gen_small_kernels import GUARD, SENTINEL, Buf, _stop_after_a_gpu_fault, inp  # noqa: F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U
WORST = {}         # what -> (error / bound, error in roundings of T, K)
EXERCISED = set()  # call_key of every call this file's tests made
NAN = float("nan")
RGB_SCALE = R.f32scale(1.0 / math.sqrt(3.0))   # EqualConv2d(3, C, 1): 1 / sqrt(fan_in), as the C ABI receives it

BWD_COMBOS = ["gx", "gx+part", "gx+part+dw", "gx+part+db", "gx+part+dw+db", "part+dw", "part+db", "part+dw+db"]
SUMSQ_CASES = [(b, n) for b in R.SUMSQ_BATCHES for n in R.SUMSQ_LENGTHS] + [(4, 3 * 32 * 32)]   # + the 32^2 image at batch 4 (the census)
DISC_ENTRY_POINTS = ["w2e_fromrgb_fwd", "w2e_fromrgb_bwd", "w2e_fromrgb_jvp", "w2e_mbstd_fwd", "w2e_mbstd_bwd", "w2e_mbstd_jvp",
                     "w2e_mbstd_hvp", "w2e_sumsq_rows"]


# ---------------------------------------------------------------------------------------------- the key of a call, and the table
def _addr(p):
    v = getattr(p, "value", p)
    return 0 if v is None else int(v)


def _int(v):
    return int(getattr(v, "value", v))


def _ops(**named):
    return "+".join(k for k, p in named.items() if _addr(p)) or "-"


def call_key(name, args):
    """(entry point, batch, C, hw, optional-operand pattern) of a call of csrc/disc.hip; for the finish kernel (entry point, taps,
    operand form) and for w2e_modconv_wsq (entry point, taps): their element loops do not depend on the sizes beyond the ragged
    cases FINISH_DIMS / WSQ_DIMS hold.  None for any other entry point."""
    if name == "w2e_fromrgb_fwd":
        return (name, _int(args[4]), _int(args[5]), _int(args[6]), _ops(bias=args[2]))
    if name == "w2e_fromrgb_bwd":
        return (name, _int(args[8]), _int(args[9]), _int(args[10]), _ops(gx=args[4], part=args[5], dw=args[6], db=args[7]))
    if name == "w2e_fromrgb_jvp":
        return (name, _int(args[4]), _int(args[5]), _int(args[6]), "-")
    if name == "w2e_mbstd_fwd":
        return (name, _int(args[2]), _int(args[3]), _int(args[4]), "-")
    if name in ("w2e_mbstd_bwd", "w2e_mbstd_jvp"):
        return (name, _int(args[3]), _int(args[4]), _int(args[5]), "-")
    if name == "w2e_mbstd_hvp":
        return (name, _int(args[4]), _int(args[5]), _int(args[6]), "-")
    if name == "w2e_sumsq_rows":
        return (name, _int(args[3]), 1, _int(args[4]), "-")
    if name == "w2e_modconv_wgrad_finish":
        sums, dz, nw, bias, d = args[3:8]
        if not _addr(d):
            form = "none"
        elif _addr(dz):
            form = "dz"
        else:
            form = "sums" + ("_nw" if _addr(nw) else "") + ("_bias" if _addr(bias) else "")
        return (name, _int(args[13]), form)
    if name == "w2e_modconv_wsq":
        return (name, _int(args[4]))
    return None


COVERAGE = {}   # call_key -> the test of this file that makes exactly this call
for _name, ((_b, _c, _hw), _) in R.FROMRGB_CASES.items():
    COVERAGE.update({("w2e_fromrgb_fwd", _b, _c, _hw, o): "test_fromrgb_forward" for o in ("bias", "-")})
    COVERAGE.update({("w2e_fromrgb_bwd", _b, _c, _hw, o): "test_fromrgb_backward" for o in BWD_COMBOS})
    COVERAGE[("w2e_fromrgb_jvp", _b, _c, _hw, "-")] = "test_fromrgb_tangent"
for _b in R.MBSTD_BATCHES:
    for _c, _hw in R.MBSTD_SHAPES:
        COVERAGE.update({(f"w2e_mbstd_{k}", _b, _c, _hw, "-"): f"test_mbstd_{t}"
                         for k, t in (("fwd", "forward"), ("bwd", "backward"), ("jvp", "tangent"), ("hvp", "hessian_vector_product"))})
COVERAGE.update({("w2e_sumsq_rows", _b, 1, _n, "-"): "test_sumsq_rows" for _b, _n in SUMSQ_CASES})
COVERAGE.update({("w2e_modconv_wgrad_finish", t, f): "test_wgrad_finish" for t in R.FINISH_TAPS for f in R.FINISH_FORMS})
COVERAGE.update({("w2e_modconv_wsq", t): "test_modconv_wsq" for t in R.FINISH_TAPS})


# ---------------------------------------------------------------------------------------------- calling and judging
def _lib():
    from where2edit_amd import _lib as L
    return L


def kcall(name, *args):
    L = _lib()
    L.call(name, *args, L.stream_ptr())
    torch.cuda.synchronize()
    EXERCISED.add(call_key(name, args))  # (after the call: a refused call exercises nothing)


def P(b):
    """The device pointer of a Buf (or NULL for None)."""
    return None if b is None else _lib().ptr(b.v)


def nan_buf(shape):
    """An operand a call must not use: all NaN between the sentinels."""
    return Buf(shape=shape)


def judge(got, ref, scale, k, what, quiet=False):
    """Every element of `got` within k (a number or a tensor) fp32 roundings of float64 relative to ITS OWN scale; an element whose
    scale is 0 must be exact.  Returns error / bound of the worst element."""
    got = got.detach().double().cpu()
    ref, scale = R.f64(ref).reshape(got.shape), R.f64(scale).reshape(got.shape)
    k = (R.f64(k) if torch.is_tensor(k) else torch.tensor(float(k), dtype=torch.float64)).expand(got.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written (NaN left) or not finite"
    assert got.numel() == 0 or float(got.abs().max()) < 1e-10 * SENTINEL, f"{what}: a sentinel was read"
    share = (got - ref).abs() / (k * U * scale).clamp_min(1e-300)
    i = int(share.argmax())
    s, n = float(share.reshape(-1)[i]), float(k.reshape(-1)[i])
    key = what.split(" [")[0]
    if s >= WORST.get(key, (-1.0, 0.0, 0.0))[0]:
        WORST[key] = (s, s * n, n)
    if not quiet:
        print(f"{what}: worst element {s * n:.3f} x 2^-24 of its scale (K = {n:g}): error / bound = {s:.4f}")
    assert s <= 1.0, f"{what}: element {i} is {s * n:.3f} x 2^-24 of its scale from float64 (K = {n:g})"
    return s


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def twice(run):
    """Run a call twice on fresh outputs: the two results (lists of Buf) must have equal bits and intact sentinels; -> the first."""
    first, second = run(), run()
    for a, b in zip(first, second):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.intact() and b.intact(), "wrote outside an output"
            assert same_bits(a.v, b.v), "two calls on the same inputs differ"
    return first


# ---------------------------------------------------------------------------------------------- fromRGB
@pytest.fixture(scope="module")
def fr_case():
    """Per case: the CPU inputs, their guarded device copies and (lazily) the float64 references -- made once, read-only."""
    made = {}

    def make(name):
        if name not in made:
            (b, c, hw), _ = R.FROMRGB_CASES[name]
            key = f"disc_kernels.fr.{name}"
            cpu = dict(x=R.heavy(key + ".x", (b, 3, hw)), w=R.heavy(key + ".w", (c, 3)), bias=R.heavy(key + ".b", (c,)),
                       gy=R.heavy(key + ".gy", (b, c, hw)), y=R.layer_output(key + ".y", (b, c, hw)), dx=R.heavy(key + ".dx", (b, 3, hw)))
            made[name] = dict(b=b, c=c, hw=hw, cpu=cpu, dev={k: inp(t) for k, t in cpu.items()}, refs={})
        return made[name]

    return make


def _inputs_intact(case):
    return all(buf.intact() for buf in case["dev"].values())


@pytest.mark.parametrize("bias", ["bias", "-"])
@pytest.mark.parametrize("name", list(R.FROMRGB_CASES))
def test_fromrgb_forward(fr_case, name, bias):
    """w2e_fromrgb_fwd, bias given and NULL: K = FROMRGB_FWD_K = 8 (disc_ref.py), T = sqrt2 * (scale |w| |x| + |bias|), times 0.2 where
    the pre-activation is safely negative.  capped_c2 walks a second pixel per thread; model_b3 / model_b4 are C = FR_MAX_C."""
    case = fr_case(name)
    b, c, hw, d, cpu = case["b"], case["c"], case["hw"], case["dev"], case["cpu"]
    ref, t = R.fromrgb_fwd(cpu["x"], cpu["w"], cpu["bias"] if bias == "bias" else None, RGB_SCALE)

    def run():
        y = Buf(shape=(b, c, hw))
        kcall("w2e_fromrgb_fwd", P(d["x"]), P(d["w"]), P(d["bias"]) if bias == "bias" else None, P(y), b, c, hw, RGB_SCALE)
        return [y]

    (y,) = twice(run)
    assert _inputs_intact(case)
    judge(y.v, ref, t, R.FROMRGB_FWD_K, f"w2e_fromrgb_fwd [{name} {bias}]")


def _bwd_refs(case):
    if "bwd" not in case["refs"]:
        cpu = case["cpu"]
        case["refs"]["bwd"] = R.fromrgb_bwd(cpu["gy"], cpu["y"], cpu["x"], cpu["w"], RGB_SCALE)
    return case["refs"]["bwd"]


@pytest.mark.parametrize("name", list(R.FROMRGB_CASES))
def test_fromrgb_backward(fr_case, name):
    """w2e_fromrgb_bwd in every legal combination of gx / part / dw / db, the slope masks from a saved y that holds 0 and -0.0 (both on
    the 0.2 side).  K (disc_ref.py): gx C + 5, dw 25 + ceil(rows / 256), db 23 + ceil(rows / 256).  Without dw and db the partials
    are not formed: `part` stays as it was and x -- read into registers but used by nothing -- is all NaN.  What was not asked for is
    not written; gx, dw and db have the same bits whatever else was asked for."""
    case = fr_case(name)
    b, c, hw, d = case["b"], case["c"], case["hw"], case["dev"]
    rows = R.fromrgb_rows(b, hw)
    assert rows == _lib().load().w2e_fromrgb_bwd_rows(b, hw)
    (rx, rw, rb), (sx, sw, sb) = _bwd_refs(case)
    x_nan = nan_buf((b, 3, hw))
    seen = {}
    for combo in BWD_COMBOS:
        want = combo.split("+")
        formed = "dw" in want or "db" in want

        def run():
            out = dict(gx=Buf(shape=(b, 3, hw)), part=Buf(shape=(rows, c, 4)), dw=Buf(shape=(c, 3)), db=Buf(shape=(c,)))
            kcall("w2e_fromrgb_bwd", P(d["gy"]), P(d["y"]), P(d["x"] if formed else x_nan), P(d["w"]),
                  *[P(out[k]) if k in want else None for k in ("gx", "part", "dw", "db")], b, c, hw, RGB_SCALE)
            for k in ("gx", "dw", "db"):
                assert k in want or out[k].untouched(), f"{combo}: {k} was written though not asked for"
            if formed:
                assert out["part"].intact() and bool(torch.isfinite(out["part"].v).all()), f"{combo}: a partial row was left unwritten"
            else:
                assert out["part"].untouched(), f"{combo}: the partials were written though neither dw nor db was asked for"
            return [out[k] if k in want else None for k in ("gx", "dw", "db")]

        gx, dw, db = twice(run)
        assert _inputs_intact(case) and x_nan.untouched()
        for k, buf, ref, scale, bound in (("gx", gx, rx, sx, R.fromrgb_gx_k(c)), ("dw", dw, rw, sw, R.fromrgb_dw_k(rows)),
                                          ("db", db, rb, sb, R.fromrgb_db_k(rows))):
            if buf is None:
                continue
            if k in seen:
                assert same_bits(seen[k].v, buf.v), f"{k} depends on what else was asked for ({combo})"
            else:
                seen[k] = buf
                judge(buf.v, ref, scale, bound, f"w2e_fromrgb_bwd {k} [{name} {combo}]")
    assert set(seen) == {"gx", "dw", "db"}


@pytest.mark.parametrize("name", list(R.FROMRGB_CASES))
def test_fromrgb_tangent(fr_case, name):
    """w2e_fromrgb_jvp: K = FROMRGB_JVP_K = 7, T = sqrt2 * slope(y) * scale |w| |dx|; no bias enters."""
    case = fr_case(name)
    b, c, hw, d, cpu = case["b"], case["c"], case["hw"], case["dev"], case["cpu"]
    ref, t = R.fromrgb_jvp(cpu["dx"], cpu["y"], cpu["w"], RGB_SCALE)

    def run():
        out = Buf(shape=(b, c, hw))
        kcall("w2e_fromrgb_jvp", P(d["dx"]), P(d["y"]), P(d["w"]), P(out), b, c, hw, RGB_SCALE)
        return [out]

    (out,) = twice(run)
    assert _inputs_intact(case)
    judge(out.v, ref, t, R.FROMRGB_JVP_K, f"w2e_fromrgb_jvp [{name}]")


def test_fromrgb_refusals_write_nothing():
    """C = 513 and hw = 0 for all three entry points; dw or db without the partials; a `part` that is not 16-byte aligned; and the two
    calls that have nothing to do (gx NULL without dw and db, with and without `part`), which return 0 and write nothing."""
    c, hw = 8, 16
    a = Buf(torch.ones(4 * 513 * 16))
    outs = {k: Buf(shape=(4 * 513 * 16 + 4,), fill=7.0) for k in ("y", "gx", "part", "dw", "db")}
    before = set(EXERCISED)

    def untouched():
        torch.cuda.synchronize()
        return all(o.intact() and bool((o.v == 7.0).all()) for o in outs.values())

    for b_, c_, hw_ in R.FROMRGB_REFUSED:
        with pytest.raises(RuntimeError, match="fromrgb_fwd: bad dims"):
            kcall("w2e_fromrgb_fwd", P(a), P(a), P(a), P(outs["y"]), b_, c_, hw_, RGB_SCALE)
        with pytest.raises(RuntimeError, match="fromrgb_jvp: bad dims"):
            kcall("w2e_fromrgb_jvp", P(a), P(a), P(a), P(outs["y"]), b_, c_, hw_, RGB_SCALE)
        with pytest.raises(RuntimeError, match="fromrgb_bwd: bad dims"):
            kcall("w2e_fromrgb_bwd", P(a), P(a), P(a), P(a), P(outs["gx"]), P(outs["part"]), P(outs["dw"]), P(outs["db"]), b_, c_, hw_, RGB_SCALE)
    for dw, db in ((outs["dw"], None), (None, outs["db"]), (outs["dw"], outs["db"])):
        with pytest.raises(RuntimeError, match="need the partials workspace"):
            kcall("w2e_fromrgb_bwd", P(a), P(a), P(a), P(a), P(outs["gx"]), None, P(dw), P(db), 1, c, hw, RGB_SCALE)
    L = _lib()
    off = outs["part"].v[1:]   # 4 bytes past a 16-byte boundary
    assert off.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        L.call("w2e_fromrgb_bwd", P(a), P(a), P(a), P(a), P(outs["gx"]), L.ptr(off), P(outs["dw"]), None, 1, c, hw, RGB_SCALE, L.stream_ptr())
    assert untouched() and EXERCISED == before
    L.call("w2e_fromrgb_bwd", P(a), P(a), P(a), P(a), None, None, None, None, 1, c, hw, RGB_SCALE, L.stream_ptr())
    L.call("w2e_fromrgb_bwd", P(a), P(a), P(a), P(a), None, P(outs["part"]), None, None, 1, c, hw, RGB_SCALE, L.stream_ptr())
    assert untouched()


# ---------------------------------------------------------------------------------------------- the minibatch stddev layer
MB_CASES = [(b, c, hw, fam) for b in R.MBSTD_BATCHES for (c, hw) in R.MBSTD_SHAPES for fam in R.FAMILIES]
MB_IDS = [f"B{b}_{c}x{hw}_{fam}" for b, c, hw, fam in MB_CASES]


@pytest.fixture(scope="module")
def mb_case():
    made = {}

    def make(b, c, hw, fam):
        key = (b, c, hw, fam)
        if key not in made:
            x, dx, gy = R.mbstd_inputs(fam, b, c, hw)
            gs = gy.clone()
            gs[:, :c] = 0.0                 # the stddev channel's cotangent alone
            gn = gy.clone()
            gn[:, :c] = NAN                 # ... with the identity channels poisoned (mbstd_hvp must not read them)
            made[key] = dict(group=R.mbstd_group(b), x=x, dx=dx, gy=gy, gs=gs, scales=R.mbstd_scales(x, gy, dx),
                             dev=dict(x=inp(x), dx=inp(dx), gy=inp(gy), gs=inp(gs), gn=inp(gn)))
        return made[key]

    return make


def _per_sample(v, group, hw):
    """[M] -> [B, hw]: the value of group m at every pixel of every sample b = g * M + m."""
    return v.repeat(group).view(-1, 1).expand(-1, hw)


@pytest.mark.parametrize("b,c,hw,fam", MB_CASES, ids=MB_IDS)
def test_mbstd_forward(mb_case, b, c, hw, fam):
    """w2e_mbstd_fwd: the C identity channels are a bit copy; every pixel of the stddev channel is within K = mbstd_s_k roundings of
    T = mean_e A_e + s log2 n.  At group 1 (batch 1) x - mean is exactly 0 and s must be within that bound of sqrt(1e-8)."""
    m = mb_case(b, c, hw, fam)
    d = m["dev"]

    def run():
        y = Buf(shape=(b, c + 1, hw))
        kcall("w2e_mbstd_fwd", P(d["x"]), P(y), b, c, hw)
        return [y]

    (y,) = twice(run)
    assert d["x"].intact() and same_bits(y.v[:, :c], d["x"].v), "the identity channels are not a bit copy of x"
    s = R.mbstd_value(m["x"])
    if m["group"] == 1:
        assert abs(float(s[0]) - 1e-4) < 1e-12
    judge(y.v[:, c], _per_sample(s, m["group"], hw), _per_sample(m["scales"]["s"], m["group"], hw), R.mbstd_s_k(m["group"], c, hw),
          f"w2e_mbstd_fwd s [B{b} {c}x{hw} {fam}]")


@pytest.mark.parametrize("b,c,hw,fam", MB_CASES, ids=MB_IDS)
def test_mbstd_backward(mb_case, b, c, hw, fam):
    """w2e_mbstd_bwd.  With the identity cotangent 0 the output is the stddev part alone: K = mbstd_gx_k = E + 2, T = ceff amp_e (1 + cs) with ceff = |coef| + (Dg / K) cabs (disc_ref.mbstd_scales); at
    group 1 it is exactly 0.  With the full cotangent: T + |gy|, one more rounding (the final addition)."""
    m = mb_case(b, c, hw, fam)
    d, group = m["dev"], m["group"]
    full, part = R.mbstd_bwd(m["gy"], m["x"])
    k = R.mbstd_gx_k(group, c, hw)
    for which, ref, scale, kk in (("gs", part, m["scales"]["gx"], k), ("gy", full, m["scales"]["gx"] + m["gy"][:, :c].double().abs(), k + 1)):
        def run():
            gx = Buf(shape=(b, c, hw))
            kcall("w2e_mbstd_bwd", P(d[which]), P(d["x"]), P(gx), b, c, hw)
            return [gx]

        (gx,) = twice(run)
        assert d["x"].intact() and d[which].intact()
        judge(gx.v, ref, scale, kk, f"w2e_mbstd_bwd {'stddev part' if which == 'gs' else 'gx'} [B{b} {c}x{hw} {fam}]")
        if group == 1:
            want = torch.zeros_like(gx.v) if which == "gs" else d["gy"].v[:, :c]
            assert bool((gx.v == want).all()), "group 1: the stddev part must be exactly 0"


@pytest.mark.parametrize("b,c,hw,fam", MB_CASES, ids=MB_IDS)
def test_mbstd_tangent(mb_case, b, c, hw, fam):
    """w2e_mbstd_jvp: the identity channels are a bit copy of dx; the stddev channel's tangent within K = mbstd_jv_k roundings of
    T = mean_e[amp_e D_e (1 + max_g cs)] + |jv| log2 n; exactly 0 at group 1."""
    m = mb_case(b, c, hw, fam)
    d, group = m["dev"], m["group"]

    def run():
        y = Buf(shape=(b, c + 1, hw))
        kcall("w2e_mbstd_jvp", P(d["x"]), P(d["dx"]), P(y), b, c, hw)
        return [y]

    (y,) = twice(run)
    assert d["x"].intact() and d["dx"].intact() and same_bits(y.v[:, :c], d["dx"].v), "the identity channels are not a bit copy of dx"
    judge(y.v[:, c], _per_sample(R.mbstd_jvp(m["x"], m["dx"]), group, hw), _per_sample(m["scales"]["jv"], group, hw),
          R.mbstd_jv_k(group, c, hw), f"w2e_mbstd_jvp tangent [B{b} {c}x{hw} {fam}]")
    if group == 1:
        assert bool((y.v[:, c] == 0).all()), "group 1: the tangent of the stddev channel must be exactly 0"


@pytest.mark.parametrize("b,c,hw,fam", MB_CASES, ids=MB_IDS)
def test_mbstd_hessian_vector_product(mb_case, b, c, hw, fam):
    """w2e_mbstd_hvp with the C identity channels of gy all NaN (only the stddev channel is read): K = mbstd_mu_k,
    T = (ceff / sd_e) amp_e D_e (1 + cs)(1 + max_g cs), ceff = |coef| + (Dg / K) cabs; exactly 0 at group 1."""
    m = mb_case(b, c, hw, fam)
    d, group = m["dev"], m["group"]

    def run():
        mu = Buf(shape=(b, c, hw))
        kcall("w2e_mbstd_hvp", P(d["gn"]), P(d["x"]), P(d["dx"]), P(mu), b, c, hw)
        return [mu]

    (mu,) = twice(run)
    assert d["x"].intact() and d["dx"].intact() and d["gn"].intact()
    judge(mu.v, R.mbstd_hvp(m["gy"], m["x"], m["dx"]), m["scales"]["mu"], R.mbstd_mu_k(group, c, hw), f"w2e_mbstd_hvp mu [B{b} {c}x{hw} {fam}]")
    if group == 1:
        assert bool((mu.v == 0).all()), "group 1: mu must be exactly 0"


@pytest.mark.parametrize("b", R.MBSTD_REFUSED)
def test_mbstd_refuses_a_batch_that_is_no_multiple_of_its_group(b):
    c, hw = 3, 5
    a = Buf(torch.ones(b * (c + 1) * hw))
    out = Buf(shape=(b * (c + 1) * hw,), fill=7.0)
    before = set(EXERCISED)
    for name, args in (("w2e_mbstd_fwd", (P(a), P(out))), ("w2e_mbstd_bwd", (P(a), P(a), P(out))), ("w2e_mbstd_jvp", (P(a), P(a), P(out))),
                       ("w2e_mbstd_hvp", (P(a), P(a), P(a), P(out)))):
        with pytest.raises(RuntimeError, match="multiple of the stddev group"):
            kcall(name, *args, b, c, hw)
    torch.cuda.synchronize()
    assert out.intact() and bool((out.v == 7.0).all()) and EXERCISED == before


# ---------------------------------------------------------------------------------------------- sumsq_rows
@pytest.mark.parametrize("b,n", SUMSQ_CASES, ids=[f"b{b}_n{n}" for b, n in SUMSQ_CASES])
def test_sumsq_rows(b, n):
    """w2e_sumsq_rows: K = sumsq_k(n) = 34 + ceil(chunks / 256) roundings of the sum itself (every term is positive).  Lengths around
    SQ_CHUNK = 4096, and 4096 * 256 + 5: 257 chunks, the finish loop's second stride."""
    x = R.heavy(f"disc_kernels.sumsq.{b}.{n}", (b, n))
    xd = inp(x)
    chunks = _lib().load().w2e_sumsq_rows_parts(n)
    assert chunks == R.sumsq_parts(n)

    def run():
        part, out = Buf(shape=(b, chunks)), Buf(shape=(b,))
        kcall("w2e_sumsq_rows", P(xd), P(part), P(out), b, n)
        assert bool(torch.isfinite(part.v).all())
        return [out, part]

    out, _ = twice(run)
    assert xd.intact()
    ref = R.sumsq(x)
    judge(out.v, ref, ref, R.sumsq_k(n), f"w2e_sumsq_rows [b{b} n{n}]")


def test_sumsq_rows_parts_is_the_formula():
    lib = _lib().load()
    for n in (-5, 0, 1, 4095, 4096, 4097, 4096 * 256 + 5, R.SQ_CHUNK * 65535 - 1, R.SQ_CHUNK * 65535, R.SQ_CHUNK * 65535 + 1, 2 ** 40):
        assert lib.w2e_sumsq_rows_parts(n) == R.sumsq_parts(n), n
    assert lib.w2e_sumsq_rows_parts(0) == 0 and lib.w2e_sumsq_rows_parts(R.SQ_CHUNK * 65535) == 0
    x, out = Buf(torch.ones(8)), Buf(shape=(8,), fill=7.0)
    with pytest.raises(RuntimeError, match="row too long"):
        kcall("w2e_sumsq_rows", P(x), P(out), P(out), 1, R.SQ_CHUNK * 65535)
    assert out.intact() and bool((out.v == 7.0).all())


# ---------------------------------------------------------------------------------------------- the weight-gradient finish
def _finish_operands(form, taps, cout, cin, batch, splits):
    key = f"disc_kernels.finish.{form}.{taps}.{cout}.{cin}.{batch}.{splits}"
    cpu = dict(slab=R.heavy(key + ".slab", (splits, taps, cout, cin)), weight=R.heavy(key + ".w", (cout, cin, taps)),
               sums=R.heavy(key + ".sums", (batch, cout, 3)), dz=R.heavy(key + ".dz", (batch, cout)),
               nw=R.heavy(key + ".nw", (1,)) + 0.5, bias=R.heavy(key + ".bias", (cout,)),
               d=torch.rand((batch, cout), generator=R._gen(key + ".d")) + 0.5, s=R.heavy(key + ".s", (batch, cin)))
    return cpu


@pytest.mark.parametrize("taps", R.FINISH_TAPS)
@pytest.mark.parametrize("form", R.FINISH_FORMS)
def test_wgrad_finish(form, taps):
    """w2e_modconv_wgrad_finish on hand-made slabs (no wgrad launch), splits x (cout, cin) x batch of disc_ref.FINISH_*: the
    [split][tap][o][i] -> [o][i][tap] transpose, the wave-interleaved split sum and the demodulation term.
      none  d = NULL: the slab sum alone, K = finish_slab_k(splits) of T = scale * sum_k |slab|; every other operand is given and all NaN.
      dz / sums*  slab + term: K = max(slab K, finish_demod_k) + 1 of the two term scales added; then the same call on an all-zero
            slab: the demodulation term alone, K = finish_demod_k of T = scale^2 |W| sum_b |dz| d^2 s^2 (|dz| of the sums form: the three
            terms on absolute values).  With dz given, noise_w and bias are given too and all NaN."""
    worst = {}
    for cout, cin in R.FINISH_DIMS:
        scale = R.f32scale(1.0 / math.sqrt(cin * taps))
        for batch in R.FINISH_BATCHES:
            for splits in R.FINISH_SPLITS:
                cpu = _finish_operands(form, taps, cout, cin, batch, splits)
                dev = {k: inp(t) for k, t in cpu.items()}
                poison = {k: nan_buf(t.shape) for k, t in cpu.items()}
                zero = inp(torch.zeros_like(cpu["slab"]))
                if form == "none":
                    ops = [poison["weight"], poison["sums"], poison["dz"], poison["nw"], poison["bias"], None, poison["s"]]
                    dzv = dzs = None
                else:
                    sums_form = form != "dz"
                    ops = [dev["weight"], dev["sums"] if sums_form else None, None if sums_form else dev["dz"],
                           dev["nw"] if "nw" in form else (None if sums_form else poison["nw"]),
                           dev["bias"] if "bias" in form else (None if sums_form else poison["bias"]), dev["d"], dev["s"]]
                    dzv, dzs = R.finish_dz(form, cpu["sums"], cpu["dz"], float(cpu["nw"][0]), cpu["bias"])
                what = f"taps {taps} {cout}x{cin} batch {batch} splits {splits}"
                for slab_name in (["slab"] if form == "none" else ["slab", "zero"]):
                    slab = dev["slab"] if slab_name == "slab" else zero
                    slab_cpu = cpu["slab"] if slab_name == "slab" else torch.zeros_like(cpu["slab"])

                    def run():
                        dw = Buf(shape=(cout, cin, taps))
                        kcall("w2e_modconv_wgrad_finish", P(slab), splits, *[P(o) for o in ops], P(dw), batch, cin, cout, taps, scale)
                        return [dw]

                    (dw,) = twice(run)
                    assert slab.intact() and all(o is None or o.intact() for o in ops), "wrote outside dW"
                    a, m = R.finish(slab_cpu, cpu["weight"], dzv, cpu["d"], cpu["s"], scale)
                    sa, sm = R.finish(slab_cpu.abs(), cpu["weight"].abs(), dzs, cpu["d"], cpu["s"], scale)
                    if form == "none":
                        k, tag = R.finish_slab_k(splits), "slab sum alone"
                    elif slab_name == "zero":
                        k, tag = R.finish_demod_k(form, batch), "demodulation term alone"
                    else:
                        k, tag = max(R.finish_slab_k(splits), R.finish_demod_k(form, batch)) + 1, "slab + demodulation term"
                    r = judge(dw.v, a + m, sa + sm.abs(), k, f"w2e_modconv_wgrad_finish {tag} ({form}) [{what}]", quiet=True)
                    if r >= worst.get(tag, (-1.0,))[0]:
                        worst[tag] = (r, r * k, k, what)
    for tag, (r, rk, k, what) in worst.items():
        print(f"w2e_modconv_wgrad_finish {tag} ({form}, taps {taps}): worst element {rk:.3f} x 2^-24 of its scale (K = {k:g}) at {what}: "
              f"error / bound = {r:.4f}")


def test_wgrad_finish_refusals_write_nothing():
    """With d given: both of sums / dz, neither, weight missing, s missing; and taps = 4 in any form."""
    batch, cin, cout, taps = 2, 7, 3, 9
    a = Buf(torch.ones(4096))
    dw = Buf(shape=(cout * cin * taps,), fill=7.0)
    before = set(EXERCISED)

    def call(weight, sums, dz, d, s, taps_=taps):
        kcall("w2e_modconv_wgrad_finish", P(a), 2, weight, sums, dz, None, None, d, s, P(dw), batch, cin, cout, taps_, 0.5)

    with pytest.raises(RuntimeError, match="exactly one of sums / dz"):
        call(P(a), P(a), P(a), P(a), P(a))
    with pytest.raises(RuntimeError, match="exactly one of sums / dz"):
        call(P(a), None, None, P(a), P(a))
    with pytest.raises(RuntimeError, match="needs weight and s"):
        call(None, P(a), None, P(a), P(a))
    with pytest.raises(RuntimeError, match="needs weight and s"):
        call(P(a), None, P(a), P(a), None)
    for d in (None, P(a)):
        with pytest.raises(RuntimeError, match="bad dims"):
            call(P(a), P(a), None, d, P(a), taps_=4)
    torch.cuda.synchronize()
    assert dw.intact() and bool((dw.v == 7.0).all()) and EXERCISED == before


@pytest.mark.parametrize("cout,cin", R.WSQ_DIMS)
@pytest.mark.parametrize("taps", R.FINISH_TAPS)
def test_modconv_wsq(taps, cout, cin):
    """w2e_modconv_wsq: K = taps + 2 roundings of the sum itself (every term is positive); scale = 0.37."""
    w = R.heavy(f"disc_kernels.wsq.{taps}.{cout}.{cin}", (cout, cin, taps))
    wd = inp(w)
    scale = R.f32scale(0.37)

    def run():
        out = Buf(shape=(cout, cin))
        kcall("w2e_modconv_wsq", P(wd), P(out), cout, cin, taps, scale)
        return [out]

    (out,) = twice(run)
    assert wd.intact()
    ref = R.wsq(w, scale)
    judge(out.v, ref, ref, R.wsq_k(taps), f"w2e_modconv_wsq [taps {taps} {cout}x{cin}]")


# ---------------------------------------------------------------------------------------------- the census
def _recorder(seen, sizes=None):
    """`seen`: call_key -> count.  `sizes`: for the finish kernel (batch, cin, cout, splits) and for w2e_modconv_wsq (cout, cin) of
    every recorded call, per key -- printed, so that the sizes behind a (taps, form) row can be read from the log."""
    real = _lib().call

    def recording(name, *args):
        key = call_key(name, args)
        if key is not None:
            seen[key] = seen.get(key, 0) + 1
            if sizes is not None and name == "w2e_modconv_wgrad_finish":
                sizes.setdefault(key, set()).add((_int(args[10]), _int(args[11]), _int(args[12]), _int(args[1])))
            if sizes is not None and name == "w2e_modconv_wsq":
                sizes.setdefault(key, set()).add((_int(args[2]), _int(args[3])))
        return real(name, *args)

    return recording


def _report(seen, sizes=None):
    for key in sorted(seen, key=str):
        print(f"census: {seen[key]:3d} x {key}  <- {COVERAGE.get(key, 'NOT COVERED')}")
    for key in sorted(sizes or {}, key=str):
        what = "(batch, cin, cout, splits)" if key[0] == "w2e_modconv_wgrad_finish" else "(cout, cin)"
        print(f"census: {key} was called with {what} = {sorted(sizes[key])}")
    missing = sorted((k for k in seen if k not in COVERAGE), key=str)
    assert not missing, f"calls in a shape / operand pattern no test of this file makes: {missing}"


@pytest.mark.parametrize("batch", [3, 4])
def test_census_of_the_discriminator_and_its_r1_penalty(monkeypatch, batch):
    """One Discriminator forward + backward and one r1_penalty forward + backward at 32^2 with every call of disc_hip recorded:
    every (entry point, batch, C, hw, operand pattern) is a COVERAGE row, and every launching entry point of csrc/disc.hip was seen."""
    import disc64
    import where2edit_amd.disc_hip as DH
    import where2edit_amd.functional as KF
    from test_gpu_discriminator import _disc
    seen, sizes = {}, {}
    monkeypatch.setattr(DH, "call", _recorder(seen, sizes))
    monkeypatch.setattr(KF, "call", _recorder(seen, sizes))
    d = _disc(32, disc64.state_dict(32, salt=9))
    x = disc64.images(batch, 32, salt=9).to(DEV)
    d(x).sum().backward()
    DH.r1_penalty(d, x).backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in d.parameters())
    _report(seen, sizes)
    assert {k[0] for k in seen} == set(DISC_ENTRY_POINTS) | {"w2e_modconv_wgrad_finish"}, "an entry point the Discriminator never called"
    assert {k[1:] for k in seen if k[0] == "w2e_modconv_wgrad_finish"} == {(1, "none"), (9, "none")}


def test_census_of_one_decoder_fine_tuning_backward(monkeypatch):
    """Generator(64) with every conv weight trained, one forward + backward: the operand forms of the finish kernel and the taps of
    w2e_modconv_wsq it really uses are COVERAGE rows."""
    import seeded
    import where2edit_amd.functional as KF
    from test_gpu_conv_wgrad import _generator
    seen, sizes = {}, {}
    monkeypatch.setattr(KF, "call", _recorder(seen, sizes))
    g = _generator(64, seeded.generator_state_dict(64))
    w = seeded.wplus_latents(2, g.n_latent, salt=91).to(DEV)
    img, _ = g([w], input_is_latent=True, randomize_noise=False)
    img.square().sum().backward()
    torch.cuda.synchronize()
    _report(seen, sizes)
    assert {k[0] for k in seen} == {"w2e_modconv_wgrad_finish", "w2e_modconv_wsq"}
    assert any(k[2] != "none" for k in seen if k[0] == "w2e_modconv_wgrad_finish"), "no demodulated layer was trained"


def test_zz_every_coverage_row_was_exercised_and_worst_ratios(request):
    """After the tests above (file order): the table of worst error / bound per output, and -- when the whole file ran -- every COVERAGE
    row was really called by this file's tests, which called nothing else."""
    for key in sorted(WORST):
        share, ratio, k = WORST[key]
        print(f"worst: {ratio:9.3f} x 2^-24 of T, K = {k:<7g} error / bound = {share:.4f}  {key}")
    whole_file = not request.config.getoption("keyword") and not any("::" in a for a in request.config.args)
    if whole_file:
        assert sorted(set(COVERAGE) - EXERCISED, key=str) == [], "COVERAGE rows no test of this file exercised"
        assert sorted(EXERCISED - set(COVERAGE), key=str) == [], "calls of this file's tests that COVERAGE does not list"
