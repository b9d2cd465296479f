"""The FIR (upfirdn2d) dispatcher's decisions, checked on the host (no GPU: fir_plan is arithmetic on the scalar arguments, the
pointers' alignment and the options).

tests/golden/fir_plans.json holds what the dispatcher decided for a census of launches x option sets BEFORE the decision became a
function of its own (tests/golden/make_golden_fir_plans.py says how it was recorded); w2e_upfirdn2d_plan and
w2e_blur_adjoint_actbwd_plan must give the same answer, field by field and refusal by refusal, for every row.  The entries of
tests/test_gpu_fir_variants.py's matrix tie the plan to variant lines that were asserted on an MI355X."""
import ctypes
import json

import pytest

import make_golden_fir_plans as census
from test_gpu_fir_variants import ACTBWD_MATRIX, FIR_MATRIX, INSTANTIATIONS, covered_fir, fir_key, instantiation


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import build
    return ctypes.CDLL(build.build(verbose=False))


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(census.OUT))


@pytest.fixture(scope="module")
def planner(lib):
    return census.Planner(lib)


@pytest.fixture(scope="module")
def plans(planner, fixture):
    """({option set: [result per query]}, the same for the actbwd plan) of the library under test, over the fixture's own census."""
    queries, actbwd = [tuple(q) for q in fixture["queries"]], [tuple(q) for q in fixture["actbwd_queries"]]
    names = lambda sets: [n for n, _ in sets]
    return (dict(zip(names(fixture["options"]), census.ask(planner, fixture["options"], queries, planner.plan))),
            dict(zip(names(fixture["actbwd_options"]), census.ask(planner, fixture["actbwd_options"], actbwd, planner.actbwd))))


def planned(r):
    """A result that is a plan of a launch: not a refusal, not an empty launch."""
    f = census.FIELDS
    return len(r) == len(f) and r[f.index("grid")] > 0


def test_the_fixture_holds_the_census_the_script_enumerates(fixture):
    """Same queries, same option sets, same fields, one result per query: no row left out on either side; and the census reaches what
    it is there for."""
    queries, actbwd, (sets, actbwd_sets) = census.census()
    assert fixture["fields"] == list(census.FIELDS)
    assert [tuple(q) for q in fixture["queries"]] == queries and [tuple(q) for q in fixture["actbwd_queries"]] == actbwd
    assert [(n, o) for n, o in fixture["options"]] == sets and [(n, o) for n, o in fixture["actbwd_options"]] == actbwd_sets
    assert len(fixture["rows"]) == len(sets) and all(len(r) == len(queries) for r in fixture["rows"])
    assert len(fixture["actbwd_rows"]) == len(actbwd_sets) and all(len(r) == len(actbwd) for r in fixture["actbwd_rows"])
    assert len(queries) * len(sets) + len(actbwd) * len(actbwd_sets) >= 2000
    res = [fixture["results"][i] for row in fixture["rows"] for i in row]
    f = {name: i for i, name in enumerate(census.FIELDS)}
    have = {instantiation(census.KERNELS[r[f["kernel"]]], r[f["act"]], r[f["planar"]], 0) for r in res if planned(r)}
    assert have == INSTANTIATIONS - {("stream4", 0, 0, 1)}, have ^ INSTANTIATIONS
    messages = {r[1] for r in res if len(r) == 2}
    for fragment in census.REFUSALS:
        assert any(fragment in m for m in messages), fragment
    assert all(any(fragment in m for fragment in census.REFUSALS) for m in messages), messages
    assert any(len(r) == len(census.FIELDS) and r[f["grid"]] == 0 for r in res)
    default = fixture["actbwd_rows"][[n for n, _ in actbwd_sets].index("default")]
    assert set(default) == {0, 1}
    assert all(set(row) <= {0, 1} for row in fixture["actbwd_rows"])


def test_every_decision_is_the_recorded_one(fixture, plans):
    """Every field of every row; a refusal compares the return code and the message; the actbwd plan its answer."""
    fir, actbwd = plans
    bad = []
    for (name, _), row in zip(fixture["options"], fixture["rows"]):
        for query, idx, got in zip(fixture["queries"], row, fir[name]):
            if got != fixture["results"][idx]:
                bad.append(f"{name} {query}: recorded {fixture['results'][idx]}, now {got}")
    for (name, _), row in zip(fixture["actbwd_options"], fixture["actbwd_rows"]):
        bad += [f"actbwd {name} {q}: recorded {want}, now {got}" for q, want, got in zip(fixture["actbwd_queries"], row, actbwd[name]) if got != want]
    assert not bad, f"{len(bad)} rows differ, e.g.\n" + "\n".join(bad[:10])


def test_every_matrix_entry_plans_to_the_variant_it_was_written_for(planner):
    """FIR_MATRIX: the plan's (kernel, act, planar) under the entry's tune_blur is the entry's; ACTBWD_MATRIX: the fused pass is taken."""
    f = {name: i for i, name in enumerate(census.FIELDS)}
    bad = []
    try:
        for e in FIR_MATRIX:
            planner.set_options(dict(census.DEFAULT_OPTIONS, tune_blur=str(e["tune_blur"])))
            r = planner.plan(census.matrix_query(e))
            got = (census.KERNELS[r[f["kernel"]]], r[f["act"]], r[f["planar"]]) if planned(r) else r
            if got != (e["kernel"], e["act"], e["planar"]):
                bad.append(f"{e}: planned {got}")
        planner.set_options(census.DEFAULT_OPTIONS)
        bad += [f"actbwd {m}: not fused" for m in ACTBWD_MATRIX if planner.actbwd((m[0][0] * m[0][1], m[1], m[2], 4, 4)) != 1]
    finally:
        planner.set_options(census.DEFAULT_OPTIONS)
    assert not bad, "\n".join(bad)


def test_planar_ok_is_the_launchers_rule(fixture, planner, plans):
    """Over the census: w2e_upfirdn2d_planar_ok is 1 exactly where the launcher does not refuse in_layout = 1 (with this library's
    pitch) for the layout."""
    names = ("planes", "in_h", "in_w", "out_h", "out_w", "kh", "kw", "up", "down", "pad_x0", "planar", "pitch")  # a query's leading fields
    checked = {0: 0, 1: 0}
    for query, r in zip(fixture["queries"], plans[0]["default"]):
        q = dict(zip(names, query))
        if q["planar"] != 1 or q["pitch"] != census.planar_pitch((q["in_w"] - 1) >> 1) or (len(r) != 2 and not planned(r)):
            continue
        if len(r) == 2 and not any(fragment in r[1] for fragment in (census.LAYOUT_REFUSAL, "tensor too large")):
            continue  # refused before the layout is looked at (a bad size, a tap count, up / down)
        accepted = not (len(r) == 2 and census.LAYOUT_REFUSAL in r[1])
        ok = planner.planar_ok(q["kh"], q["kw"], q["up"], q["down"], q["out_w"])
        assert ok == int(accepted), (query, r)
        checked[ok] += 1
    assert checked[0] >= 100 and checked[1] >= 100, checked


def test_every_planned_variant_is_in_the_gpu_matrix(fixture, plans):
    """What fir_plan can produce, tests/test_gpu_fir_variants.py runs: the census key of every planned row is in covered_fir().  Left
    out, and never a key that a generator or discriminator row produces:
      * sweep and golden rows of a form -- (taps, up, down, act) -- that no generator or discriminator row launches: the synthetic tap
        shapes and up / down pairs of the boundary sweep (tests/test_gpu_parity.py runs the golden cases against the reference's outputs);
      * SIZE_FALLBACKS: the generic kernel where a 4x4 launch is past down4's limits of 2^29 input floats / 2^31 outputs."""
    SIZE_FALLBACKS = {fir_key("generic", 0, 0, 0, 1, 2, 4, 4, 4096), fir_key("generic", 0, 0, 0, 1, 1, 4, 4, 16)}
    origins = census.fir_census()
    f = {name: i for i, name in enumerate(census.FIELDS)}
    covered = covered_fir()
    form = lambda q: (q[5], q[6], q[7], q[8], q[12])
    launched = {form(q) for origin, q in origins if origin in ("generator", "discriminator")}
    misses, left_out, real, checked = {}, set(SIZE_FALLBACKS), set(), 0
    for name, _ in fixture["options"]:
        for (origin, q), r in zip(origins, plans[0][name]):
            if not planned(r):
                continue
            key = fir_key(census.KERNELS[r[f["kernel"]]], r[f["act"]], r[f["planar"]], 0, q[7], q[8], q[5], q[6], q[4])
            if origin in ("generator", "discriminator"):
                real.add(key)
            if origin in ("sweep", "golden") and form(q) not in launched:
                left_out.add(key)
                continue
            if origin == "limits" and key in SIZE_FALLBACKS:
                continue
            checked += 1
            if key not in covered:
                misses.setdefault(key, f"{key}, planned for {q} ({origin}) under {name}")
    assert checked >= 2000
    assert not (left_out - covered) & real, (left_out - covered) & real
    assert not misses, "\n".join(misses.values())
