"""The 3x3 conv dispatcher's decisions, checked on the host (no GPU: conv_plan is arithmetic on the mode, the shape and the options).

tests/golden/conv_plans.json holds what the dispatcher decided for a census of shapes x option sets BEFORE the decision became a
function of its own (tests/golden/make_golden_conv_plans.py says how it was recorded); w2e_conv3x3_plan must give the same answer,
field by field and refusal by refusal, for every row.  The cost model's `* 0.995` tie-break makes the choice sensitive to the order of
floating-point operations, so "the refactor changed no decision" is shown exhaustively here rather than argued."""
import ctypes
import json

import pytest

import make_golden_conv_plans as census
from test_gpu_conv_variants import DIRECT_MATRIX, covered_direct


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import build
    return ctypes.CDLL(build.build(verbose=False))


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(census.OUT))


@pytest.fixture(scope="module")
def plans(lib, fixture):
    """{option set: [result per shape]} of the library under test, over the fixture's own census (options restored afterwards)."""
    planner = census.Planner(lib)
    shapes = [tuple(s) for s in fixture["shapes"]]
    out = {}
    try:
        for name, options in fixture["options"]:
            planner.set_options(options)
            out[name] = [planner.plan(s) for s in shapes]
    finally:
        planner.set_options(census.DEFAULT_OPTIONS)
    return out


def test_the_fixture_holds_the_census_the_script_enumerates(fixture):
    """Same shapes, same option sets, same fields, one result per query: no row left out on either side."""
    shapes, sets = census.census()
    assert fixture["fields"] == list(census.FIELDS)
    assert [tuple(s) for s in fixture["shapes"]] == shapes and len(shapes) >= 200
    assert [(n, o) for n, o in fixture["options"]] == sets
    assert len(fixture["rows"]) == len(sets) and all(len(r) == len(shapes) for r in fixture["rows"])
    assert len(shapes) * len(sets) >= 3000
    # the census does reach the corners it is there for: refusals, split-K, both pipelines, bf16x3, both UP forms
    res = [fixture["results"][i] for row in fixture["rows"] for i in row]
    ok = [r for r in res if len(r) == len(census.FIELDS)]
    f = {name: i for i, name in enumerate(census.FIELDS)}
    assert len(ok) < len(res)
    for what in ("use_all", "use_dma", "use_x3", "border_wgs"):
        assert any(r[f[what]] for r in ok) and any(not r[f[what]] for r in ok), what
    assert any(r[f["splits"]] > 1 for r in ok) and {r[f["cfg"]] for r in ok} == set(range(12))


def test_every_decision_is_the_recorded_one(fixture, plans):
    """Every field of every row; a refusal compares the return code and the message."""
    bad = []
    for (name, _), row in zip(fixture["options"], fixture["rows"]):
        for shape, idx, got in zip(fixture["shapes"], row, plans[name]):
            want = fixture["results"][idx]
            if got != want:
                bad.append(f"{name} {shape}: recorded {want}, now {got}")
    assert not bad, f"{len(bad)} rows differ, e.g.\n" + "\n".join(bad[:10])


def test_the_recorded_bench_selections_are_reproduced(plans):
    """profiles/r05_bench_cfg_selections.txt: the plan reproduces the tile, whether K is split and the pipeline of every recorded
    launch.  (The record has no epilogue: a SAME / DOWN launch matches with or without the bias / PReLU epilogue.)"""
    shapes, _ = census.census()
    at = {s: i for i, s in enumerate(shapes)}
    f = {name: i for i, name in enumerate(census.FIELDS)}
    rec = census.bench_selections()
    assert len(rec) >= 100
    misses = []
    for mode, k, n, h, w, b, cfg, split, dma in rec:
        got = [plans["default"][at[(mode, b, k, n, h, w, prelu, 0)]] for prelu in ((0,) if mode == census.UP else (0, 1))]
        if not any(len(r) == len(census.FIELDS) and (r[f["cfg"]], r[f["splits"]] > 1, bool(r[f["use_dma"]])) == (cfg, split, dma) for r in got):
            misses.append(f"mode {mode} K {k} N {n} {h}x{w} B {b}: recorded cfg {cfg} split {split} dma {dma}, planned {got}")
    assert not misses, "\n".join(misses)


def test_every_planned_variant_is_in_the_matrix_of_the_gpu_tests(fixture, plans):
    """What conv_plan can produce, tests/test_gpu_conv_variants.py runs: (mode, all-phase, tile, split, dma, x3) of every row that was not
    refused is in its matrix, keyed without the epilogue.  A variant outside it is a tile whose instantiation mask and tile_fits
    disagree, or an untested one.  Left out: the conv_precision = bf16x3 set (that matrix has no bf16x3 case: tests/test_gpu_parity.py
    runs those), and forced-tile rows whose tile the matrix does not list for the mode."""
    covered = {key[:6] for key in covered_direct()}
    tiles = {(mode, all_phase): set(t) for mode, all_phase, t, *_ in DIRECT_MATRIX.values()}
    f = {name: i for i, name in enumerate(census.FIELDS)}
    misses, checked = {}, 0
    for name, options in fixture["options"]:
        if options["conv_precision"] != "f32":
            continue
        for shape, r in zip(fixture["shapes"], plans[name]):
            if len(r) != len(census.FIELDS) or r[f["grid"]] == 0:  # refused, or an empty batch
                continue
            key = (shape[0], r[f["use_all"]], r[f["cfg"]], r[f["splits"]] > 1, r[f["use_dma"]], r[f["use_x3"]])
            if options["tune_cfg"] and key[2] not in tiles[key[:2]]:
                continue
            checked += 1
            if key not in covered:
                misses.setdefault(key, f"{key} (mode, all-phase, cfg, split, dma, x3), planned for {shape} under {name}")
    assert checked >= 3000
    assert not misses, "\n".join(misses.values())
