"""Which form a stride-1 3x3 conv takes, checked on the host (no GPU: w2e_wino_plan is arithmetic on its arguments and two options).

tests/golden/wino_forms.json holds what the Python policies decided -- functional._wino_form, irse_hip._wino_form and the shape
predicates under them -- for a census of 13,440 shapes x 48 (family, request, option set) groups BEFORE the decision moved into the
library, and what w2e_wino_gemm_plan plus functional.wino_gemm_conv's forced-split arithmetic gave for the GEMM form
(tests/golden/make_golden_wino_forms.py says how it was recorded).  w2e_wino_plan must give the same answer for every row."""
import ctypes

import pytest

import make_golden_wino_forms as census


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import build
    return ctypes.CDLL(build.build(verbose=False))


@pytest.fixture(scope="module")
def fixture():
    return census.load()


@pytest.fixture(scope="module")
def query(lib):
    q = census.Query(lib)
    yield q
    q.set_options(census.DEFAULT_OPTIONS)


def test_the_fixture_holds_the_census_the_script_enumerates(fixture):
    """Same grid, one character per decision, and the census reaches every form for every family: all zeros cannot pass."""
    assert (fixture["batches"], fixture["channels"], fixture["sizes"]) == (list(census.BATCHES), list(census.CHANNELS), [list(s) for s in census.SIZES])
    assert fixture["forced_splits"] == list(census.FORCED_SPLITS)
    shapes, groups = census.shapes(), census.groups()
    assert len(shapes) == 13440 and len(groups) == 48 and sorted(fixture["forms"]) == sorted(g[0] for g in groups)
    forms = {key: fixture["strings"][i] for key, i in fixture["forms"].items()}
    assert all(len(s) == len(shapes) and set(s) <= set("048") for s in forms.values())
    for flags in (fixture["fits_gemm"], fixture["fits_fused"]):
        assert sorted(flags) == sorted(v[0] for v in census.VARIANTS)
        assert all(len(fixture["strings"][i]) == len(shapes) and set(fixture["strings"][i]) == set("01") for i in flags.values())
    count = lambda variant, request, digit: sum(forms[f"{variant}/{request}/{o[0]}"].count(digit) for o in census.OPTION_SETS)
    assert (count("generator", "auto", "4"), count("generator", "auto", "8")) == (920, 276)  # of 40,320 each
    assert (count("encoder", "auto", "4"), count("encoder", "auto", "8")) == (1675, 612)
    for variant in ("generator", "generator_dot", "encoder"):
        assert min(count(variant, "auto", "4"), count(variant, "auto", "8"), count(variant, "4", "4"), count(variant, "8", "8")) >= 250, variant
    assert count("encoder_no_fused", "auto", "4") >= 1675 and count("encoder_no_fused", "4", "4") >= 1675
    # a request is never answered with the other form, a bf16x3 / forced-tile library and "direct" never with any, no switch -> no fused
    assert all(set(forms[g[0]]) <= {"direct": {"0"}, "4": {"0", "4"}, "8": {"0", "8"}, "auto": set("048")}[g[2][0]] for g in groups)
    assert all(set(forms[g[0]]) == {"0"} for g in groups if g[3][0] != "f32")
    assert all("8" not in forms[g[0]] for g in groups if g[1][0] == "encoder_no_fused")
    assert len(fixture["gemm_plans"]) == fixture["strings"][fixture["fits_gemm"]["encoder"]].count("1") >= 4000
    assert any(row[1] > 1 for row in fixture["gemm_plans"]) and any(row[1] == 1 for row in fixture["gemm_plans"])


def test_every_decision_is_the_recorded_one(fixture, query):
    """Form and both fit flags of all 645,120 rows, under the library's real options."""
    shapes, bad, rows = census.shapes(), [], 0
    for key, variant, (_, request), (_, options, _) in census.groups():
        query.set_options(options)
        want = zip(fixture["strings"][fixture["forms"][key]], fixture["strings"][fixture["fits_gemm"][variant[0]]],
                   fixture["strings"][fixture["fits_fused"][variant[0]]])
        for shape, (form, fits_gemm, fits_fused) in zip(shapes, want):
            got = query.plan(variant, request, shape)
            rows += 1
            if got[:3] != [int(form), int(fits_gemm), int(fits_fused)]:
                bad.append(f"{key} {shape}: recorded form {form} fits {fits_gemm} {fits_fused}, now {got[:3]}")
    assert rows == 645120
    assert not bad, f"{len(bad)} rows differ, e.g.\n" + "\n".join(bad[:10])


def test_the_gemm_forms_tiles_split_and_workspace_are_the_recorded_ones(fixture, query):
    """tiles_padded, splits and workspace_floats wherever the GEMM form fits -- the library's own split and forced ones (the tests' knob
    functional.GEMM_SPLITS) --, identical for every family, request and epilogue that the form fits, and zero where it does not."""
    query.set_options(census.DEFAULT_OPTIONS)
    shapes = census.shapes()
    fits = {v[0]: fixture["strings"][fixture["fits_gemm"][v[0]]] for v in census.VARIANTS}
    plans = iter(fixture["gemm_plans"])
    bad = []
    for i, shape in enumerate(shapes):
        if fits["encoder"][i] == "0":
            assert query.plan(census.VARIANTS[2], 4, shape)[3:] == [0, 0, 0], shape
            continue
        row = next(plans)
        for j, forced in enumerate(census.FORCED_SPLITS):
            want = [row[0], row[1 + 2 * j], row[2 + 2 * j]]
            for variant in census.VARIANTS[:3]:
                got = query.plan(variant, 4 if forced else -1, shape, forced)[3:]
                if got != (want if fits[variant[0]][i] == "1" else [0, 0, 0]):
                    bad.append(f"{variant[0]} {shape} forced {forced}: recorded {want}, now {got}")
    assert next(plans, None) is None
    assert not bad, f"{len(bad)} plans differ, e.g.\n" + "\n".join(bad[:10])


def test_bad_arguments_are_refused_with_a_message(lib, query):
    ok = (0, -1, 1, 0, 8, 512, 512, 64, 64, 0)
    out = (ctypes.c_int64 * len(census.FIELDS))()
    assert lib.w2e_wino_plan(*ok, out) == 0 and list(out) == [4, 1, 0, 2048, 1, 8 * 512 * 8]
    for index, value in ((0, 2), (1, 2), (1, 5), (3, 4), (3, -1), (4, -1), (9, -1)):  # family, request, epilogue, batch, forced splits
        args = list(ok)
        args[index] = value
        assert lib.w2e_wino_plan(*args, out) != 0 and lib.w2e_last_error().startswith(b"wino_plan:"), args
    assert lib.w2e_wino_plan(*ok, None) != 0
    # an empty batch, dimensions no kernel takes and sizes past every int product: direct, nothing fits, no arithmetic on them
    for shape in ((0, 64, 64, 32, 32), (8, 0, 64, 32, 32), (8, 64, 0, 32, 32), (8, 64, 64, 0, 0), (8, 64, 64, -4, 32),
                  (2 ** 31 - 1,) * 5, (2 ** 31 - 1, 256, 2 ** 31 - 64, 2 ** 31 - 16, 2 ** 31 - 32), (1, 8, 64, 2 ** 31 - 1, 4)):
        for variant in census.VARIANTS:
            assert query.plan(variant, -1, shape, 16) == [0] * 6, shape
