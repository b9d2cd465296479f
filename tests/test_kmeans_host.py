"""Offline k-means (where2edit_amd.clustering_feature.kmeans / fit_clusters), the part that needs no GPU: the float64
restatement the GPU tests compare against (tests/kmeans_ref.py) reproduces the scikit-learn fixture (tests/golden/kmeans.npz,
make_golden_kmeans.py), argument errors are raised before any kernel, and the new entry points are declared.  Also the conditions
on the seeded inputs of tests/test_gpu_kmeans_kernels.py (tests/mask_ref.py: KMEANS_SHAPES, kmeans_step_case)."""
import pytest
import torch

import kmeans_ref as R
import mask_ref as M
from helpers import golden, rel_err


def test_float64_helper_reproduces_the_scikit_learn_fixture():
    g = golden("kmeans")
    X = R.fixture_matrix()
    assert tuple(X.shape) == (4096, 72)
    cen, lab, inertia, _ = R.kmeans(X, R.K, 10, torch.Generator().manual_seed(0))
    print(f"helper inertia {inertia:.6f}, fixture {float(g['inertia']):.6f}")
    assert abs(inertia - float(g["inertia"])) <= 1e-6 * float(g["inertia"])
    perm = R.match(cen, g["centres"])
    assert rel_err(cen[perm], g["centres"]) <= 1e-5
    # the helper's labelling of the FIXTURE's centres against scikit-learn's own labels: the cap the GPU test holds `assign` to
    hl, _, gap = R.nearest(X, g["centres"])
    differ = int((hl.numpy() != g["labels"]).sum())
    print(f"helper vs scikit-learn labels: {differ} of {len(hl)} differ; smallest relative gap of the two best distances {float(gap.min()):.3e}")
    assert differ <= 0.001 * len(hl)
    assert torch.equal(torch.bincount(hl, minlength=R.K), torch.from_numpy(g["counts"]))


def test_single_forgy_starts_miss_the_optimum_that_ten_plusplus_starts_reach():
    """Why the seeding and the restarts: K distinct random points as the start end above the optimum for some seeds."""
    g = golden("kmeans")
    X = R.fixture_matrix()
    ratios = []
    for seed in range(8):
        idx = torch.multinomial(torch.ones(X.shape[0]), R.K, generator=torch.Generator().manual_seed(seed))
        ratios.append(R.lloyd(X, X[idx])[2] / float(g["inertia"]))
    print("single Forgy start, inertia / optimum over seeds 0-7:", " ".join(f"{r:.3f}" for r in ratios))
    assert min(ratios) >= 1 - 1e-6 and max(ratios) > 1.2


def test_argument_errors_are_raised_without_a_gpu():
    from where2edit_amd import clustering_feature as CF
    pts = torch.zeros(2, 16, 4, 4)
    with pytest.raises(ValueError, match="n_clusters <= 32"):
        CF.kmeans(pts, 33)
    with pytest.raises(ValueError, match="n_init must be 1"):
        CF.kmeans(pts, 3, init=torch.zeros(3, 18), n_init=10)
    with pytest.raises(ValueError, match="empty chunk list"):
        CF.kmeans([], 3)
    with pytest.raises(ValueError, match="init is"):
        CF.kmeans(pts, 3, init="forgy")
    with pytest.raises(ValueError, match="chunks disagree"):
        CF.kmeans([pts, torch.zeros(1, 32, 4, 4)], 3)
    with pytest.raises(ValueError, match="n_clusters <= 32"):
        CF.fit_clusters(None, attention_layer=7, clusters=40)
    with pytest.raises(ValueError, match="steps and batch"):
        CF.fit_clusters(None, steps=0, attention_layer=7, clusters=6)
    with pytest.raises(ValueError, match="attention_layer counts from 1"):
        CF.fit_clusters(None, attention_layer=0, clusters=6)
    from where2edit_amd import build
    build.build(verbose=False)  # (the next check needs the library: without it the loader's "not found" error comes first)
    with pytest.raises(RuntimeError, match="GPU only"):  # and no CPU path behind it
        CF.kmeans(pts, 3, n_init=1)


# ---- conditions on the seeded inputs of tests/test_gpu_kmeans_kernels.py, checked on the reference alone
def test_kmeans_case_lists_hold_what_the_gpu_tests_rely_on():
    assert all(shape in M.KMEANS_SHAPES for shape in M.ASSIGN_SHAPES + M.KMEANS_STEP_SHAPES)
    assert len(set(M.KMEANS_SHAPES)) == len(M.KMEANS_SHAPES)
    # the fused step's cases are exactly the listed shapes that the fused step takes
    assert [shape for shape in M.KMEANS_SHAPES if M.kmeans_step_fits(*shape[:4])] == [s for s in M.KMEANS_SHAPES if s in M.KMEANS_STEP_SHAPES]
    assert {M.kmeans_kp(k) for _, _, _, k, _ in M.KMEANS_STEP_SHAPES} == {8, 16, 24, 32}
    # (tiles per image, tiles, live pixels of the last tile): the figures of the case comments
    assert M.kmeans_tiles(10, 3) == (1, 3, 100)
    assert M.kmeans_tiles(14, 1) == (2, 2, 68)   # 196 pixels: 68 in the second tile, 68 - 64 = 4 live lanes in its upper half
    assert M.kmeans_tiles(12, 5) == (2, 10, 16)  # 144 pixels: 16 in the second tile
    assert M.kmeans_tiles(6, 2) == (1, 2, 36) and M.kmeans_tiles(2, 1) == (1, 1, 4)
    assert M.kmeans_tiles(16, 2) == (2, 4, 128) and M.kmeans_tiles(64, 1) == (32, 32, 128)
    assert any(c % 16 for c, *_ in M.KMEANS_STEP_SHAPES) and any(c % 4 for c, *_ in M.KMEANS_STEP_SHAPES) and any(c < 4 for c, *_ in M.KMEANS_STEP_SHAPES)
    assert any(c + 2 * p > 512 for c, p, *_ in M.KMEANS_STEP_SHAPES) and any(p == 0 for _, p, *_ in M.KMEANS_STEP_SHAPES)


def test_wide_cases_need_the_three_block_form_and_fit_it():
    """The LDS arithmetic of csrc/kmeans.hip's mode 0 restated: more than 160 KB with six blocks of partial distances, within with three."""
    floats = lambda d, kp, blocks: d * kp + blocks * 64 * kp + M.KMEANS_TILE + 2 * kp  # noqa: E731
    for c, p, _, k, _ in M.KMEANS_WIDE_SHAPES + [(960, 32, 8, 32, 1)]:
        d, kp = c + 2 * p, M.kmeans_kp(k)
        assert 4 * floats(d, kp, 6) > 160 * 1024 >= 4 * floats(d, kp, 3), (c, p, k)
    assert {M.kmeans_kp(k) for _, _, _, k, _ in M.KMEANS_WIDE_SHAPES} == {8, 16, 32}
    for c, p, s, k, b in M.KMEANS_WIDE_SHAPES:
        per, tiles, last = M.kmeans_tiles(s, b)
        # both halves of a tile and the reuse of the blocks from tile to tile: several tiles per workgroup at grid 1 and 3, a full tile,
        # and a last tile whose upper half has live and dead lanes
        assert per >= 2 and tiles > 3 and 64 < last < M.KMEANS_TILE, (s, b)
        assert 4 * (c + 2 * p + 256) * (8 if k <= 8 else 16 if k <= 16 else 32) <= 160 * 1024  # w2e_cluster_assign takes it
    assert all(4 * floats(c + 2 * p, M.kmeans_kp(k), 6) <= 160 * 1024 for c, p, _, k, _ in M.KMEANS_SHAPES if c != 960)
    # the refusals of tests/test_gpu_kmeans_kernels.py: beyond three blocks at KP = 32; beyond six at KP = 24, which has no other form
    assert 4 * floats(1100, 32, 3) > 160 * 1024 and 4 * floats(1400, M.kmeans_kp(20), 6) > 160 * 1024


@pytest.mark.parametrize("c,p,s,k,b", M.KMEANS_SHAPES + M.KMEANS_WIDE_SHAPES)
def test_kmeans_cases_have_few_near_ties(c, p, s, k, b):
    """tests/test_mask_ref_host.py's test_assignment_cases_have_few_near_ties over KMEANS_SHAPES: the gap rule excludes at most 1 % of a
    case's pixels."""
    feat, cen = M.assign_case(c, p, s, k, b)
    dist, ids = M.assign_ref(feat.double(), cen.double(), p)
    _, gap = M.assign_margins(dist)
    excluded = int((gap <= M.ASSIGN_GAP).sum())
    print(f"kmeans case {(c, p, s, k, b)}: {excluded} of {gap.numel()} pixels within {M.ASSIGN_GAP:g} of a tie; smallest gap {float(gap.min()):.3e}; "
          f"{len(ids.unique())} of {k} clusters used")
    assert excluded <= M.ASSIGN_MAX_TIES * gap.numel()


@pytest.mark.parametrize("c,p,s,k,b", M.KMEANS_STEP_SHAPES)
def test_step_labellings_hold_an_empty_cluster_a_long_run_and_an_alternation(c, p, s, k, b):
    """What the float64 argmin of kmeans_step_case is, not what the labelling was meant to be: no near-ties, cluster K - 1 empty, per
    image a run longer than a tile (where the image has more than one) and a stretch where the id changes at every pixel."""
    feat, cen, lab = M.kmeans_step_case(c, p, s, k, b)
    dist, ids = M.assign_ref(feat.double(), cen.double(), p)
    _, gap = M.assign_margins(dist)
    assert int((gap <= M.ASSIGN_GAP).sum()) <= M.ASSIGN_MAX_TIES * gap.numel()
    per, _, _ = M.kmeans_tiles(s, b)
    runs = [M.longest_run(i.reshape(-1)) for i in ids]
    alts = [M.longest_alternation(i.reshape(-1)) for i in ids]
    print(f"step case {(c, p, s, k, b)}: {int((ids != lab).sum())} ids differ from the labelling; longest run per image {runs}, longest "
          f"alternation {alts}; {len(ids.unique())} of {k} clusters used")
    assert torch.equal(ids, lab)
    if k > 1:
        assert not bool((ids == k - 1).any()) and len(ids.unique()) == min(k - 1, len(lab.unique()))
    if per > 1:
        assert min(runs) > M.KMEANS_TILE
    if k > 2:
        assert min(alts) >= M.kmeans_step_run(s)[1]  # 32 pixels, or what the run leaves of a small image (14 of 144)
    if k == 1:
        assert min(runs) == s * s


def test_step_labellings_between_them_hold_every_feature():
    """At least one fused-step case has an empty cluster, one a run longer than a tile, one an alternation of 32 pixels."""
    labs = [(k, M.kmeans_step_labelling(s, k, b).reshape(b, -1)) for _, _, s, k, b in M.KMEANS_STEP_SHAPES]
    assert sum(k > 1 and not bool((lab == k - 1).any()) for k, lab in labs) >= 5
    assert sum(min(M.longest_run(i) for i in lab) > M.KMEANS_TILE for _, lab in labs) >= 4
    assert sum(min(M.longest_alternation(i) for i in lab) >= 32 for _, lab in labs) >= 4


def test_kmeans_entry_points_are_declared():
    import ctypes
    import os
    from where2edit_amd import _lib, build
    names = ("w2e_kmeans_plan", "w2e_kmeans_pass", "w2e_kmeans_reduce")
    header = open(os.path.join(os.path.dirname(build.PKG), "include", "w2e_attention.h")).read()
    lib = ctypes.CDLL(build.build(verbose=False))
    for n in names:
        assert n in _lib._PROTOS and f"int {n}(" in header and hasattr(lib, n)
    # argument validation happens before any HIP call
    lib.w2e_last_error.restype = ctypes.c_char_p
    res, args = _lib._PROTOS["w2e_kmeans_pass"]
    lib.w2e_kmeans_pass.restype, lib.w2e_kmeans_pass.argtypes = res, args
    d = ctypes.c_void_p(4096)
    assert lib.w2e_kmeans_pass(0, d, d, None, None, None, 0, d, 8, 1, 64, 4, 32, 33, None) != 0 and b"clusters <= 32" in lib.w2e_last_error()
    assert lib.w2e_kmeans_pass(2, d, d, None, None, None, 0, d, 8, 1, 64, 4, 32, 9, None) != 0 and b"clusters <= 8" in lib.w2e_last_error()
    assert lib.w2e_kmeans_pass(1, d, d, None, None, None, 0, d, 8, 1, 64, 4, 33, 6, None) != 0 and b"even size" in lib.w2e_last_error()
    assert lib.w2e_kmeans_pass(1, d, d, None, None, None, 0, d, 8, 1, 512, 32, 128, 32, None) != 0 and b"of LDS" in lib.w2e_last_error()
    assert lib.w2e_kmeans_pass(1, ctypes.c_void_p(4100), d, None, None, None, 0, d, 8, 1, 64, 4, 32, 6, None) != 0 and b"16-byte aligned" in lib.w2e_last_error()
