"""Offline k-means (where2edit_amd.clustering_feature.kmeans / fit_clusters), the part that needs no GPU: the float64
restatement the GPU tests compare against (tests/kmeans_ref.py) reproduces the scikit-learn fixture (tests/golden/kmeans.npz,
make_golden_kmeans.py), argument errors are raised before any kernel, and the new entry points are declared."""
import pytest
import torch

import kmeans_ref as R
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
