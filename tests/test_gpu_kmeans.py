"""Offline k-means on the HIP kernels (where2edit_amd.clustering_feature.kmeans / fit_clusters; csrc/kmeans.hip) against the
float64 restatement of tests/kmeans_ref.py and the scikit-learn fixture tests/golden/kmeans.npz (make_golden_kmeans.py)."""
import numpy as np
import pytest
import torch

import kmeans_ref as R
import seeded
from helpers import assert_close, golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fixture():
    from where2edit_amd import clustering_feature as CF
    pts = R.fixture_points(DEV)
    X = CF.points_matrix(pts).double().cpu()
    assert tuple(pts.shape) == (4, 64, 32, 32) and tuple(X.shape) == (4096, 72)
    assert rel_err(X, R.fixture_matrix()) <= 1e-6  # the device's bilinear up-sampling against the host's
    return CF, pts, X


def test_seeding_picks_the_float64_helpers_points():
    """Greedy k-means++ on the GPU with the helper's draws: the same K indices, the same running minimum distances.  The draws
    keep 1e-4 (relative) away from every step of the CDF they are looked up in, so a reordered fp32 sum cannot move an index."""
    CF, pts, X = _fixture()
    for seed in (0, 1, 2):
        idx, mind, draws, margin = R.plusplus(X, R.K, generator=torch.Generator().manual_seed(seed), min_margin=1e-4)
        assert margin > 1e-4, margin
        centres, gpu_idx, gpu_mind = CF.kmeans_plusplus(pts, R.K, draws=draws)
        print(f"seed {seed}: helper {idx}, gpu {gpu_idx}, margin {margin:.3e}, mind rel err {rel_err(gpu_mind, mind):.3e}")
        assert gpu_idx == idx
        assert_close(gpu_mind, mind, 1e-5, "mind after seeding")
        assert_close(centres, X[idx], 1e-6, "seeded centres")
    # the chunked walk sees the same points under the same indices
    _, chunk_idx, chunk_mind = CF.kmeans_plusplus(list(pts.split(1)), R.K, draws=draws)
    assert chunk_idx == idx and rel_err(chunk_mind, mind) <= 1e-5


def test_fit_reaches_the_scikit_learn_fixture():
    CF, pts, X = _fixture()
    g = golden("kmeans")
    res = CF.kmeans(pts, R.K, n_init=10, generator=0)
    print(f"inertia {res.inertia:.4f} (fixture {float(g['inertia']):.4f}), restarts {[round(v, 2) for v in res.inertias]}, n_iter {res.n_iter}")
    assert abs(res.inertia - float(g["inertia"])) <= 1e-5 * float(g["inertia"])
    assert len(res.inertias) == 10 and res.inertia == min(res.inertias) and res.empty_clusters == 0
    perm = R.match(res.centres.cpu(), g["centres"])
    assert_close(res.centres.cpu()[perm], g["centres"], 1e-4, "centres")
    assert torch.equal(res.counts.cpu()[perm], torch.from_numpy(g["counts"]))
    assert res.assign.dtype == torch.int32 and tuple(res.assign.shape) == (4, 32, 32)
    lab, _, gap = R.nearest(X, res.centres.cpu())
    near_tie = gap < 1e-5
    differ = lab != res.assign.cpu().long().reshape(-1)
    print(f"assign: {int(differ.sum())} of {len(lab)} differ from the float64 labelling, {int(near_tie.sum())} near-ties")
    assert int(near_tie.sum()) <= 0.001 * len(lab) and not bool((differ & ~near_tie).any())
    assert torch.equal(torch.bincount(res.assign.cpu().long().reshape(-1), minlength=R.K), res.counts.cpu())
    assert torch.equal(CF.predict(pts, res.centres), res.assign)
    assert abs(CF.inertia(pts, res.centres) - res.inertia) <= 1e-6 * res.inertia
    # init="random" and an explicit init run too
    one = CF.kmeans(pts, R.K, init=g["centres"].float(), max_iter=5)
    assert len(one.inertias) == 1 and abs(one.inertia - float(g["inertia"])) <= 1e-5 * float(g["inertia"])
    rnd = CF.kmeans(pts, R.K, init="random", n_init=2, generator=3)
    assert len(rnd.inertias) == 2 and rnd.inertia >= float(g["inertia"]) * (1 - 1e-5)


def test_one_lloyd_step_is_right_deterministic_and_chunking_independent():
    CF, pts, X = _fixture()
    init = X[torch.tensor([5, 700, 1500, 2300, 3100, 3900])].float()
    sums_ref, counts_ref, inertia_ref = R.lloyd_step(X, init)
    sums, counts, inertia = CF.lloyd_step(pts, init.to(DEV), fused=True)
    print(f"step: sums rel err {rel_err(sums, sums_ref):.3e}, inertia rel err {abs(inertia - inertia_ref) / inertia_ref:.3e}")
    assert_close(sums, sums_ref, 1e-5, "per-cluster sums")
    assert torch.equal(counts.cpu().long(), counts_ref)
    assert abs(inertia - inertia_ref) <= 1e-5 * inertia_ref
    again = CF.lloyd_step(pts, init.to(DEV), fused=True)
    assert torch.equal(again[0], sums) and torch.equal(again[1], counts) and again[2] == inertia
    for other in (CF.lloyd_step(pts, init.to(DEV), chunk=1, fused=True), CF.lloyd_step(pts, init.to(DEV), chunk=4, fused=True),
                  CF.lloyd_step([pts[:1], pts[1:3], pts[3:]], init.to(DEV), fused=True)):
        assert_close(other[0], sums, 1e-6, "sums under another chunking")
        assert torch.equal(other[1], counts) and abs(other[2] - inertia) <= 1e-6 * inertia
    # the two-kernel form (what runs when centres + sums do not fit the LDS) computes the same
    two = CF.lloyd_step(pts, init.to(DEV), fused=False)
    dflt = CF.lloyd_step(pts, init.to(DEV))  # whichever form kmeans() runs
    assert_close(dflt[0], sums, 1e-6, "default-form sums")
    # a chunk whose storage does not start on 16 bytes cannot take the fused step's 4-pixel loads: refused there, computed by the other form
    odd = torch.empty(pts.numel() + 1, device=DEV)[1:].view_as(pts).copy_(pts)
    assert odd.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        CF.lloyd_step(odd, init.to(DEV), fused=True)
    unaligned = CF.lloyd_step(odd, init.to(DEV))
    assert_close(unaligned[0], sums, 1e-6, "sums of an unaligned chunk")
    assert torch.equal(unaligned[1], counts)
    assert_close(two[0], sums, 1e-6, "two-kernel sums")
    assert torch.equal(two[1], counts) and abs(two[2] - inertia) <= 1e-6 * inertia
    mean, var = CF.mean_variance(pts)
    assert_close(mean, X.mean(0), 1e-5, "mean of the points")
    assert abs(var - R.mean_variance(X)) <= 1e-5 * R.mean_variance(X)


def test_ten_seeded_starts_always_reach_the_optimum_single_forgy_runs_do_not():
    CF, pts, X = _fixture()
    want = float(golden("kmeans")["inertia"])
    reached = []
    for seed in range(8):
        res = CF.kmeans(pts, R.K, n_init=10, generator=seed)
        reached.append(res.inertia / want)
    forgy = []
    for seed in range(8):
        _, centres = CF.lloyd(pts, R.K, generator=torch.Generator().manual_seed(seed))
        forgy.append(CF.inertia(pts, centres) / want)
    print("kmeans(n_init=10), inertia / optimum over seeds 0-7:", " ".join(f"{r:.6f}" for r in reached))
    print("single Forgy lloyd(), inertia / optimum over seeds 0-7:", " ".join(f"{r:.3f}" for r in forgy),
          f"-> {sum(abs(r - 1) <= 1e-5 for r in forgy)} of 8 reach it")
    assert all(abs(r - 1) <= 1e-5 for r in reached), reached


def test_training_time_shape_times_eight():
    """[8,512,64,64] random activations, K = 20: predict is cluster_assign bit for bit (same distance arithmetic), and the fused
    step's sums are cluster_sums' on that assignment.  256 full tiles: on 256 CUs w2e_kmeans_plan gives every workgroup exactly one,
    as it does on the [4,64,32,32] fixture above (32 tiles).  Workgroups that walk several tiles, partial tiles, the KP = 16 kernels
    and the other shapes at which the pass kernel takes another path are in tests/test_gpu_kmeans_kernels.py, which chooses the grid."""
    from where2edit_amd import clustering_feature as CF
    from where2edit_amd.run_attention import cluster_assign
    pts = seeded.tensor("kmeans_scale.points", (8, 512, 64, 64)).to(DEV)
    centres = (0.3 * seeded.tensor("kmeans_scale.centres", (20, 576))).to(DEV)
    assign = cluster_assign(pts, centres)
    assert torch.equal(CF.predict(pts, centres), assign)
    sums, counts, inertia = CF.lloyd_step(pts, centres, fused=True)
    ref_sums, ref_counts = CF.cluster_sums(pts, assign, 20)
    assert int(ref_counts.min()) > 0
    assert torch.equal(counts.float(), ref_counts)
    assert_close(sums, ref_sums, 1e-5, "fused step vs cluster_sums")
    d = ((CF.points_matrix(pts[:1]).double() - centres.double()[assign[0].reshape(-1).long()]) ** 2).sum()
    assert abs(CF.inertia(pts[:1], centres) - float(d)) <= 1e-5 * float(d)
    big = (0.3 * seeded.tensor("kmeans_scale.centres32", (32, 576))).to(DEV)  # K = 32 at 576 dimensions: the two-kernel form
    with pytest.raises(RuntimeError, match="does not fit"):
        CF.lloyd_step(pts, big, fused=True)
    a32 = cluster_assign(pts, big)
    s32, c32, _ = CF.lloyd_step(pts, big)
    r32, rc32 = CF.cluster_sums(pts, a32, 32)
    assert torch.equal(c32.float(), rc32)
    assert_close(s32, r32, 1e-5, "two-kernel step vs cluster_sums")


def test_fit_clusters_drives_a_generator_to_a_centres_file(tmp_path):
    import make_golden_attention as M
    from where2edit_amd import checkpoints, clustering_feature as CF
    from where2edit_amd.attention_model import Generator
    from where2edit_amd.stylegan2 import freeze_conv_weights
    g = Generator(256, 512, 8)
    g.load_state_dict(seeded.generator_state_dict(256), strict=True)
    g = g.to(DEV).eval()
    freeze_conv_weights(g)
    res = CF.fit_clusters(g, steps=4, batch=1, attention_layer=M.ATT_LAYER, clusters=6, generator=11)
    with torch.no_grad():
        _, _, _, fm = g([seeded.wplus_latents(1, g.n_latent).to(DEV)], input_is_latent=True, randomize_noise=False, return_features=True)
    c, s = fm[M.ATT_LAYER - 1].shape[1], fm[M.ATT_LAYER - 1].shape[2]
    assert tuple(res.centres.shape) == (6, c + 2 * (c // 16)) and bool(torch.isfinite(res.centres).all())
    assert tuple(res.assign.shape) == (4, 2 * s, 2 * s) and int(res.counts.min()) > 0 and int(res.counts.sum()) == 4 * 4 * s * s
    path = tmp_path / "clusters.pkl"
    checkpoints.save_clusters(res.centres, path)
    assert torch.equal(checkpoints.load_clusters(path), res.centres.cpu())
    rows = seeded.wplus_latents(5, g.n_latent, salt=3)
    again = CF.fit_clusters(g, steps=2, batch=2, attention_layer=M.ATT_LAYER, clusters=6, latents=rows, generator=11, n_init=2)
    assert tuple(again.assign.shape) == (4, 2 * s, 2 * s) and len(again.inertias) == 2
