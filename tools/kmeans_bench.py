"""Times the offline k-means walks at the reference's scale (clustering_feature.py:347-397: 300 x [1,512,128,128] activations
up-sampled from 64^2, K = 20; fewer images with --images):

  * the k-means++ seeding pass (2 + int(log K) candidates at once) and one fused Lloyd step of csrc/kmeans.hip,
  * the same step as two kernels (w2e_kmeans_pass mode 0 + w2e_cluster_accumulate),
  * the training-time pair the package had before: cluster_assign + cluster_sums,

on the same random points, with HIP events around device-synchronised repeats, and prints one JSON line per variant with the
achieved GB/s against ONE read of the points (B*C*s*s*4 bytes).  The variants are run alternately, `--repeats` times each
(>= 5): `ms_min .. ms_max` is the run-to-run spread a difference has to exceed.  --sklearn also times scikit-learn's KMeans on
the host for a reduced point set (one Lloyd iteration's worth is not separable there: the whole fit is timed).
Every interval is a whole call of the Python entry point: it includes the allocation of the partials and the ctypes calls (tens of
microseconds), nothing at 300 images and a visible share with a small --images.  Lines are appended to --out.

    python tools/kmeans_bench.py [--images 300] [--sklearn] [--out profiles/kmeans_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--clusters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-images", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "kmeans_bench.jsonl"))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("--repeats must be >= 5: the spread is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench needs the GPU: a host timing says nothing about these kernels")
    from where2edit_amd import clustering_feature as CF
    from where2edit_amd.run_attention import cluster_assign
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    pts = torch.empty((a.images, a.channels, a.size, a.size), device=dev)
    for i in range(a.images):  # (one image at a time: no second copy of 10 GB)
        pts[i].normal_(generator=g)
    k, d = a.clusters, a.channels + 2 * (a.channels // 16)
    centres = 0.3 * torch.randn((k, d), device=dev, generator=g)
    t = CF.n_local_trials(k)
    P = CF._Points([pts])
    mind = torch.rand(P.n, device=dev, generator=g) * 100
    cand = torch.empty((t, P.n), device=dev)
    assign = cluster_assign(pts, centres)

    def fused():
        CF._lloyd_step(P, centres, fused=True)

    def two_kernels():
        CF._lloyd_step(P, centres, fused=False)

    def parent_pair():
        CF.cluster_sums(pts, cluster_assign(pts, centres), k)

    variants = {"seed_pass": lambda: CF._walk(P, 2, centres[:t], t, mind=mind, cand=cand),
                "assign_mind": lambda: CF._walk(P, 0, centres, 1, assign=[assign]),
                "fused_step": fused, "two_kernel_step": two_kernels, "parent_assign_plus_sums": parent_pair,
                "parent_assign": lambda: cluster_assign(pts, centres), "parent_sums": lambda: CF.cluster_sums(pts, assign, k)}
    if not CF._fused_fits(P, k):
        variants.pop("fused_step")
    times = {n: [] for n in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    nbytes = pts.numel() * 4
    lines = []
    for name, ms in times.items():
        med = statistics.median(ms)
        lines.append({"tool": "kmeans_bench", "variant": name, "images": a.images, "channels": a.channels, "size": a.size, "clusters": k,
                      "points": P.n, "bytes_one_read": nbytes, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "repeats": len(ms),
                      "gb_per_s_one_read": nbytes / med / 1e6})
    if a.sklearn:
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            print("scikit-learn does not import here: host timing skipped", file=sys.stderr)
        else:
            X = CF.points_matrix(pts[:a.sklearn_images]).cpu().numpy()
            t0 = time.perf_counter()
            km = KMeans(n_clusters=k, n_init=1, random_state=42).fit(X)
            dt = time.perf_counter() - t0
            t0 = time.perf_counter()
            res = CF.kmeans(pts[:a.sklearn_images], k, n_init=1, generator=42)
            torch.cuda.synchronize()
            lines.append({"tool": "kmeans_bench", "variant": "sklearn_host_fit_n_init_1", "images": a.sklearn_images, "points": int(X.shape[0]),
                          "seconds": dt, "n_iter": int(km.n_iter_), "seconds_per_iter": dt / max(int(km.n_iter_), 1),
                          "hip_fit_seconds_same_points": time.perf_counter() - t0, "hip_n_iter": res.n_iter})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
