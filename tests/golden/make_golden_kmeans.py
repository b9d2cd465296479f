"""Generates tests/golden/kmeans.npz: what scikit-learn's KMeans computes on the seeded fixture problem of tests/kmeans_ref.py
(4096 points of 72 dimensions, K = 6): centres, inertia, counts and labels of `KMeans(6, n_init=10, random_state=42)`.

    python tests/golden/make_golden_kmeans.py        (needs scikit-learn; never runs on the GPU box)

The fixture is only usable if the optimum is unambiguous, so this script also asserts what the tests lean on: every 10-start
run (random_state 0-7 and 42) lands on the same inertia to 1e-6 relative, the labels are a float64 nearest-centre labelling,
and no point is a near-tie (two best distances within 1e-5 relative).  K = 10 (more clusters than prototypes) does not have the
first property, which is why the fixture uses K = 6."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import kmeans_ref as R  # noqa: E402


def main():
    from sklearn.cluster import KMeans
    import sklearn
    X = R.fixture_matrix().numpy()
    assert X.shape == (4096, 72)
    runs = {rs: KMeans(n_clusters=R.K, n_init=10, random_state=rs).fit(X) for rs in list(range(8)) + [42]}
    ref = runs[42]
    for rs, km in runs.items():
        assert abs(km.inertia_ - ref.inertia_) <= 1e-6 * ref.inertia_, (rs, km.inertia_, ref.inertia_)
    singles = {init: [KMeans(n_clusters=R.K, n_init=1, init=init, random_state=rs).fit(X).inertia_ / ref.inertia_ for rs in range(8)]
               for init in ("random", "k-means++")}
    lab, _, gap = R.nearest(torch.from_numpy(X), torch.from_numpy(ref.cluster_centers_))
    assert np.array_equal(lab.numpy(), ref.labels_) and float(gap.min()) > 1e-5, float(gap.min())
    counts = np.bincount(ref.labels_, minlength=R.K)
    path = os.path.join(HERE, "kmeans.npz")
    np.savez_compressed(path, centres=ref.cluster_centers_, inertia=np.float64(ref.inertia_), counts=counts.astype(np.int64),
                        labels=ref.labels_.astype(np.uint8), n_iter=np.int64(ref.n_iter_))
    print("scikit-learn", sklearn.__version__, "inertia", ref.inertia_, "counts", counts.tolist(), "min gap", float(gap.min()))
    for init, r in singles.items():
        print(f"single start, init={init}: inertia / optimum over seeds 0-7:", " ".join(f"{v:.3f}" for v in r))
    print("saved", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
