"""Float64 restatement of the offline k-means on the literal [N,D] point matrix (clustering_feature.points_matrix), for the
tests of where2edit_amd.clustering_feature.kmeans: the seeded fixture problem, greedy k-means++ (2 + int(log K)
candidates per round, inverse-CDF draws from supplied uniforms), Lloyd with scikit-learn's stopping rule, and the helpers
the comparisons need.  CPU only, no GPU library."""
import math

import numpy as np
import torch

import seeded

B, C, S, K = 4, 64, 16, 6  # -> 4 * 32 * 32 = 4096 points of 64 + 2 * 4 = 72 dimensions


def fixture_feature():
    """[4,64,16,16]: six prototype vectors ~ N(0,1), one label per 4x4 block (constant inside a block, so the bilinear x2
    up-sampling blends only along block edges), + 0.3 N(0,1)."""
    protos = seeded.tensor("kmeans_fixture.protos", (K, C), 1.0)
    lab = torch.from_numpy(np.random.RandomState(3).randint(0, K, size=(B, S // 4, S // 4)))
    lab = lab.repeat_interleave(4, 1).repeat_interleave(4, 2)
    return (protos[lab].permute(0, 3, 1, 2) + 0.3 * seeded.tensor("kmeans_fixture.noise", (B, C, S, S))).contiguous()


def fixture_points(device="cpu"):
    from where2edit_amd.clustering_feature import clustering_points
    return clustering_points(fixture_feature().to(device))


def fixture_matrix():
    from where2edit_amd.clustering_feature import points_matrix
    return points_matrix(fixture_points()).double()


def sq_dists(X, cen):
    """[N,K] squared distances in the sum (a-b)^2 form, float64."""
    return ((X.double()[:, None, :] - cen.double()[None, :, :]) ** 2).sum(2)


def nearest(X, cen):
    """(labels [N], squared distance to the nearest centre [N], relative gap between the two best distances [N])."""
    d = sq_dists(X, cen)
    lab = d.argmin(1)
    if d.shape[1] == 1:
        return lab, d[:, 0], torch.full_like(d[:, 0], float("inf"))
    two = d.topk(2, dim=1, largest=False).values
    return lab, two[:, 0], (two[:, 1] - two[:, 0]) / two[:, 1].clamp_min(1e-300)


def lloyd_step(X, cen):
    """(sums [K,D], counts [K], inertia) of the nearest-centre labelling."""
    lab, dmin, _ = nearest(X, cen)
    k = cen.shape[0]
    sums = torch.zeros((k, X.shape[1]), dtype=torch.float64).index_add_(0, lab, X.double())
    return sums, torch.bincount(lab, minlength=k), float(dmin.sum())


def n_local_trials(k):
    return 2 + int(math.log(k))


def plusplus(X, k, draws=None, generator=None, min_margin=0.0):
    """Greedy k-means++.  draws [k, T] uniforms: draws[0,0] picks the first centre (floor(u * N)), row c the T candidates of round
    c by inverse CDF over the running minimum squared distance.  Without `draws` they come from `generator`, and a draw is taken
    again while its scaled value v lies within min_margin * v of a step of the CDF (such a draw could land on the neighbouring
    point when the CDF is summed in another order or precision).  Returns (indices, mind [N], draws used, smallest margin)."""
    X = X.double()
    n, t = X.shape[0], n_local_trials(k)
    used = torch.zeros((k, t), dtype=torch.float64)
    used[0] = torch.as_tensor(draws[0], dtype=torch.float64) if draws is not None else torch.rand(t, generator=generator, dtype=torch.float64)
    first = min(int(float(used[0, 0]) * n), n - 1)
    idx = [first]
    mind = sq_dists(X, X[first:first + 1])[:, 0]
    margin = float("inf")

    def margins(cdf, u):
        v = u * cdf[-1]
        i = torch.searchsorted(cdf, v).clamp(max=n - 1)
        below = torch.where(i > 0, cdf[(i - 1).clamp_min(0)], torch.zeros_like(v))
        return torch.minimum(v - below, cdf[i] - v) / v, i

    for c in range(1, k):
        cdf = torch.cumsum(mind, 0)
        if draws is not None:
            u = torch.as_tensor(draws[c], dtype=torch.float64)
        else:
            u = torch.rand(t, generator=generator, dtype=torch.float64)
            for _ in range(10000):
                bad = margins(cdf, u)[0] <= min_margin
                if not bad.any():
                    break
                u[bad] = torch.rand(int(bad.sum()), generator=generator, dtype=torch.float64)
        used[c] = u
        m, ids = margins(cdf, u)
        margin = min(margin, float(m.min()))
        dc = sq_dists(X, X[ids])                       # [N, T]
        pots = torch.minimum(mind[:, None], dc).sum(0)
        best = int(pots.argmin())
        mind = torch.minimum(mind, dc[:, best])
        idx.append(int(ids[best]))
    return idx, mind, used, margin


def mean_variance(X):
    return float(X.double().var(0, unbiased=False).mean())


def lloyd(X, init, max_iter=300, tol=1e-4):
    """Lloyd from `init` with scikit-learn's stop (squared centre shift <= tol * mean variance); an empty cluster keeps its
    centre.  Returns (centres, labels, inertia, n_iter) with labels / inertia of the returned centres."""
    X = X.double()
    cen = init.double().clone()
    bound = tol * mean_variance(X)
    it = 0
    for it in range(1, max_iter + 1):
        sums, counts, _ = lloyd_step(X, cen)
        new = torch.where(counts[:, None] > 0, sums / counts[:, None].clamp_min(1), cen)
        shift = float(((new - cen) ** 2).sum())
        cen = new
        if shift <= bound:
            break
    lab, dmin, _ = nearest(X, cen)
    return cen, lab, float(dmin.sum()), it


def kmeans(X, k, n_init, generator):
    """n_init greedy-k-means++ starts; the lowest inertia wins."""
    best = None
    for _ in range(n_init):
        draws = torch.rand((k, n_local_trials(k)), generator=generator, dtype=torch.float64)
        idx = plusplus(X, k, draws)[0]
        run = lloyd(X, X[idx])
        if best is None or run[2] < best[2]:
            best = run
    return best


def match(centres, ref):
    """perm with centres[perm[j]] the centre nearest to ref[j]; asserts it is a permutation."""
    perm = sq_dists(ref, centres).argmin(1)
    assert sorted(perm.tolist()) == list(range(ref.shape[0])), perm
    return perm
