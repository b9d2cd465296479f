"""attention/clustering_feature.py, the offline step that produces the k-means centres the region-attention net
assigns pixels to: per sampled image, the `attention_layer` activation bilinearly up-sampled x2 plus C/16 x-position and
C/16 y-position channels (:373-387) are the points; the reference hands all of them to sklearn's CPU KMeans (:394) and
also carries its own torch `lloyd` (:212-235, forgy init, centre-shift tolerance).

Here the points never leave the GPU and are never materialised as an [N, 576] matrix: Lloyd's two steps run on the
up-sampled activations in place -- `w2e_cluster_assign` (the same kernel the net uses at training time) and
`w2e_cluster_accumulate` (per-cluster sums by a fixed-order reduction, position channels evaluated analytically).

`fit_clusters` / `kmeans` are the reference's workflow itself (:347-397, with what sklearn's KMeans does there: k-means++
seeding, restarts, its stopping rule) on the persistent kernel of csrc/kmeans.hip; `lloyd` stays the reference's helper."""
import bisect
import ctypes
import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from ._lib import call, ptr, stream_ptr
from .run_attention import _i32ptr, cluster_assign


def clustering_points(blend_feature):
    """:373-381: the x2 bilinear (align_corners=True) up-sampling of the activation; the position channels are implicit
    (2*i/(size-1) - 1 along x and y, C/16 copies each).  Returns [B,C,2s,2s] on the input's device."""
    size = blend_feature.shape[2] * 2
    return F.interpolate(blend_feature.detach(), size=size, mode="bilinear", align_corners=True).contiguous()


def points_matrix(points):
    """The literal [B*s*s, C + 2*(C//16)] matrix of :382-391 (tests / interop with sklearn only)."""
    b, c, s, _ = points.shape
    pc = c // 16
    xs = torch.arange(s, device=points.device).float().unsqueeze(0).repeat(s, 1) * 2 / float(s - 1) - 1
    ys = torch.arange(s, device=points.device).float().unsqueeze(1).repeat(1, s) * 2 / float(s - 1) - 1
    cat = torch.cat([points, xs[None, None].repeat(b, pc, 1, 1), ys[None, None].repeat(b, pc, 1, 1)], 1)
    return cat.permute(0, 2, 3, 1).reshape(-1, c + 2 * pc)


def cluster_sums(points, assign, clusters):
    """(sums [K, D], counts [K]) of the points of every cluster."""
    b, c, s, _ = points.shape
    pc = c // 16
    partial = torch.empty((b, clusters, c + 2 * pc), device=points.device, dtype=torch.float32)
    counts = torch.empty((b, clusters), device=points.device, dtype=torch.float32)
    call("w2e_cluster_accumulate", ptr(points), _i32ptr(assign), ptr(partial), ptr(counts), b, c, pc, s, clusters, stream_ptr())
    return partial.sum(0), counts.sum(0)


def _forgy_draw(n_points, n_clusters, generator=None):
    return torch.multinomial(torch.ones(n_points), n_clusters, generator=generator).tolist()


def forgy(points, n_clusters, generator=None):
    """:205-209: n_clusters distinct points drawn uniformly."""
    pts = _Points([points])
    return pts.rows(_forgy_draw(pts.n, n_clusters, generator))


def lloyd(points, n_clusters, tol=1e-4, initial_state=None, max_iter=300, generator=None):
    """:212-235: assign every point to its nearest centre, move the centres to the means, until the summed centre shift,
    squared, falls under `tol`.  points: [B,C,s,s] (clustering_points).  Returns (assign int32 [B,s,s], centres [K,D]).
    A cluster that loses all its points keeps its centre (the reference's mean of an empty selection is NaN)."""
    centres = (initial_state if initial_state is not None else forgy(points, n_clusters, generator)).to(points.device, torch.float32).clone()
    assign = None
    for _ in range(max_iter):
        assign = cluster_assign(points, centres)
        sums, counts = cluster_sums(points, assign, n_clusters)
        new = torch.where(counts[:, None] > 0, sums / counts[:, None].clamp_min(1), centres)
        shift = torch.sum(torch.sqrt(torch.sum((new - centres) ** 2, dim=1)))
        centres = new
        if float(shift) ** 2 < tol:
            break
    return assign, centres


# ------------------------------------------------------------------------------------------------------------------------
# Offline k-means as the reference runs it (:347-397 + scikit-learn 0.24's KMeans defaults): greedy k-means++ seeding, n_init
# restarts, the centre-shift stopping rule relative to the variance of the points, best inertia wins.  Every walk of the
# points is one launch of the persistent kernel of csrc/kmeans.hip (`w2e_kmeans_pass`): seeding pass, fused Lloyd step,
# assignment + min distance.  The points stay on the device as the [b,C,s,s] tensors clustering_points() returns.
MAX_CLUSTERS = 32
_ASSIGN, _STEP, _SEED = 0, 1, 2
# The Lloyd step's form where both fit.  False: assignment (w2e_kmeans_pass mode 0) + w2e_cluster_accumulate.  The fused kernel becomes
# the default only once tools/kmeans_bench.py shows it faster than that pair on the MI355X by more than its spread.
_FUSED_DEFAULT = False


@dataclass
class KMeansResult:
    centres: torch.Tensor      # [K, D] float32
    assign: torch.Tensor       # int32 [B, s, s], the labelling of `centres`
    inertia: float             # sum of squared distances to `centres`
    n_iter: int                # Lloyd iterations of the winning restart
    counts: torch.Tensor       # [K] int64, points per cluster under `assign`
    inertias: list = field(default_factory=list)  # final inertia of every restart, in order
    empty_clusters: int = 0    # clusters of the result without a point


def _as_chunks(points, chunk=None):
    """`points` as a list of [b_i,C,s,s] tensors: a list is taken as given, a tensor is walked `chunk` images at a time."""
    if isinstance(points, (list, tuple)):
        if chunk is not None:
            raise ValueError("kmeans: `chunk` splits one tensor; a list of tensors is already chunked")
        chunks = list(points)
        if not chunks:
            raise ValueError("kmeans: empty chunk list")
    else:
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"kmeans: chunk must be >= 1 (got {chunk})")
        chunks = [points] if chunk is None else [points[i:i + int(chunk)] for i in range(0, points.shape[0], int(chunk))]
        if not chunks:
            raise ValueError("kmeans: no points")
    first = chunks[0]
    for t in chunks:
        if not torch.is_tensor(t) or t.ndim != 4 or t.shape[2] != t.shape[3] or t.shape[0] < 1:
            raise ValueError("kmeans: every chunk is a [b,C,s,s] tensor (clustering_points) with b >= 1")
        if t.shape[1:] != first.shape[1:] or t.device != first.device:
            raise ValueError(f"kmeans: chunks disagree: {tuple(t.shape)} on {t.device} vs {tuple(first.shape)} on {first.device}")
    return chunks


def _check_clusters(n_clusters, n_points=None):
    if not 1 <= int(n_clusters) <= MAX_CLUSTERS:
        raise ValueError(f"kmeans: 1 <= n_clusters <= {MAX_CLUSTERS} (got {n_clusters}): the kernels keep one distance per cluster in registers")
    if n_points is not None and n_clusters > n_points:
        raise ValueError(f"kmeans: {n_clusters} clusters for {n_points} points")


def _generator(generator):
    """A torch.Generator (CPU), an int seed, or None (a fresh generator seeded from the global one)."""
    if isinstance(generator, torch.Generator):
        return generator
    g = torch.Generator()
    g.manual_seed(int(generator) if generator is not None else int(torch.randint(0, 2 ** 31 - 1, (1,))))
    return g


class _Points:
    """The chunks, their row offsets in the literal [N,D] matrix (points_matrix order: image, y, x) and the launch plan of each."""

    def __init__(self, chunks):
        self.chunks = [c.contiguous() for c in chunks]
        _, self.c, self.s, _ = self.chunks[0].shape
        self.pc = self.c // 16
        self.d = self.c + 2 * self.pc
        self.device = self.chunks[0].device
        self.offsets = [0]
        for c in self.chunks:
            self.offsets.append(self.offsets[-1] + c.shape[0] * self.s * self.s)
        self.n = self.offsets[-1]
        self._plans = {}

    def plan(self, batch, clusters):
        key = (batch, clusters)
        if key not in self._plans:
            grid, fused = ctypes.c_int(0), ctypes.c_int(0)  # (fused: centres + running sums fit the LDS)
            call("w2e_kmeans_plan", batch, self.c, self.pc, self.s, clusters, ctypes.byref(grid), ctypes.byref(fused))
            self._plans[key] = (grid.value, bool(fused.value))
        return self._plans[key]

    def rows(self, indices):
        """[len(indices), D] rows of the point matrix."""
        out = []
        for i in indices:
            j = bisect.bisect_right(self.offsets, i) - 1
            bi, p = divmod(i - self.offsets[j], self.s * self.s)
            y, x = divmod(p, self.s)
            pos = torch.tensor([x * 2 / float(self.s - 1) - 1] * self.pc + [y * 2 / float(self.s - 1) - 1] * self.pc, device=self.device)
            out.append(torch.cat([self.chunks[j][bi, :, y, x], pos]))
        return torch.stack(out)


def _vptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _walk(pts, mode, centres, n_out, assign=None, mind=None, cand=None):
    """One walk of all the points in `mode`; returns the float64 accumulator [n_out] (chunks and workgroup partials added in a
    fixed order by w2e_kmeans_reduce).  assign: list of int32 tensors per chunk; mind: [N] float32; cand: [T, N] float32."""
    centres = centres.to(pts.device, torch.float32).contiguous()
    k = centres.shape[0]
    if centres.shape[1] != pts.d:
        raise RuntimeError(f"kmeans: centres {tuple(centres.shape)} for points of {pts.d} dimensions")
    acc = torch.zeros(n_out, device=pts.device, dtype=torch.float64)
    for j, x in enumerate(pts.chunks):
        b = x.shape[0]
        grid, _ = pts.plan(b, k)
        partial = torch.empty((grid, n_out), device=pts.device, dtype=torch.float32)
        lo = pts.offsets[j]
        call("w2e_kmeans_pass", mode, ptr(x), ptr(centres), _i32ptr(assign[j]) if assign is not None else None,
             ptr(mind[lo:]) if mind is not None else None, ctypes.c_void_p(cand.data_ptr() + 4 * lo) if cand is not None else None,
             cand.shape[1] if cand is not None else 0, ptr(partial), grid, b, pts.c, pts.pc, pts.s, k, stream_ptr())
        call("w2e_kmeans_reduce", ptr(partial), grid, n_out, _vptr(acc), stream_ptr())
    return acc


def _new_assign(pts):
    return [torch.empty((c.shape[0], pts.s, pts.s), device=pts.device, dtype=torch.int32) for c in pts.chunks]


def _fused_fits(pts, k):
    """The fused step needs centres + sums within the LDS and 16-byte aligned chunks (it reads 4 pixels per load)."""
    return all(pts.plan(c.shape[0], k)[1] and c.data_ptr() % 16 == 0 for c in pts.chunks)


def _lloyd_step(pts, centres, assign=None, fused=None):
    """(sums [K,D] float64, counts [K] float64, inertia 0-d float64) of the nearest-centre labelling of `centres`; the labelling goes
    to `assign` (list per chunk) when given.  fused: None = the default form where it fits, True = the fused kernel or an error,
    False = assignment + w2e_cluster_accumulate."""
    k, d1 = centres.shape[0], pts.d + 1
    if fused and not _fused_fits(pts, k):
        raise RuntimeError(f"kmeans: the fused Lloyd step does not fit {k} clusters of {pts.d} dimensions in the LDS (or a chunk is not 16-byte aligned)")
    if fused is None:
        fused = _FUSED_DEFAULT and _fused_fits(pts, k)
    if fused:
        acc = _walk(pts, _STEP, centres, k * d1 + 1, assign=assign)
        table = acc[:k * d1].view(k, d1)
        return table[:, :pts.d], table[:, pts.d], acc[k * d1]
    # centres + running sums beyond the LDS (K > 24 at 576 dimensions), or the A/B switch: two kernels
    assign = assign if assign is not None else _new_assign(pts)
    inertia = _walk(pts, _ASSIGN, centres, 1, assign=assign)[0]
    sums = torch.zeros((k, pts.d), device=pts.device, dtype=torch.float64)
    counts = torch.zeros(k, device=pts.device, dtype=torch.float64)
    for x, a in zip(pts.chunks, assign):
        b = x.shape[0]
        partial = torch.empty((b, k, pts.d), device=pts.device, dtype=torch.float32)
        cnt = torch.empty((b, k), device=pts.device, dtype=torch.float32)
        call("w2e_cluster_accumulate", ptr(x), _i32ptr(a), ptr(partial), ptr(cnt), b, pts.c, pts.pc, pts.s, k, stream_ptr())
        sums += partial.double().sum(0)
        counts += cnt.double().sum(0)
    return sums, counts, inertia


def lloyd_step(points, centres, chunk=None, fused=None):
    """One Lloyd step from `centres`: (sums [K,D], counts [K], inertia), float64 on the device, of the nearest-centre labelling.
    fused=True insists on the fused kernel (an error where centres + sums do not fit the LDS: K > 24 at 576 dimensions),
    fused=False runs assignment + w2e_cluster_accumulate, None what kmeans() runs."""
    _check_clusters(centres.shape[0])
    sums, counts, inertia_ = _lloyd_step(_Points(_as_chunks(points, chunk)), centres, fused=fused)
    return sums, counts, float(inertia_)


def mean_variance(points, chunk=None):
    """(mean [D] float64, mean over the D dimensions of the per-dimension variance) of the points, implicit position channels
    included: two walks with one 'cluster' -- the sums about 0, then the squared distances to the mean (no E[x^2] - E[x]^2)."""
    pts = points if isinstance(points, _Points) else _Points(_as_chunks(points, chunk))
    zero = torch.zeros((1, pts.d), device=pts.device)
    sums, counts, _ = _lloyd_step(pts, zero)
    mean = sums[0] / counts[0]
    spread = _walk(pts, _ASSIGN, mean[None].float(), 1)[0]
    return mean, float(spread) / (pts.n * pts.d)


def n_local_trials(n_clusters):
    """Candidates per round of the greedy k-means++ (scikit-learn: 2 + int(log K))."""
    return 2 + int(math.log(n_clusters))


def _plusplus(pts, n_clusters, draws):
    """Greedy k-means++ (Arthur & Vassilvitskii 2007, with scikit-learn's best-of-T-candidates rounds).  draws: [K, T] uniforms in
    [0,1), float64, on the host: draws[0,0] picks the first centre uniformly, draws[c] the T candidates of round c by inverse CDF
    over the running minimum distances.  Returns (centres [K,D], indices (list), mind [N] float32)."""
    t = n_local_trials(n_clusters)
    draws = torch.as_tensor(draws, dtype=torch.float64).cpu()
    if tuple(draws.shape) != (n_clusters, t):
        raise ValueError(f"kmeans: draws must be [{n_clusters}, {t}] (got {tuple(draws.shape)})")
    n = pts.n
    cand = torch.empty((t, n), device=pts.device, dtype=torch.float32)
    first = min(int(float(draws[0, 0]) * n), n - 1)
    indices, centres = [first], pts.rows([first])
    _walk(pts, _SEED, centres, 1, cand=cand)
    mind = cand[0].clone()
    for c in range(1, n_clusters):
        cdf = torch.cumsum(mind.double(), 0)  # 8 B per point; the features are 4*D
        ids = torch.searchsorted(cdf, draws[c].to(pts.device) * cdf[-1]).clamp_(max=n - 1).tolist()
        rows = pts.rows(ids)
        pots = _walk(pts, _SEED, rows, t, mind=mind, cand=cand)
        best = int(torch.argmin(pots))
        torch.minimum(mind, cand[best], out=mind)  # commit: the candidate's distance plane is still there
        indices.append(ids[best])
        centres = torch.cat([centres, rows[best:best + 1]])
    return centres, indices, mind


def kmeans_plusplus(points, n_clusters, *, draws=None, generator=None, chunk=None):
    """The seeding alone: (centres [K,D], the K point indices in points_matrix order, the minimum squared distance of every
    point to the chosen centres [N]).  `draws` ([K, 2 + int(log K)] uniforms) replaces the generator's numbers."""
    _check_clusters(n_clusters)
    pts = _Points(_as_chunks(points, chunk))
    _check_clusters(n_clusters, pts.n)
    if draws is None:
        draws = torch.rand((n_clusters, n_local_trials(n_clusters)), generator=_generator(generator), dtype=torch.float64)
    return _plusplus(pts, n_clusters, draws)


def kmeans(points, n_clusters, *, init="k-means++", n_init=None, max_iter=300, tol=1e-4, generator=None, chunk=None):
    """scikit-learn 0.24's `KMeans(n_clusters).fit` (what :394 runs) on the device.  points: the [B,C,s,s] tensor of
    clustering_points(), or a list of such tensors; the 2*(C//16) position channels stay implicit.

    init: "k-means++" (greedy, 2 + int(log K) candidates per round), "random" (forgy's draw: K distinct points) or a [K,D]
    tensor.  n_init: restarts, default 10 -- 1 with an explicit init tensor, where any other value is refused.  The restart
    with the lowest inertia wins.  Stopping rule: squared Frobenius norm of the centre shift <= tol * (mean over the D
    dimensions of the variance of the points), or max_iter.  One more assignment pass follows the loop, so `assign`,
    `inertia` and `counts` belong to the returned centres.  generator: a torch.Generator on the CPU or an int seed.
    chunk: walk a single tensor `chunk` images at a time.  Sums, counts and inertia are added chunk by chunk in a fixed order
    in float64: identical chunking and seed give bit-identical results, another chunking the same up to fp32 summation order.

    A cluster that loses all its points keeps its centre, as lloyd() does (scikit-learn relocates it to the point farthest
    from its centre); `empty_clusters` reports how many the result has.  K <= 32."""
    _check_clusters(n_clusters)
    explicit = torch.is_tensor(init)
    if explicit:
        if n_init not in (None, 1):
            raise ValueError(f"kmeans: an explicit init is one start: n_init must be 1 (got {n_init})")
        n_init = 1
        if init.ndim != 2 or init.shape[0] != n_clusters:
            raise ValueError(f"kmeans: init {tuple(init.shape)} for {n_clusters} clusters")
    elif init not in ("k-means++", "random"):
        raise ValueError(f"kmeans: init is 'k-means++', 'random' or a [K,D] tensor (got {init!r})")
    n_init = 10 if n_init is None else int(n_init)
    if n_init < 1 or max_iter < 1:
        raise ValueError("kmeans: n_init and max_iter must be >= 1")
    pts = _Points(_as_chunks(points, chunk))
    _check_clusters(n_clusters, pts.n)
    gen = _generator(generator)
    _, var = mean_variance(pts)
    bound = tol * var
    best, inertias = None, []
    for _ in range(n_init):
        if explicit:
            centres = init.to(pts.device, torch.float32).clone()
        elif init == "random":
            centres = pts.rows(_forgy_draw(pts.n, n_clusters, gen))  # forgy()'s draw, over all chunks
        else:
            centres, _, _ = _plusplus(pts, n_clusters, torch.rand((n_clusters, n_local_trials(n_clusters)), generator=gen, dtype=torch.float64))
        n_iter = 0
        for n_iter in range(1, max_iter + 1):
            sums, counts, _ = _lloyd_step(pts, centres)
            new = torch.where(counts[:, None] > 0, sums / counts[:, None].clamp_min(1), centres.double())
            shift = float(((new - centres.double()) ** 2).sum())
            centres = new.float()
            if shift <= bound:
                break
        assign = _new_assign(pts)
        _, counts, inertia = _lloyd_step(pts, centres, assign=assign)
        inertias.append(float(inertia))
        if best is None or inertias[-1] < best.inertia:
            best = KMeansResult(centres, assign, inertias[-1], n_iter, counts.round().long())
    best.assign = torch.cat(best.assign)
    best.inertias = inertias
    best.empty_clusters = int((best.counts == 0).sum())
    return best


def predict(points, centres, chunk=None):
    """int32 [B,s,s]: the nearest centre of every point (bit-identical to run_attention.cluster_assign)."""
    pts = _Points(_as_chunks(points, chunk))
    _check_clusters(centres.shape[0])
    assign = _new_assign(pts)
    _walk(pts, _ASSIGN, centres, 1, assign=assign)
    return torch.cat(assign)


def inertia(points, centres, chunk=None):
    """Sum over the points of the squared distance to the nearest centre."""
    pts = _Points(_as_chunks(points, chunk))
    _check_clusters(centres.shape[0])
    return float(_walk(pts, _ASSIGN, centres, 1)[0])


def fit_clusters(g_ema, *, steps=300, batch=1, attention_layer, clusters, truncation=0.7, latents=None, generator=None, **kmeans_kw):
    """The body of the reference's main_worker (:347-397) without leaving the device: `steps` times, sample z and truncate it
    towards mean_latent(4096) (or draw `batch` rows of `latents`, the reference's --latent_path), run the generator with
    return_features=True, randomize_noise=False and keep clustering_points(feature_map[attention_layer - 1]); then kmeans()
    over the kept chunks.  Returns the KMeansResult; checkpoints.save_clusters(result.centres, path) writes the reference's
    pickle.  generator: torch.Generator on the CPU or an int seed (z draws, latent rows and the k-means draws)."""
    _check_clusters(clusters)
    if steps < 1 or batch < 1:
        raise ValueError(f"fit_clusters: steps and batch must be >= 1 (got {steps}, {batch})")
    if attention_layer < 1:
        raise ValueError(f"fit_clusters: attention_layer counts from 1 (got {attention_layer})")
    if latents is not None and (not torch.is_tensor(latents) or latents.ndim != 3 or len(latents) < 1):
        raise ValueError("fit_clusters: latents is a [n, n_latent, 512] tensor of W+ codes")
    gen = _generator(generator)
    device = next(g_ema.parameters()).device
    kept = None  # [steps*batch, C, 2s, 2s]: one tensor, so that a walk is one launch over every image (a batch-1 chunk has too few tiles to fill the device)
    with torch.no_grad():
        mean = g_ema.mean_latent(4096) if latents is None else None
        for i in range(steps):
            if latents is not None:
                w = latents[torch.randint(len(latents), (batch,), generator=gen)].to(device)
            else:
                z = torch.randn(batch, g_ema.style_dim, generator=gen).to(device)
                _, w, _ = g_ema([z], return_latents=True, truncation=truncation, truncation_latent=mean)
            _, _, _, feature_map = g_ema([w], input_is_latent=True, randomize_noise=False, return_features=True)
            if attention_layer > len(feature_map):
                raise ValueError(f"fit_clusters: attention_layer {attention_layer} of {len(feature_map)} recorded layers")
            x = clustering_points(feature_map[attention_layer - 1])
            if kept is None:
                kept = torch.empty((steps * batch,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
            kept[i * batch:(i + 1) * batch] = x
    return kmeans(kept, clusters, generator=gen, **kmeans_kw)
