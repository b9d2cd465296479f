"""Plain restatements of the region-mask operations of include/w2e_attention.h on stock torch ops, in the dtype of their inputs
(float64 in the tests; float32 where a test measures what an equally valid fp32 evaluation costs).  Written from the header's formulas
and the reference's lines (attention/run_attention.py:775-884, utils.py:244-263, clustering_feature.py:212-235), not from the kernels.
The one index that decides which pixel a gather reads, `nearest_index`, is torch's own F.interpolate: neither closed form is trusted.
Also the seeded inputs that the CPU test (tests/test_mask_ref_host.py) and the GPU test (tests/test_gpu_mask_kernels.py) share."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import seeded
from oracle import attention_net as OA


# ---------------------------------------------------------------------------------------------------- the nearest resize
@functools.lru_cache(maxsize=None)
def _nearest_index(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, n_in)
    return F.interpolate(src, size=n_out, mode="nearest").reshape(n_out).long()


def nearest_index(n_in, n_out):
    """idx [n_out] with F.interpolate(x, n_out, mode='nearest')[..., d] == x[..., idx[d]] for a length-n_in axis: read off an
    `arange` that torch itself resized (float32, CPU; indices below 2^24 are exact in float32)."""
    return _nearest_index(int(n_in), int(n_out)).clone()


def nearest_gather(x, size):
    """F.interpolate(x, size) (nearest) of a [..., r, r] tensor through `nearest_index` (any dtype, integer ids included)."""
    idx = nearest_index(x.shape[-1], size)
    return x[..., idx, :][..., idx]


# ---------------------------------------------------------------------------------------------------- cluster assignment
def points_matrix(feat, pos_channels):
    """The literal [B*S*S, C+2P] point matrix of run_attention.py:775-790: the feature channels, then P copies of the x position and
    P copies of the y position, both linspace(-1, 1, S)."""
    b, c, s, _ = feat.shape
    lin = torch.linspace(-1, 1, s, dtype=feat.dtype)
    xs = lin[None, :].expand(s, s)[None, None].expand(b, pos_channels, s, s)
    ys = lin[:, None].expand(s, s)[None, None].expand(b, pos_channels, s, s)
    return torch.cat([feat, xs, ys], 1).permute(0, 2, 3, 1).reshape(b * s * s, c + 2 * pos_channels)


def assign_ref(feat, centroids, pos_channels):
    """(dist [B*S*S, K] = sum((a - b)^2), ids [B,S,S] = argmin: the lowest k among equals)."""
    b, _, s, _ = feat.shape
    pts = points_matrix(feat, pos_channels)
    dist = ((pts[:, None, :] - centroids[None, :, :]) ** 2).sum(-1)
    return dist, torch.argmin(dist, 1).reshape(b, s, s)


def accumulate_ref(feat, assign, pos_channels, clusters):
    """(partial [B,K,C+2P], counts [B,K]) of w2e_cluster_accumulate: index_add of the point matrix' rows, per image."""
    b, c, s, _ = feat.shape
    d = c + 2 * pos_channels
    pts = points_matrix(feat, pos_channels).reshape(b, s * s, d)
    ids = assign.reshape(b, s * s).long()
    partial, counts = feat.new_zeros(b, clusters, d), feat.new_zeros(b, clusters)
    for bb in range(b):
        partial[bb].index_add_(0, ids[bb], pts[bb])
        counts[bb].index_add_(0, ids[bb], feat.new_ones(s * s))
    return partial, counts


# The shapes (C, P, S, K, B) of tests/test_gpu_mask_kernels.py and what each one exercises in cluster_assign.
ASSIGN_SHAPES = [
    (512, 32, 16, 20, 2),  # KP = 32; 106 KB LDS opt-in
    (37, 2, 9, 8, 3),      # wave split 9/9/9/10; prefetch tail; 81 pixels; K = KP
    (64, 4, 13, 9, 1),     # KP = 16 with 7 padded columns
    (3, 0, 5, 1, 2),       # wave 0 owns no channel; P = 0; K = 1
    (16, 1, 64, 32, 1),    # full K = 32
    (16, 1, 2, 17, 1),     # minimum S = 2
    (960, 32, 8, 32, 1),   # exactly the 160 KB bound of cluster_assign (in w2e_kmeans_pass mode 0: the three-block kernel; KMEANS_WIDE_SHAPES)
]
ASSIGN_GAP = 1e-4       # a pixel whose float64 runner-up is closer than this (relative) may go either way
ASSIGN_SLACK = 1e-5     # the chosen centre is at most this much (relative) farther than the float64 minimum
ASSIGN_MAX_TIES = 0.01  # share of a case's pixels that the gap rule may exclude


def assign_case(c, p, s, k, b):
    """Prototype-plus-noise features (every pixel = one of K prototypes + 0.25 noise) and centres = the prototypes + small position
    entries, as the fixtures of this branch are built: float32 (feat [B,C,S,S], centroids [K, C+2P])."""
    key = f"maskk.assign.{c}.{p}.{s}.{k}.{b}"
    protos = seeded.tensor(key + ".protos", (k, c), 1.0)
    lab = torch.from_numpy(np.random.RandomState(c * 131 + s * 7 + k).randint(0, k, size=(b, s, s)))
    feat = (protos[lab].permute(0, 3, 1, 2) + 0.25 * seeded.tensor(key + ".noise", (b, c, s, s))).contiguous()
    cen = torch.cat([protos, 0.05 * seeded.tensor(key + ".cpos", (k, 2 * p))], 1).contiguous()
    return feat, cen


def position_case():
    """An assignment that only the position channels decide: every centre has the same feature part, and the position parts are the
    3 x 3 grid {-2/3, 0, 2/3}^2, so a pixel belongs to the grid cell it lies in.  (In assign_case the prototypes are so far apart that
    the 2P position terms never change the nearest centre: a kernel that dropped them would still pass there.)
    (C, P, S, K, B) = (4, 3, 12, 9, 2): feat [2,4,12,12] = 0.05 noise, centroids [9, 4 + 6]."""
    c, p, s, k, b = 4, 3, 12, 9, 2
    feat = (0.05 * seeded.tensor("maskk.assign.position.feat", (b, c, s, s))).contiguous()
    grid = torch.tensor([-2.0 / 3.0, 0.0, 2.0 / 3.0])
    xs, ys = grid.repeat(3), grid.repeat_interleave(3)  # centre 3 * iy + ix
    cen = torch.cat([torch.zeros(k, c), xs[:, None].expand(k, p), ys[:, None].expand(k, p)], 1).contiguous()
    return feat, cen, p


def assign_margins(dist):
    """(min [N], relative gap of the runner-up [N]; +inf where K = 1) of a float64 distance matrix."""
    if dist.shape[1] == 1:
        return dist[:, 0], torch.full_like(dist[:, 0], float("inf"))
    two = torch.topk(dist, 2, dim=1, largest=False).values
    return two[:, 0], (two[:, 1] - two[:, 0]) / two[:, 0].clamp_min(1e-300)


def accumulate_assignment(s, k, b):
    """Seeded ids [B,S,S] in [0, K) that leave cluster K - 1 empty (K = 1 has no valid assignment with an empty cluster: all 0)."""
    rs = np.random.RandomState(s * 1000 + k * 10 + b)
    return torch.from_numpy(rs.randint(0, max(k - 1, 1), size=(b, s, s)).astype(np.int32))


def tie_case():
    """Small-integer features and centres, P = 0: every fp32 product and sum below is an exact small integer, so equal float64
    distances are equal fp32 distances.  Centres 3 and 8 repeat centres 0 and 1; centres 4 / 5 are centre 2 +- the same offset in
    one channel's sign, which ties wherever the feature equals centre 2 in that channel; the small value range makes many more.
    (feat [2,6,9,9], centroids [9,6]; K = 9 runs the KP = 16 kernel with 7 padded columns of zeros -- themselves candidates for a
    wrong tie-break if the k < K guard were missing.)"""
    rs = np.random.RandomState(77)
    cen = torch.from_numpy(rs.randint(-2, 3, size=(9, 6)).astype(np.float32))
    cen[3], cen[8] = cen[0], cen[1]
    cen[4], cen[5] = cen[2], cen[2]
    cen[4, 1], cen[5, 1] = cen[2, 1] + 1, cen[2, 1] - 1
    feat = torch.from_numpy(rs.randint(-2, 3, size=(2, 6, 9, 9)).astype(np.float32))
    feat[0, :, 0, 0] = 0.0  # a pixel at the origin: ties with the zero padding unless k < K is honoured
    return feat.contiguous(), cen.contiguous()


# ---------------------------------------------------------------------------------------------------- the k-means pass kernel
# The shapes (C, P, S, K, B) at which the fused Lloyd step of csrc/kmeans.hip (w2e_kmeans_pass mode 1) is tested: even S, centres + sums
# within the LDS.  The kernel walks 128-pixel tiles, eight waves = 2 pixel halves x 4 channel quarters, 16 planes in flight.
KMEANS_STEP_SHAPES = [
    (512, 32, 16, 20, 2),  # KP = 24; D = 576 > 512: a thread of the second read owns columns t and t + 512; 2 full tiles per image
    (37, 2, 10, 8, 3),     # quarters 9/9/9/10; prefetch tail; 100 pixels per image: one partial tile, 36 live lanes in the upper half; K = KP
    (64, 4, 14, 9, 1),     # KP = 16; 196 pixels: the second tile has 68 live pixels, 4 live lanes in the upper half
    (3, 0, 6, 1, 2),       # a wave with no channel; P = 0; K = 1; 36 pixels: an upper half with no live lane
    (16, 1, 64, 32, 1),    # 32 full tiles
    (16, 1, 2, 17, 1),     # 4 pixels
    (18, 1, 12, 5, 5),     # C % 4 != 0 (quarters 4/5/4/5); 144 pixels: the second tile has 16 live pixels; 10 tiles: at grid 3 a workgroup
                           # takes tiles of different images
]
# Assignment and seeding modes: every shape of w2e_cluster_assign's test, then the step's
KMEANS_SHAPES = ASSIGN_SHAPES + [shape for shape in KMEANS_STEP_SHAPES if shape not in ASSIGN_SHAPES]
# Mode 0 beside centres that leave no room for six [64][KP] blocks of partial distances (160 KB = 40960 floats; the kernel needs
# D * KP + blocks * 64 * KP + 128 + 2 * KP): its three-block instantiations of KP = 8, 16 and 32, in which the two pixel halves of a
# tile take turns at the blocks.  (960, 32, 8, 32, 1) above is a KP = 32 case too, but its 64 pixels leave the upper half without a
# live lane and give no workgroup a second tile.  S = 14, B = 2: 196 pixels per image, a full tile and one of 68 pixels (4 live lanes in
# the upper half), 4 tiles, so that at grid 1 and 3 a workgroup reuses the blocks from tile to tile.  All three are shapes that
# w2e_cluster_assign takes.  (KP = 24 has no three-block form: (1400, 0, ., 20, .) is refused.)
KMEANS_WIDE_SHAPES = [
    (4800, 0, 14, 5, 2),    # KP = 8:  41616 floats with six blocks, 40080 with three
    (2200, 0, 14, 12, 2),   # KP = 16: 41504 / 38432
    (960, 32, 14, 32, 2),   # KP = 32: 45248 / 39104
]
KMEANS_TILE = 128
KMEANS_SEED_CANDIDATES = (1, 3, 8)


def kmeans_tiles(s, b):
    """(tiles per image, tiles, live pixels of an image's last tile)"""
    per = -(-s * s // KMEANS_TILE)
    return per, b * per, s * s - (per - 1) * KMEANS_TILE


def kmeans_kp(k):
    return 8 if k <= 8 else 16 if k <= 16 else 24 if k <= 24 else 32


def kmeans_step_fits(c, p, s, k):
    """include/w2e_attention.h, mode 1: an even S, and centres [D][KP] + six blocks of partial distances [64][KP] + the tile's ids [128] +
    [2][KP] + the running sums and counts [K][D+1], in floats, within 160 KB of LDS."""
    d, kp = c + 2 * p, kmeans_kp(k)
    return s % 2 == 0 and 4 * (d * kp + 6 * 64 * kp + KMEANS_TILE + 2 * kp + k * (d + 1)) <= 160 * 1024


def kmeans_step_run(s):
    """(length of the single-id run, length of the alternating stretch after it) of kmeans_step_labelling"""
    run = 130 if s * s > KMEANS_TILE else s * s // 2
    return run, min(32, s * s - run)


def kmeans_step_labelling(s, k, b):
    """Ids [B,S,S] for the fused step's run-length flush, per image in pixel order: one run of a single id (130 pixels -- longer than a
    tile -- where the image has more than a tile, else half the image), then 32 pixels (or what is left) that alternate between two ids,
    then seeded ids.  Cluster K - 1 is never used (K = 1: all 0; K = 2: one usable id, so no alternation)."""
    npix, usable = s * s, max(k - 1, 1)
    run, alt = kmeans_step_run(s)
    rs = np.random.RandomState(s * 1000 + k * 10 + b + 1)
    lab = rs.randint(0, usable, size=(b, npix))
    for bb in range(b):
        lab[bb, :run] = bb % usable
        lab[bb, run:run + alt] = (np.arange(alt) + bb) % 2 % usable + (usable > 2)  # ids 1, 2 (or 0, 1 of two usable ids)
    return torch.from_numpy(lab.reshape(b, s, s))


def kmeans_step_case(c, p, s, k, b):
    """assign_case with the labelling of kmeans_step_labelling, and centre K - 1 moved far away from every point (+100 in every feature
    channel): an empty cluster.  (feat [B,C,S,S], centroids [K, C+2P], the labelling [B,S,S])"""
    key = f"maskk.kmeans.step.{c}.{p}.{s}.{k}.{b}"
    protos = seeded.tensor(key + ".protos", (k, c), 1.0)
    lab = kmeans_step_labelling(s, k, b)
    feat = (protos[lab].permute(0, 3, 1, 2) + 0.25 * seeded.tensor(key + ".noise", (b, c, s, s))).contiguous()
    cen = torch.cat([protos, 0.05 * seeded.tensor(key + ".cpos", (k, 2 * p))], 1).contiguous()
    if k > 1:
        cen[k - 1, :c] += 100.0
    return feat, cen, lab


def longest_run(ids):
    """Length of the longest stretch of equal consecutive entries of a 1-D tensor."""
    change = torch.nonzero(ids[1:] != ids[:-1]).reshape(-1) + 1
    edges = torch.cat([torch.zeros(1, dtype=torch.long), change, torch.tensor([ids.numel()])])
    return int((edges[1:] - edges[:-1]).max())


def longest_alternation(ids):
    """Length of the longest stretch of a 1-D tensor in which every entry differs from the one before it."""
    best = cur = 1
    for changed in (ids[1:] != ids[:-1]).tolist():
        cur = cur + 1 if changed else 1
        best = max(best, cur)
    return best


# ---------------------------------------------------------------------------------------------------- demodulation, logits
def demod_ref(wscaled, style, eps):
    """d[b,o] = rsqrt(sum_i (wscaled[i,o] * style[b,i])^2 + eps)   (wscaled [C,32], style [B,C])"""
    return torch.rsqrt((wscaled[None] * style[:, :, None]).square().sum(1) + eps)


def logits_ref(feats, per, wl, s_last, bias_last, nw_last, initial_bias, noises, size, eps, return_pre=False):
    """include/w2e_attention.h's formulas in the dtype of the inputs (float64 in the tests), on stock ops.  `per`: (wscaled [C,32],
    style [B,C], bias [32], noise strength [1]) per source; `noises`: one [B, size*size] tensor or None per source, then
    attention_last's.  The gather is torch's nearest resize (nearest_index).  return_pre: also the list of the modulated conv sums
    [B,32,size*size] per source (w2e_attention_logits_train's `pre`)."""
    b, acts, pres = s_last.shape[0], [], []
    for j, f in enumerate(feats):
        wsc, style, bias, nw = per[4 * j:4 * j + 4]
        g = nearest_gather(f, size).reshape(b, f.shape[1], -1)
        m = torch.einsum("io,bi,bip->bop", wsc, style, g)
        pre = m * demod_ref(wsc, style, eps)[:, :, None] + bias[None, :, None]
        if noises[j] is not None:
            pre = pre + nw * noises[j][:, None, :]
        pres.append(m)
        acts.append(F.leaky_relu(pre, 0.2) * 2 ** 0.5)
    a = torch.cat(acts, 1)
    d_last = torch.rsqrt((s_last * wl).square().sum(1) + eps)
    v = (a * (wl * s_last)[:, :, None]).sum(1) * d_last[:, None] + bias_last
    if noises[-1] is not None:
        v = v + nw_last * noises[-1]
    each = torch.sigmoid(F.leaky_relu(v, 0.2) * 2 ** 0.5 + initial_bias).reshape(b, size, size)
    return (each, pres) if return_pre else each


# ---------------------------------------------------------------------------------------------------- cluster pooling
def pool_ref(each, assign, size, clusters, threshold=0.8):
    """run_attention.py:843-884 in the dtype of `each`: (final, loss_reg, loss_tv, same) of oracle/attention_net.py:99-113, with an
    assignment given at its own resolution (torch's nearest resize) that may hold ids outside [0, K)."""
    b = each.shape[0]
    choice = nearest_gather(assign.long(), size)
    same = torch.ones_like(each)
    loss_reg = each.new_zeros(1)
    for bb in range(b):
        for k in range(clusters):
            m = choice[bb] == k
            if m.any():
                mean = each[bb][m].mean()
                full = torch.zeros_like(choice, dtype=torch.bool)
                full[bb] = m
                same = torch.where(full, mean, same)
                loss_reg = loss_reg + torch.relu(mean - 0.7)
    loss_reg = loss_reg / float(b)
    loss_tv = F.mse_loss(each, same.detach())
    amap = same.unsqueeze(1)
    thr = torch.where(amap < threshold, amap - amap.detach(), amap)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(each.dtype)
    try:
        final = OA.gaussian_blur5(thr)
    finally:
        torch.set_default_dtype(prev)
    return final, loss_reg, loss_tv, same


def pool_means_ref(each, assign, size, clusters):
    """(means [B,K]: 0 for an empty cluster, counts [B,K]) in the dtype of `each`."""
    choice = nearest_gather(assign.long(), size)
    means, counts = each.new_zeros(each.shape[0], clusters), each.new_zeros(each.shape[0], clusters)
    for bb in range(each.shape[0]):
        for k in range(clusters):
            m = choice[bb] == k
            if m.any():
                means[bb, k], counts[bb, k] = each[bb][m].mean(), m.sum()
    return means, counts


# The shapes (size, csize, K, B) of the cluster_pool tests and what each one exercises.
POOL_SHAPES = [
    (128, 64, 32, 2),  # the 128 KB LDS path
    (3, 3, 1, 1),      # every tap folds
    (22, 26, 7, 2),    # a differing index (26 -> 22)
    (46, 14, 5, 1),    # a differing index (14 -> 46)
    (5, 1, 2, 3),      # single-pixel cluster map
    (64, 64, 20, 2),   # the shipped setting's size and K
]
POOL_THRESHOLD = 0.8


def pool_case(size, cs, k, b):
    """The launches [(assign int32 [B,cs,cs], each float32 [B,size,size])] of one cluster_pool shape.  `each` is a level per cluster
    (0.75 / 0.55 / 0.85 / 0.65 / 0.95 by id: both sides of 0.8, none near it) + 0.04 noise, as test_cluster_pool_bwd_vs_float64 builds
    it; cluster K - 1 is never assigned, one cluster-map pixel holds -1 and one holds K.  One launch holds all of that where the shape
    allows it.  Two shapes do not: K = 1 (an empty cluster leaves no mean) and csize = 1 with B = 3 (three ids in all); they get
    several launches that hold it between them."""
    key = f"maskk.pool.{size}.{cs}.{k}.{b}"
    levels = torch.tensor([0.75, 0.55, 0.85, 0.65, 0.95])

    def each_of(assign, salt, level_of=None):
        lv = levels[assign.long().clamp(0, k - 1) % 5] if level_of is None else level_of
        return (nearest_gather(lv, size) + 0.04 * seeded.tensor(f"{key}.each{salt}", (b, size, size))).clamp(0.01, 0.99).contiguous()

    if (size, cs, k, b) == (3, 3, 1, 1):
        mixed = torch.tensor([[[-1, 0, 0], [0, 0, 0], [0, 1, 0]]], dtype=torch.int32)
        none = torch.tensor([[[-1, 1, -1], [1, -1, 1], [-1, 1, 1]]], dtype=torch.int32)
        return [(mixed, each_of(mixed, 0, torch.full((1, 3, 3), 0.9))), (mixed, each_of(mixed, 1, torch.full((1, 3, 3), 0.5))),
                (none, each_of(none, 2, torch.full((1, 3, 3), 0.9)))]
    if (size, cs, k, b) == (5, 1, 2, 3):
        first = torch.tensor([0, -1, 0], dtype=torch.int32).reshape(3, 1, 1)
        second = torch.tensor([1, 2, 0], dtype=torch.int32).reshape(3, 1, 1)
        lv = torch.tensor([0.9, 0.6, 0.5]).reshape(3, 1, 1)
        return [(first, each_of(first, 0, lv)), (second, each_of(second, 1, lv))]
    rs = np.random.RandomState(size * 100 + cs)
    assign = torch.from_numpy(rs.randint(0, k - 1, size=(b, cs, cs)).astype(np.int32))
    idx = nearest_index(cs, size)  # (a down-sizing gather skips cluster-map pixels: put the two ids where it reads)
    assign[0, idx[0], idx[0]], assign[-1, idx[-1], idx[-2]] = -1, k
    return [(assign, each_of(assign, 0))]


def pool_boundary_case():
    """threshold 0.75 exactly: cluster 0 holds the constant 0.75 (kept: the comparison is `<`), cluster 1 the constant 0.5 (zeroed).
    Both are dyadic, so every fp32 partial sum of either is exact and so is the mean.  (assign [1,8,8], each [1,16,16], K = 2)"""
    assign = torch.zeros(1, 8, 8, dtype=torch.int32)
    assign[:, :, 5:] = 1
    each = torch.where(nearest_gather(assign, 16) == 0, 0.75, 0.5).float().contiguous()
    return assign, each, 0.75
