"""The region-mask kernels of include/w2e_attention.h (csrc/attention.hip), one entry point at a time, against the float64 restatements
of tests/mask_ref.py: w2e_cluster_assign, w2e_cluster_accumulate, w2e_attention_demod, w2e_attention_logits (and the bit-identity and
`pre` of w2e_attention_logits_train) and w2e_cluster_pool, each called through its C entry point at the shapes where a kernel can go
wrong -- every KP instantiation, channel counts that no wave split or chunk divides, dead lanes, the LDS limits, NULL arguments, and
resize ratios (26 -> 22, 14 -> 46) at which torch's nearest index is not floor(dst * in / out).

Tolerances.  `each`, `same`, `thr`, `final` and `pre`: 1e-4 in helpers.rel_err, the figure this branch's tests state (TOL in
tests/test_gpu_attention_train.py).  `means`, `demod` and `partial` have no committed figure: the same operation runs in fp32 on stock
torch ops, and the kernel may sit four times as far from float64 as that does (tests/test_gpu_adam.py's rule: the order of summation
is the only legitimate difference).  Assignments are judged by float64 distances (mask_ref.ASSIGN_SLACK / ASSIGN_GAP; the share of
near-tied pixels is bounded on the CPU in tests/test_mask_ref_host.py).  Counts and ties are exact.  Every comparison prints what it
measured; profiles/mask_kernels_gpu_tests.log keeps one run."""
import pytest
import torch

import mask_ref as R
import seeded
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
NAN = float("nan")


def _abi():
    from where2edit_amd import _lib as L
    from where2edit_amd import run_attention as RA
    return L, RA


def _close(a, b, what):
    e = rel_err(a, b)
    print(f"  {what}: rel err {e:.3e}")
    assert e <= TOL, f"{what}: rel err {e:.3e} > {TOL:.0e}"


def _elementwise(a, b):
    """max |a - b| / |b|: for outputs whose entries differ by orders of magnitude (a demodulation row of rsqrt(eps) = 1e4)."""
    a, b = a.double().cpu(), b.double().cpu()
    return float(((a - b).abs() / b.abs()).max())


def _within_four_times_torch_fp32(kernel, torch32, ref64, what, err=rel_err):
    dk, dt = err(kernel, ref64), err(torch32, ref64)
    print(f"  {what}: kernel {dk:.3e}, stock torch ops in fp32 {dt:.3e} from float64 (helpers.rel_err: kernel {rel_err(kernel, ref64):.3e})")
    assert dk <= 4 * dt, f"{what}: kernel {dk:.3e} > 4 x {dt:.3e}"


def _filled(shape, value=NAN, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------- w2e_cluster_assign
def _assign(feat, cen, p, k):
    L, RA = _abi()
    b, c, s, _ = feat.shape
    out = _filled((b, s, s), -7, torch.int32)
    fg, cg = feat.to(DEV), cen.to(DEV)  # (named: a temporary is freed, and its block reused, as soon as its pointer is taken)
    L.call("w2e_cluster_assign", L.ptr(fg), L.ptr(cg), RA._i32ptr(out), b, c, p, s, k, L.stream_ptr())
    return out.cpu().long()


@pytest.mark.parametrize("c,p,s,k,b", R.ASSIGN_SHAPES)
def test_cluster_assign_vs_float64(c, p, s, k, b):
    """The chosen centre is within 1e-5 (relative) of the nearest in float64 for every pixel, and is the float64 argmin wherever the
    runner-up is more than 1e-4 away.  (960, 32, 8, 32, 1) is D = 1024 with K = 32: exactly the documented 160 KB of LDS."""
    feat, cen = R.assign_case(c, p, s, k, b)
    dist, want = R.assign_ref(feat.double(), cen.double(), p)
    got = _assign(feat, cen, p, k)
    assert ((got >= 0) & (got < k)).all()
    best, gap = R.assign_margins(dist)
    chosen = dist.gather(1, got.reshape(-1, 1))[:, 0]
    clear = gap > R.ASSIGN_GAP
    print(f"cluster_assign C {c} P {p} S {s} K {k} B {b}: distance to the chosen centre vs the float64 minimum: rel err "
          f"{rel_err(chosen, best):.3e}, worst ratio - 1 = {float((chosen / best).max() - 1):.3e}; {int((~clear).sum())} of {clear.numel()} "
          f"pixels within {R.ASSIGN_GAP:g} of a tie; ids differing from argmin: {int((got.reshape(-1) != want.reshape(-1)).sum())}")
    assert (chosen <= (1 + R.ASSIGN_SLACK) * best).all()
    assert torch.equal(got.reshape(-1)[clear], want.reshape(-1)[clear])


def test_cluster_assign_where_only_the_position_channels_decide():
    """mask_ref.position_case under the criteria of test_cluster_assign_vs_float64: the centres differ in their position parts only."""
    feat, cen, p = R.position_case()
    dist, want = R.assign_ref(feat.double(), cen.double(), p)
    got = _assign(feat, cen, p, cen.shape[0])
    best, gap = R.assign_margins(dist)
    chosen = dist.gather(1, got.clamp(0, cen.shape[0] - 1).reshape(-1, 1))[:, 0]
    clear = gap > R.ASSIGN_GAP
    print(f"cluster_assign, position channels only: distance to the chosen centre vs the float64 minimum: rel err {rel_err(chosen, best):.3e}; "
          f"ids differing from argmin: {int((got != want).sum())} of {want.numel()}")
    assert ((got >= 0) & (got < cen.shape[0])).all()
    assert (chosen <= (1 + R.ASSIGN_SLACK) * best).all()
    assert torch.equal(got.reshape(-1)[clear], want.reshape(-1)[clear])


def test_cluster_assign_breaks_exact_ties_like_argmin():
    feat, cen = R.tie_case()
    dist, want = R.assign_ref(feat.double(), cen.double(), 0)
    got = _assign(feat, cen, 0, cen.shape[0])
    tied = (dist == dist.min(1, keepdim=True).values).sum(1) > 1
    print(f"cluster_assign, exact ties: {int(tied.sum())} tied pixels of {tied.numel()}; ids differing from torch.argmin: "
          f"{int((got != want).sum())}; rel err of the ids {rel_err(got, want):.3e}")
    assert torch.equal(got, want)


def test_cluster_assign_limits_are_refused_before_the_launch():
    L, RA = _abi()
    for c, p, k, message in ((964, 32, 32, "LDS"), (16, 1, 33, "clusters <= 32")):  # D = 1028 at K = 32: 164352 B;  K = 33
        feat, cen = torch.zeros(1, c, 8, 8, device=DEV), torch.zeros(k, c + 2 * p, device=DEV)
        out = _filled((1, 8, 8), -7, torch.int32)
        with pytest.raises(RuntimeError, match=message):
            L.call("w2e_cluster_assign", L.ptr(feat), L.ptr(cen), RA._i32ptr(out), 1, c, p, 8, k, L.stream_ptr())
        torch.cuda.synchronize()
        assert (out == -7).all()  # nothing ran


# ---------------------------------------------------------------------------------------------------- w2e_cluster_accumulate
@pytest.mark.parametrize("c,p,s,k,b", R.ASSIGN_SHAPES[:-1])
def test_cluster_accumulate_vs_float64(c, p, s, k, b):
    L, RA = _abi()
    feat, _ = R.assign_case(c, p, s, k, b)
    assign = R.accumulate_assignment(s, k, b)
    partial_o, counts_o = R.accumulate_ref(feat.double(), assign, p, k)
    partial_t, _ = R.accumulate_ref(feat, assign, p, k)
    fg, ag = feat.to(DEV), assign.to(DEV)
    runs = []
    for _ in range(2):
        partial, counts = _filled((b, k, c + 2 * p)), _filled((b, k))  # written, not accumulated
        L.call("w2e_cluster_accumulate", L.ptr(fg), RA._i32ptr(ag), L.ptr(partial), L.ptr(counts), b, c, p, s, k, L.stream_ptr())
        runs.append((partial.cpu(), counts.cpu()))
    (partial, counts), again = runs
    print(f"cluster_accumulate C {c} P {p} S {s} K {k} B {b}: counts rel err {rel_err(counts, counts_o):.3e}")
    assert torch.equal(counts.double(), counts_o) and counts.sum() == b * s * s
    if k > 1:
        assert (counts[:, k - 1] == 0).all() and (partial[:, k - 1] == 0).all()  # the empty cluster
    _within_four_times_torch_fp32(partial, partial_t, partial_o, "partial")
    assert torch.equal(partial, again[0]) and torch.equal(counts, again[1])  # fixed-order sums: bit-identical


# ---------------------------------------------------------------------------------------------------- w2e_attention_demod
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 32])
def test_attention_demod_vs_float64(n, batch):
    """Channel counts 512 / 1 / 7 / 40 in turn within one launch (1 and 7: fewer channels than the kernel's 8 channel residues).  With
    batch 3, sample 1 of source 0 has an all-zero style: rsqrt(eps) = 1e4 next to entries of order 1, hence the elementwise relative
    error.  (With batch 1 a zero row would be the whole output of n = 1, where stock torch is exact and leaves no distance to scale.)"""
    L, RA = _abi()
    eps = 1e-8
    chans = [(512, 1, 7, 40)[j % 4] for j in range(n)]
    ws = [seeded.tensor(f"maskk.demod.w{j}", (c, 32), 1.0 / c ** 0.5) for j, c in enumerate(chans)]
    st = [seeded.tensor(f"maskk.demod.s{j}.{batch}", (batch, c), 0.5, 1.0) for j, c in enumerate(chans)]
    if batch > 1:
        st[0][1] = 0.0
    out = _filled((n, batch, 32))
    keep = [(w.to(DEV), s.to(DEV)) for w, s in zip(ws, st)]
    descs = (RA._AttSource * n)()
    for j, (w, s) in enumerate(keep):
        descs[j].wscaled, descs[j].style, descs[j].demod, descs[j].channels = L.ptr(w).value, L.ptr(s).value, L.ptr(out[j]).value, chans[j]
    L.call("w2e_attention_demod", descs, n, batch, eps, L.stream_ptr())
    ref = torch.stack([R.demod_ref(w.double(), s.double(), eps) for w, s in zip(ws, st)])
    t32 = torch.stack([R.demod_ref(w, s, eps) for w, s in zip(ws, st)])
    print(f"attention_demod n {n} B {batch} channels {sorted(set(chans))}")
    _within_four_times_torch_fp32(out, t32, ref, "demod (elementwise relative)", _elementwise)
    if batch > 1:
        assert _elementwise(out[0, 1], torch.full((32,), eps ** -0.5)) <= 1e-6  # the zero row: rsqrt(eps), within a few fp32 ulps


# ---------------------------------------------------------------------------------------------------- w2e_attention_logits
LOGITS_CASES = [
    (16, 2, ((512, 4), (256, 32), (32, 16), (3, 64), (129, 16), (128, 1))),  # C > 128 with a tail (129); C < 32; res 1; res 4..64
    (22, 3, ((40, 26), (8, 5))),                                             # 26 -> 22: a differing index
    (46, 1, ((8, 14), (16, 92))),                                            # 14 -> 46: a differing index; 2116 pixels: a tile tail
    (1, 2, ((8, 4),)),                                                       # a single output pixel
    (8, 2, ((8, 8),) * 32),                                                  # W2E_ATT_MAX_SOURCES
]


@pytest.mark.parametrize("size,batch,shapes", LOGITS_CASES, ids=lambda v: str(v) if isinstance(v, int) else f"{len(v)}src")
def test_attention_logits_vs_float64(size, batch, shapes):
    """`each` of the forward-only entry point with noise_last NULL and non-NULL; sources alternate NULL / non-NULL noise (a lone source
    has noise), every strength non-zero.  i.i.d. features: one wrong source pixel is an O(1) error in `pre`.  The train entry point
    returns the same `each` bit for bit and the float64 `pre`."""
    L, RA = _abi()
    n, eps, npix = len(shapes), 1e-8, size * size
    t = lambda name, shape, scale=1.0, shift=0.0: seeded.tensor(f"maskk.logits{size}.{name}", shape, scale, shift)  # noqa: E731
    feats = [t(f"f{j}", (batch, c, r, r)) for j, (c, r) in enumerate(shapes)]
    per = []
    for j, (c, r) in enumerate(shapes):
        per += [t(f"w{j}", (c, 32), 1.0 / c ** 0.5), t(f"s{j}", (batch, c), 0.5, 1.0), t(f"b{j}", (32,), 0.3), t(f"nw{j}", (1,), 0.05, 0.3)]
    wl, sl, bl, nwl, ib = (t("wl", (32 * n,), 1.0 / (32 * n) ** 0.5), t("sl", (batch, 32 * n), 0.5, 1.0), t("bl", (1,), 0.2), t("nwl", (1,), 0.05, 0.4),
                           t("ib", (1,), 0.1, 0.6))
    noises = [t(f"noise{j}", (batch, npix)) if (n == 1 or j % 2) else None for j in range(n)]
    assert all(float(per[4 * j + 3].abs()) > 0.05 for j in range(n)) and float(nwl.abs()) > 0.05
    assert n == 1 or (any(z is None for z in noises) and any(z is not None for z in noises))
    dbl = lambda x: None if x is None else x.double()  # noqa: E731
    demods = [R.demod_ref(per[4 * j].double(), per[4 * j + 1].double(), eps).float() for j in range(n)]  # an input of this entry point
    d_last = torch.rsqrt((sl.double() * wl.double()).square().sum(1) + eps).float()
    dev = lambda x: None if x is None else x.to(DEV).contiguous()  # noqa: E731
    g_feats, g_per, g_noises, g_demods = [dev(f) for f in feats], [dev(x) for x in per], [dev(z) for z in noises], [dev(d) for d in demods]
    g_wl, g_sl, g_bl, g_nwl, g_ib, g_dl = (dev(x) for x in (wl, sl, bl, nwl, ib, d_last))
    descs = (RA._AttSource * n)()
    for j, (c, r) in enumerate(shapes):
        d = descs[j]
        d.feat, d.wscaled, d.style, d.demod, d.bias = (L.ptr(x).value for x in (g_feats[j], g_per[4 * j], g_per[4 * j + 1], g_demods[j], g_per[4 * j + 2]))
        d.noise = None if g_noises[j] is None else L.ptr(g_noises[j]).value
        d.noise_w, d.channels, d.res = L.ptr(g_per[4 * j + 3]).value, c, r
    print(f"attention_logits size {size} B {batch} sources {shapes if n <= 6 else (n, shapes[0])}")
    for noise_last in (None, t("noise_last", (batch, npix))):
        each_o, pre_o = R.logits_ref([f.double() for f in feats], [x.double() for x in per], wl.double(), sl.double(), bl.double(), nwl.double(),
                                     ib.double(), [dbl(z) for z in noises] + [dbl(noise_last)], size, eps, return_pre=True)
        g_nl = dev(noise_last)
        partial, each = _filled((n, batch, npix)), _filled((batch, size, size))
        L.call("w2e_attention_logits", descs, n, L.ptr(g_wl), L.ptr(g_sl), L.ptr(g_dl), L.ptr(g_bl), L.ptr(g_nl), L.ptr(g_nwl), L.ptr(g_ib),
               L.ptr(partial), L.ptr(each), batch, size, L.stream_ptr())
        tag = "noise_last NULL" if noise_last is None else "noise_last given"
        _close(each, each_o, f"each ({tag})")
        partial2, each2, pre = _filled((n, batch, npix)), _filled((batch, size, size)), _filled((n, batch, 32, npix))
        L.call("w2e_attention_logits_train", descs, n, L.ptr(g_wl), L.ptr(g_sl), L.ptr(g_dl), L.ptr(g_bl), L.ptr(g_nl), L.ptr(g_nwl), L.ptr(g_ib),
               L.ptr(partial2), L.ptr(each2), L.ptr(pre), batch, size, L.stream_ptr())
        assert torch.equal(each2, each) and torch.equal(partial2, partial), "the train entry point's `each` is not the forward's"
        _close(pre, torch.stack(pre_o), f"pre ({tag})")


# ---------------------------------------------------------------------------------------------------- w2e_cluster_pool
def _pool(each, assign, size, k, threshold, with_thr=True):
    L, RA = _abi()
    b, cs = each.shape[0], assign.shape[1]
    same, means, counts, final = _filled((b, size, size)), _filled((b, k)), _filled((b, k)), _filled((b, 1, size, size))
    thr = _filled((b, 1, size, size)) if with_thr else None
    eg, ag = each.to(DEV), assign.to(DEV)
    L.call("w2e_cluster_pool", L.ptr(eg), RA._i32ptr(ag), L.ptr(same), L.ptr(means), L.ptr(counts), L.ptr(thr), L.ptr(final),
           b, size, cs, k, float(threshold), L.stream_ptr())
    return same.cpu(), means.cpu(), counts.cpu(), None if thr is None else thr.cpu(), final.cpu()


@pytest.mark.parametrize("size,cs,k,b", R.POOL_SHAPES)
def test_cluster_pool_vs_float64(size, cs, k, b):
    """Every launch of mask_ref.pool_case (tests/test_mask_ref_host.py shows on the CPU that they hold an empty cluster, ids -1 and K
    and means on both sides of 0.8, none within 1e-3 of it)."""
    print(f"cluster_pool size {size} csize {cs} K {k} B {b}")
    for i, (assign, each) in enumerate(R.pool_case(size, cs, k, b)):
        final_o, _, _, same_o = R.pool_ref(each.double(), assign, size, k, R.POOL_THRESHOLD)
        means_o, counts_o = R.pool_means_ref(each.double(), assign, size, k)
        means_t, _ = R.pool_means_ref(each, assign, size, k)
        thr_o = torch.where(same_o < R.POOL_THRESHOLD, 0.0, same_o).unsqueeze(1)
        same, means, counts, thr, final = _pool(each, assign, size, k, R.POOL_THRESHOLD)
        print(f" launch {i}: counts rel err {rel_err(counts, counts_o):.3e}")
        assert torch.equal(counts.double(), counts_o)
        choice = R.nearest_gather(assign.long(), size)
        outside = (choice < 0) | (choice >= k)
        assert (same[outside] == 1.0).all() and counts.sum() == (~outside).sum()  # out-of-range ids: 1.0, counted nowhere
        assert (means[counts == 0] == 0).all()                                    # empty clusters: mean 0
        _close(same, same_o, "same"), _close(thr, thr_o, "thr"), _close(final, final_o, "final")
        if (counts > 0).any():
            _within_four_times_torch_fp32(means, means_t, means_o, "means")
        same2, means2, counts2, _, final2 = _pool(each, assign, size, k, R.POOL_THRESHOLD, with_thr=False)
        assert torch.equal(same2, same) and torch.equal(means2, means) and torch.equal(counts2, counts) and torch.equal(final2, final), "thr = NULL"


def test_cluster_pool_keeps_a_mean_that_equals_the_threshold():
    assign, each, threshold = R.pool_boundary_case()
    same, means, counts, thr, final = _pool(each, assign, 16, 2, threshold)
    choice = R.nearest_gather(assign.long(), 16)
    want = torch.where(choice == 0, 0.75, 0.5).float()
    assert torch.equal(means, torch.tensor([[0.75, 0.5]])) and torch.equal(counts, torch.tensor([[160.0, 96.0]]))
    assert torch.equal(same, want)
    assert torch.equal(thr[:, 0], torch.where(choice == 0, 0.75, 0.0).float())  # 0.75 < 0.75 is false: kept; 0.5 is zeroed
    final_o = R.pool_ref(each.double(), assign, 16, 2, threshold)[0]
    print("cluster_pool, a mean equal to the threshold")
    _close(final, final_o, "final")
