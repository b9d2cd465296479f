"""The offline k-means kernels of include/w2e_attention.h (csrc/kmeans.hip) through their C entry points -- w2e_kmeans_pass in its three
modes, w2e_kmeans_reduce, w2e_kmeans_plan -- against float64 restatements (tests/mask_ref.py), with the grid chosen by the test: 1 and
3 workgroups (every workgroup walks several tiles, at 3 also tiles of different images), the plan's grid, and tiles + 2 (two workgroups
get no tile).  The shapes (mask_ref.KMEANS_SHAPES / KMEANS_STEP_SHAPES) hold partial tiles, every KP instantiation, channel counts that
neither 4 nor 16 divides, a wave without a channel, P = 0, and D > 512; KMEANS_WIDE_SHAPES the centres beside which mode 0 keeps three
blocks of partial distances, not six.

Tolerances.  `mind`, `cand_dist`, the inertia and the seeding potentials: 1e-5 (helpers.rel_err; relative for the scalars), the figure
tests/test_gpu_kmeans.py holds them to.  Assignments are judged by float64 distances (mask_ref.ASSIGN_SLACK / ASSIGN_GAP; the share of
near-tied pixels is bounded on the CPU in tests/test_kmeans_host.py).  The fused step's sums have no committed figure: the same sums run
in fp32 on stock torch ops, and the kernel may sit four times as far from float64 as that does (tests/test_gpu_mask_kernels.py's rule).
They are compared by the kernel's own ids, so a near-tied pixel cannot move a sum.  Counts, ties, the finish step on small integers
and everything stated as bit-identical are exact.  Every comparison prints what it measured; profiles/kmeans_kernels_gpu_tests.log
keeps one run."""
import ctypes
import functools

import pytest
import torch

import mask_ref as R
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
NAN = float("nan")
ASSIGN, STEP, SEED = 0, 1, 2
PRELOAD = 1000.0  # what the float64 accumulator holds before w2e_kmeans_reduce adds to it


def _abi():
    from where2edit_amd import _lib as L
    from where2edit_amd import run_attention as RA
    return L, RA


def _filled(shape, value=NAN, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _same(a, b):
    """Bit-equal, NaN sentinels included."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _plan(b, c, p, s, k):
    L, _ = _abi()
    grid, fused = ctypes.c_int(-1), ctypes.c_int(-1)
    L.call("w2e_kmeans_plan", b, c, p, s, k, ctypes.byref(grid), ctypes.byref(fused))
    return grid.value, fused.value


def _grids(c, p, s, k, b):
    _, tiles, _ = R.kmeans_tiles(s, b)
    return list(dict.fromkeys([1, 3, _plan(b, c, p, s, k)[0], tiles + 2])), tiles


def _pass(mode, fg, cg, p, grid, assign=True, mind=True, cand_ld=0):
    """One launch with sentinel-filled outputs; `mind` in seeding mode is the tensor to read (or None).  Returns the device tensors
    (assign, mind, cand [8, cand_ld], partial [grid, n_out])."""
    L, RA = _abi()
    b, c, s, _ = fg.shape
    k, d = cg.shape[0], c + 2 * p
    n_out = {ASSIGN: 1, STEP: k * (d + 1) + 1, SEED: k}[mode]
    a = _filled((b, s, s), -7, torch.int32) if assign else None
    if mode == SEED:
        m, cand = mind, _filled((8, cand_ld))
    else:
        m, cand = (_filled((b, s, s)) if mind else None), None
    partial = _filled((grid, n_out))
    L.call("w2e_kmeans_pass", mode, L.ptr(fg), L.ptr(cg), None if a is None else RA._i32ptr(a), L.ptr(m), L.ptr(cand), cand_ld, L.ptr(partial),
           grid, b, c, p, s, k, L.stream_ptr())
    return a, m, cand, partial


def _reduce(partial, acc):
    L, _ = _abi()
    L.call("w2e_kmeans_reduce", L.ptr(partial), partial.shape[0], partial.shape[1], ctypes.c_void_p(acc.data_ptr()), L.stream_ptr())
    return acc


def _cluster_assign(fg, cg, p):
    L, RA = _abi()
    b, c, s, _ = fg.shape
    out = _filled((b, s, s), -7, torch.int32)
    L.call("w2e_cluster_assign", L.ptr(fg), L.ptr(cg), RA._i32ptr(out), b, c, p, s, cg.shape[0], L.stream_ptr())
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    """The inputs of one case and its float64 reference, computed once and shared (nothing below writes to them): feat, cen, p, the
    literal point matrix in float64 and in fp32, the float64 distance matrix, argmin, minimum and runner-up gap."""
    if kind == "assign":
        feat, cen = R.assign_case(*shape)
        p = shape[1]
    elif kind == "step":
        feat, cen, _ = R.kmeans_step_case(*shape)
        p = shape[1]
    elif kind == "position":
        feat, cen, p = R.position_case()
    else:
        feat, cen = R.tie_case()
        p = 0
    dist, want = R.assign_ref(feat.double(), cen.double(), p)
    best, gap = R.assign_margins(dist)
    return dict(feat=feat, cen=cen, p=p, pts=R.points_matrix(feat.double(), p), pts32=R.points_matrix(feat, p), dist=dist, want=want.reshape(-1),
                best=best, gap=gap)


def _check_assignment(what, ref, a, m, partial, tiles):
    """The criteria of an assignment (modes 0 and 1): `a`, `m` and the inertia entries `partial` [grid] of one launch."""
    k = ref["cen"].shape[0]
    ids = a.cpu().long().reshape(-1)
    assert ((ids >= 0) & (ids < k)).all(), f"{what}: ids outside [0, {k})"
    chosen = ref["dist"].gather(1, ids.reshape(-1, 1))[:, 0]
    clear = ref["gap"] > R.ASSIGN_GAP
    e_mind = rel_err(m.reshape(-1), chosen)
    want = float(chosen.sum())
    acc = _reduce(partial.reshape(-1, 1).contiguous(), torch.full((1,), PRELOAD, dtype=torch.float64, device=DEV))
    e_inertia = abs(float(acc[0]) - PRELOAD - want) / want
    print(f"  {what}: worst chosen / minimum - 1 = {float((chosen / ref['best']).max() - 1):.3e}; {int((~clear).sum())} of {clear.numel()} pixels within "
          f"{R.ASSIGN_GAP:g} of a tie; ids differing from argmin {int((ids != ref['want']).sum())}; mind rel err {e_mind:.3e}; inertia rel err {e_inertia:.3e}")
    assert (chosen <= (1 + R.ASSIGN_SLACK) * ref["best"]).all(), what
    assert torch.equal(ids[clear], ref["want"][clear]), what
    assert e_mind <= TOL, f"{what}: mind rel err {e_mind:.3e}"
    assert e_inertia <= TOL, f"{what}: inertia rel err {e_inertia:.3e}"
    assert (partial[tiles:] == 0).all(), f"{what}: a workgroup without a tile wrote a non-zero partial row"
    return ids


def _assign_mode(kind, shape):
    ref = _case(kind, shape)
    feat, cen, p = ref["feat"], ref["cen"], ref["p"]
    (b, c, s, _), k = feat.shape, cen.shape[0]
    fg, cg = feat.to(DEV), cen.to(DEV)
    grids, tiles = _grids(c, p, s, k, b)
    print(f"kmeans_pass mode 0, {kind} case C {c} P {p} S {s} K {k} B {b}: {tiles} tiles, grids {grids}")
    first = None
    for grid in grids:
        a, m, _, partial = _pass(ASSIGN, fg, cg, p, grid)
        _check_assignment(f"grid {grid}", ref, a, m, partial[:, 0], tiles)
        if first is None:
            first = (a, m)
            assert torch.equal(a, _cluster_assign(fg, cg, p)), "mode 0 is not w2e_cluster_assign bit for bit"
        assert torch.equal(a, first[0]) and _same(m, first[1]), f"grid {grid}: assign / mind differ from grid {grids[0]}'s"
        a2, m2, _, partial2 = _pass(ASSIGN, fg, cg, p, grid, assign=False)
        assert a2 is None and _same(m2, m) and _same(partial2, partial), f"grid {grid}: assign = NULL changed mind or the partials"
        a3, m3, _, partial3 = _pass(ASSIGN, fg, cg, p, grid, mind=False)
        assert m3 is None and torch.equal(a3, a) and _same(partial3, partial), f"grid {grid}: mind = NULL changed assign or the partials"
    return first[0].cpu().long(), ref


# ---------------------------------------------------------------------------------------------------- mode 0: assignment
@pytest.mark.parametrize("c,p,s,k,b", R.KMEANS_SHAPES)
def test_assign_mode_vs_float64(c, p, s, k, b):
    """(960, 32, 8, 32, 1) is D = 1024 at K = 32: 128 KB of centres, which leave room for three blocks of partial distances, not six
    -- the kernel's three-block form (as first written, w2e_kmeans_pass refused this shape, which w2e_cluster_assign takes)."""
    _assign_mode("assign", (c, p, s, k, b))


@pytest.mark.parametrize("c,p,s,k,b", R.KMEANS_WIDE_SHAPES)
def test_assign_mode_three_block_form_vs_float64(c, p, s, k, b):
    """The three-block instantiations of KP = 8, 16 and 32, in which the pixel halves of a tile take turns at the blocks: 4 tiles of 128
    and 68 pixels (tests/test_kmeans_host.py), so both halves hold live pixels, the upper one dead lanes too, and at grid 1 and 3 a
    workgroup reuses the blocks from tile to tile.  Every criterion of test_assign_mode_vs_float64, the bit-identity with
    w2e_cluster_assign included."""
    _assign_mode("assign", (c, p, s, k, b))


def test_assign_mode_where_only_the_position_channels_decide():
    _assign_mode("position", None)


def test_assign_mode_breaks_exact_ties_like_argmin():
    ids, ref = _assign_mode("ties", None)
    tied = (ref["dist"] == ref["dist"].min(1, keepdim=True).values).sum(1) > 1
    print(f"  exact ties: {int(tied.sum())} tied pixels of {tied.numel()}; ids differing from torch.argmin: {int((ids.reshape(-1) != ref['want']).sum())}")
    assert tied.sum() > 0 and torch.equal(ids.reshape(-1), ref["want"])


# ---------------------------------------------------------------------------------------------------- mode 1: the fused Lloyd step
@pytest.mark.parametrize("kind", ["assign", "step"])
@pytest.mark.parametrize("c,p,s,k,b", R.KMEANS_STEP_SHAPES)
def test_step_mode_vs_float64(c, p, s, k, b, kind):
    """kind "assign": mask_ref.assign_case, whose seeded labels change at nearly every pixel and use every cluster.  kind "step":
    mask_ref.kmeans_step_case -- a run longer than a tile, an alternation, cluster K - 1 empty (tests/test_kmeans_host.py)."""
    ref = _case(kind, (c, p, s, k, b))
    feat, cen = ref["feat"], ref["cen"]
    d, n = c + 2 * p, b * s * s
    fg, cg = feat.to(DEV), cen.to(DEV)
    grids, tiles = _grids(c, p, s, k, b)
    assert _plan(b, c, p, s, k)[1] == 1
    print(f"kmeans_pass mode 1, {kind} case C {c} P {p} S {s} K {k} B {b}: {tiles} tiles, grids {grids}")
    sums_first = bound = None
    for grid in grids:
        a, m, _, partial = _pass(STEP, fg, cg, p, grid)
        ids = _check_assignment(f"grid {grid}", ref, a, m, partial[:, k * (d + 1)], tiles)
        a0, m0, _, partial0 = _pass(ASSIGN, fg, cg, p, grid)
        assert torch.equal(a, a0) and _same(m, m0) and _same(partial[:, k * (d + 1)], partial0[:, 0]), f"grid {grid}: not mode 0's assignment / inertia"
        again = _pass(STEP, fg, cg, p, grid)
        assert _same(again[3], partial) and torch.equal(again[0], a) and _same(again[1], m), f"grid {grid}: a second run differs"
        table = _reduce(partial, torch.zeros(k * (d + 1) + 1, dtype=torch.float64, device=DEV))[:k * (d + 1)].view(k, d + 1).cpu()
        sums, counts = table[:, :d], table[:, d]
        want_counts = torch.bincount(ids, minlength=k).double()
        assert torch.equal(counts, want_counts) and counts.sum() == n, f"grid {grid}: counts {counts.tolist()} against bincount {want_counts.tolist()}"
        want = torch.zeros(k, d, dtype=torch.float64).index_add_(0, ids, ref["pts"])  # by the kernel's own ids
        stock = torch.zeros(k, d).index_add_(0, ids, ref["pts32"])
        dk, dt = rel_err(sums, want), rel_err(stock, want)
        print(f"  grid {grid}: sums: kernel {dk:.3e}, stock torch ops in fp32 {dt:.3e} from float64; counts exact, {int((counts == 0).sum())} empty")
        assert dk <= 4 * dt, f"grid {grid}: sums: kernel {dk:.3e} > 4 x {dt:.3e}"
        assert (sums[counts == 0] == 0).all(), f"grid {grid}: an empty cluster has a non-zero sum"
        assert (partial[tiles:] == 0).all(), f"grid {grid}: a workgroup without a tile wrote a non-zero partial row"
        if sums_first is None:
            sums_first, bound = sums, 4 * dt
        else:
            e = rel_err(sums, sums_first)
            print(f"  grid {grid}: sums against grid {grids[0]}'s: rel err {e:.3e}")
            assert e <= bound, f"grid {grid}: sums differ from grid {grids[0]}'s by {e:.3e} > {bound:.3e}"
    if kind == "step" and k > 1:
        assert counts[k - 1] == 0  # the centre placed far away


# ---------------------------------------------------------------------------------------------------- mode 2: the seeding pass
@pytest.mark.parametrize("c,p,s,k,b", R.KMEANS_SHAPES)
def test_seed_mode_vs_float64(c, p, s, k, b):
    """T = 1, 3, 8 candidates = rows of the literal fp32 point matrix (repeated where the case has fewer than T points), `mind` NULL
    (the first round: +inf) and given, cand_ld = B*S*S + 5."""
    ref = _case("assign", (c, p, s, k, b))
    n, ld = b * s * s, b * s * s + 5
    fg = ref["feat"].to(DEV)
    grids, tiles = _grids(c, p, s, 8, b)
    given = ((ref["pts"] - ref["pts"][n // 2]) ** 2).sum(1).float()  # fp32 distances to one point: the minimum falls on both sides
    print(f"kmeans_pass mode 2, C {c} P {p} S {s} B {b}: {tiles} tiles, grids {grids}")
    for t in R.KMEANS_SEED_CANDIDATES:
        rows = torch.linspace(0, n - 1, t).round().long()
        cand = ref["pts32"][rows].contiguous()
        d64 = ((ref["pts"][:, None, :] - cand.double()[None, :, :]) ** 2).sum(-1)  # [N, T]
        cg = cand.to(DEV)
        for mind in (None, given):
            mg = None if mind is None else mind.to(DEV)
            want = (d64 if mind is None else torch.minimum(mind.double()[:, None], d64)).sum(0)
            first = None
            for grid in grids:
                _, _, planes, partial = _pass(SEED, fg, cg, p, grid, assign=False, mind=mg, cand_ld=ld)
                e_cand = rel_err(planes[:t, :n], d64.t())
                pots = _reduce(partial, torch.full((t,), PRELOAD, dtype=torch.float64, device=DEV)).cpu() - PRELOAD
                e_pot = float(((pots - want).abs() / want).max())
                print(f"  T {t} mind {'NULL' if mind is None else 'given'} grid {grid}: cand_dist rel err {e_cand:.3e}; potentials worst rel err {e_pot:.3e}")
                assert e_cand <= TOL and e_pot <= TOL
                assert torch.isnan(planes[:, n:]).all() and torch.isnan(planes[t:]).all(), "written beyond B*S*S columns or T planes"
                assert mg is None or torch.equal(mg.cpu(), mind), "mind was written"
                assert (partial[tiles:] == 0).all()
                first = planes if first is None else first
                assert _same(planes, first), f"grid {grid}: cand_dist differs from grid {grids[0]}'s"


# ---------------------------------------------------------------------------------------------------- w2e_kmeans_reduce
def test_reduce_adds_the_rows_in_double_onto_what_acc_holds():
    """Small integers: every float64 partial sum is exact, so the result is the float64 sum whatever the order -- and equal, not close."""
    L, _ = _abi()
    gen = torch.Generator().manual_seed(5)
    for n in (1, 256, 257, 600):
        start = torch.randint(-50, 50, (n,), generator=gen).double()
        for rows in (1, 3, 37):
            partial = torch.randint(-9, 10, (rows, n), generator=gen).float()
            acc = _reduce(partial.to(DEV), start.to(DEV))
            assert torch.equal(acc.cpu(), start + partial.double().sum(0)), (n, rows)
        kept = start.to(DEV)
        dummy = _filled((1, n))
        L.call("w2e_kmeans_reduce", L.ptr(dummy), 0, n, ctypes.c_void_p(kept.data_ptr()), L.stream_ptr())
        assert torch.equal(kept.cpu(), start), f"rows = 0 changed acc (n {n})"
    print("kmeans_reduce: n 1 / 256 / 257 / 600 x rows 1 / 3 / 37 equal the float64 sums (rel err 0.000e+00); rows = 0 leaves acc")


# ---------------------------------------------------------------------------------------------------- w2e_kmeans_plan
def test_plan_grid_and_fused():
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    shapes = list(R.KMEANS_SHAPES) + [(512, 32, 16, 24, 1), (512, 32, 16, 25, 1),  # D = 576: 148256 B against 181348 B
                                      (512, 32, 17, 20, 1),                        # an odd S
                                      (890, 0, 8, 16, 0),                          # no image: one workgroup
                                      (16, 1, 128, 6, 3), (16, 1, 128, 6, 300),    # 384 and 38400 tiles: more than CUs
                                      (16, 1, 2, 8, cus - 1), (16, 1, 2, 8, cus), (16, 1, 2, 8, cus + 1)]
    both = set()
    for c, p, s, k, b in shapes:
        grid, fused = _plan(b, c, p, s, k)
        _, tiles, _ = R.kmeans_tiles(s, b)
        want = R.kmeans_step_fits(c, p, s, k)
        print(f"kmeans_plan C {c} P {p} S {s} K {k} B {b}: grid {grid} ({tiles} tiles, {cus} CUs), fused {fused} (formula {int(want)})")
        assert grid == max(1, min(tiles, cus)) and fused == int(want)
        both.add(fused)
    assert both == {0, 1}


# ---------------------------------------------------------------------------------------------------- refusals
def test_limits_are_refused_before_the_launch():
    L, RA = _abi()
    #         mode  C    P   S  K   grid  cand_ld  feat offset (floats)  message
    cases = [(ASSIGN, 16, 1, 8, 33, 2, 0, 0, "clusters <= 32"),
             (SEED, 16, 1, 8, 9, 2, 64, 0, "clusters <= 8"),
             (SEED, 16, 1, 8, 3, 2, 63, 0, "ld >= B\\*S\\*S"),
             (STEP, 16, 1, 9, 6, 2, 0, 0, "even size"),
             (STEP, 16, 1, 8, 6, 2, 0, 1, "16-byte aligned"),
             (STEP, 512, 32, 8, 32, 2, 0, 0, "of LDS"),
             (ASSIGN, 1100, 0, 8, 32, 2, 0, 0, "of LDS"),  # beyond the three-block form too
             (ASSIGN, 1400, 0, 8, 20, 2, 0, 0, "of LDS"),  # KP = 24 has no three-block form (w2e_cluster_assign stops at D = 1024 there)
             (ASSIGN, 16, 1, 8, 6, 0, 0, 0, "grid 0"),
             (ASSIGN, 16, 1, 8, 6, 4097, 0, 0, "grid 4097"),
             (3, 16, 1, 8, 6, 2, 0, 0, "mode 3"),
             (-1, 16, 1, 8, 6, 2, 0, 0, "mode -1")]
    for mode, c, p, s, k, grid, ld, offset, message in cases:
        d = c + 2 * p
        feat = torch.zeros(c * s * s + 4, device=DEV)[offset:offset + c * s * s].view(1, c, s, s)
        assert feat.data_ptr() % 16 == 4 * offset
        cen = torch.zeros(k, d, device=DEV)
        a, m, cand, partial = _filled((1, s, s), -7, torch.int32), _filled((1, s, s)), _filled((8, 64)), _filled((4, k * (d + 1) + 1))
        with pytest.raises(RuntimeError, match=message):
            L.call("w2e_kmeans_pass", mode, L.ptr(feat), L.ptr(cen), RA._i32ptr(a), L.ptr(m), L.ptr(cand), ld, L.ptr(partial), grid, 1, c, p, s, k,
                   L.stream_ptr())
        torch.cuda.synchronize()
        assert (a == -7).all() and torch.isnan(m).all() and torch.isnan(cand).all() and torch.isnan(partial).all(), f"{message}: something ran"
        print(f"kmeans_pass refuses mode {mode} C {c} P {p} S {s} K {k} grid {grid} cand_ld {ld} feat offset {offset}: '{message}'")
