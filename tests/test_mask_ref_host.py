"""CPU checks of tests/mask_ref.py, the float64 restatements that tests/test_gpu_mask_kernels.py holds the region-mask kernels to:
torch's nearest-resize index against both closed forms, the restatement against oracle/attention_net.py on the seeded fixture inputs,
and the conditions on the seeded inputs that the GPU tests rely on (few near-ties in the assignment cases, exact ties in the tie
case, cluster means well away from the threshold)."""
import math

import numpy as np
import pytest
import torch

import make_golden_attention as M
import mask_ref as R
import mask_train_common as C
from helpers import rel_err
from oracle import attention_net as OA
from oracle import ops as OO


def _fp32_formula(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, n_in - 1))


def _integer_formula(n_in, n_out):
    return (torch.arange(n_out) * n_in) // n_out


def test_nearest_index_is_the_fp32_formula_for_every_pair_up_to_130():
    differing = 0
    for n_in in range(1, 131):
        for n_out in range(1, 131):
            idx = R.nearest_index(n_in, n_out)
            assert torch.equal(idx, _fp32_formula(n_in, n_out)), (n_in, n_out)
            differing += int(not torch.equal(idx, _integer_formula(n_in, n_out)))
    print(f"pairs in, out <= 130 at which floor(dst * in / out) is not torch's index: {differing}")
    assert differing > 0


def test_nearest_index_is_the_integer_formula_at_every_power_of_two_pair():
    for n_in in (2 ** i for i in range(0, 11)):
        for n_out in (2 ** i for i in range(0, 8)):
            assert torch.equal(R.nearest_index(n_in, n_out), _integer_formula(n_in, n_out)), (n_in, n_out)


@pytest.mark.parametrize("n_in,n_out,dst,torch_src,integer_src", [(26, 22, 11, 12, 13), (14, 46, 23, 6, 7)])
def test_nearest_index_differs_from_the_integer_formula_where_the_gpu_tests_need_it(n_in, n_out, dst, torch_src, integer_src):
    assert int(R.nearest_index(n_in, n_out)[dst]) == torch_src
    assert int(_integer_formula(n_in, n_out)[dst]) == integer_src
    x = torch.arange(n_in * n_in, dtype=torch.float32).reshape(1, 1, n_in, n_in)
    assert torch.equal(R.nearest_gather(x, n_out), torch.nn.functional.interpolate(x, n_out))


def test_logits_ref_and_pool_ref_reproduce_the_oracle_on_the_seeded_fixture_inputs():
    """each / same / final of oracle/attention_net.py in float64 (its gathers are F.interpolate calls, its convs F.conv2d) against the
    header's formulas as mask_ref states them, fed with the state_dict entries the header names: the restatement cannot drift from
    the oracle, which tests/golden/attention_net.npz ties to the reference's own class."""
    _, sd = C.seeded_state_dict()
    x, att_text, _ = M.inputs()
    feats = M.feature_maps()
    cfg = dict(attention_layer=M.ATT_LAYER, cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS)
    _, _, final_o, _, extra = C.oracle_forward(sd, x, feats, M.SIZE, att_text, **cfg)
    d = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    text = att_text.double()
    srcs = [("first", -1)] + [(str(c), c) for c in OA.LAYER_NUM if c < len(x)]
    assert len(srcs) == M.LAYERS
    fl, per = [], []
    for tag, fi in srcs:
        w = d[f"attention_{tag}.conv.weight"]
        fl.append(feats[fi].double())
        per += [(w[0, :, :, 0, 0] / math.sqrt(w.shape[2])).t(), OO.equal_linear(text, d[f"attention_textca_{tag}.weight"], d[f"attention_textca_{tag}.bias"]),
                d[f"attention_{tag}.activate.bias"], d[f"attention_{tag}.noise.weight"]]
    wl = d["attention_last.conv.weight"][0, 0, :, 0, 0] / math.sqrt(32 * len(srcs))
    s_last = OO.equal_linear(text, d["attention_textca_last.weight"], d["attention_textca_last.bias"])
    each = R.logits_ref(fl, per, wl, s_last, d["attention_last.activate.bias"], d["attention_last.noise.weight"], d["initial_bias"],
                        [None] * (len(srcs) + 1), M.SIZE, 1e-8)
    _, ids = R.assign_ref(feats[M.CLUSTER_LAYER - 1].double(), d["initial_state"], 32)
    assert torch.equal(ids, OA.assign_clusters(feats[M.CLUSTER_LAYER - 1], sd["initial_state"]))
    final, _, _, same = R.pool_ref(each, ids.int(), M.SIZE, M.CLUSTERS)
    for name, a, b in (("each", each, extra["each"]), ("same", same, extra["same"]), ("final", final, final_o)):
        e = rel_err(a.detach(), b.detach())
        print(f"  mask_ref vs the float64 oracle, {name}: rel err {e:.3e}")
        assert e <= 1e-12, name


@pytest.mark.parametrize("c,p,s,k,b", R.ASSIGN_SHAPES)
def test_assignment_cases_have_few_near_ties(c, p, s, k, b):
    """The gap rule of the GPU test (a pixel whose float64 runner-up is within ASSIGN_GAP may go either way) excludes at most 1 % of
    a case's pixels -- a condition on the seeded inputs, so it is checked here, on the reference alone."""
    feat, cen = R.assign_case(c, p, s, k, b)
    dist, ids = R.assign_ref(feat.double(), cen.double(), p)
    _, gap = R.assign_margins(dist)
    excluded = int((gap <= R.ASSIGN_GAP).sum())
    print(f"assign case {(c, p, s, k, b)}: {excluded} of {gap.numel()} pixels within {R.ASSIGN_GAP:g} of a tie; smallest gap {float(gap.min()):.3e}; "
          f"{len(ids.unique())} of {k} clusters used")
    assert excluded <= R.ASSIGN_MAX_TIES * gap.numel()


def test_position_case_is_decided_by_the_position_channels_alone():
    feat, cen, p = R.position_case()
    dist, ids = R.assign_ref(feat.double(), cen.double(), p)
    _, gap = R.assign_margins(dist)
    assert int((gap <= R.ASSIGN_GAP).sum()) <= R.ASSIGN_MAX_TIES * gap.numel()
    cell = (torch.arange(12) // 4)  # linspace(-1, 1, 12) against the cell borders at -1/3 and 1/3
    assert torch.equal(ids, (3 * cell[:, None] + cell[None, :]).expand(2, 12, 12))
    without = torch.argmin(((feat.double().permute(0, 2, 3, 1).reshape(-1, 1, 4) - cen.double()[None, :, :4]) ** 2).sum(-1), 1)
    print(f"position case: smallest gap {float(gap.min()):.3e}; without the position channels {int((without != ids.reshape(-1)).sum())} of "
          f"{ids.numel()} ids change")
    assert (without != ids.reshape(-1)).sum() >= ids.numel() // 2


def test_tie_case_ties_exactly_and_argmin_takes_the_lowest_k():
    feat, cen = R.tie_case()
    d32, _ = R.assign_ref(feat, cen, 0)
    d64, ids = R.assign_ref(feat.double(), cen.double(), 0)
    assert torch.equal(d32.double(), d64) and torch.equal(d64, d64.round())  # exact small integers in both formats
    tied = (d64 == d64.min(1, keepdim=True).values).sum(1)
    print(f"tie case: {int((tied > 1).sum())} of {tied.numel()} pixels have more than one nearest centre (up to {int(tied.max())})")
    assert (tied > 1).sum() >= tied.numel() // 4
    lowest = (d64 == d64.min(1, keepdim=True).values).int().argmax(1)
    assert torch.equal(ids.reshape(-1), lowest)
    for a, b_ in ((0, 3), (1, 8)):  # the identical centres: the later one never wins, the earlier one does somewhere
        assert torch.equal(cen[a], cen[b_]) and not (ids == b_).any()
    assert (ids == 0).any() or (ids == 1).any()
    assert (cen.abs().sum(1) > 0).all() and d64[0].min() > 0  # pixel (0, 0, 0) is the origin: strictly nearer to a zero padding column


@pytest.mark.parametrize("size,cs,k,b", R.POOL_SHAPES)
def test_pool_cases_hold_what_the_gpu_test_needs(size, cs, k, b):
    """Over the launches of a shape: an empty cluster, ids -1 and K, cluster means on both sides of the threshold and none within 1e-3
    of it (the kernel compares in fp32; 0.8 is not a float32)."""
    seen = set()
    for assign, each in R.pool_case(size, cs, k, b):
        assert assign.shape == (b, cs, cs) and each.shape == (b, size, size) and assign.dtype == torch.int32
        choice = R.nearest_gather(assign.long(), size)
        means, counts = R.pool_means_ref(each.double(), assign, size, k)
        live = means[counts > 0]
        assert ((live - R.POOL_THRESHOLD).abs() > 1e-3).all()
        seen |= {"empty"} if (counts == 0).any() else set()
        seen |= {"-1"} if (choice == -1).any() else set()
        seen |= {"K"} if (choice == k).any() else set()
        seen |= {"above"} if (live > R.POOL_THRESHOLD).any() else set()
        seen |= {"below"} if (live < R.POOL_THRESHOLD).any() else set()
    assert seen == {"empty", "-1", "K", "above", "below"}, seen
