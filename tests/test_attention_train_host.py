"""The opt-in trainable mask branch, host side (no GPU): the float64 oracle against the reference's own mask-parameter gradients
(tests/golden/attention_grad.npz), the C ABI of the backward kernels, the opt-in switch and the trainer's `train_mask_from` schedule."""
import os
import re

import pytest
import torch
from torch import nn

import make_golden_attention as M
import mask_train_common as C
from helpers import golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("w2e_attention_logits_train", "w2e_attention_logits_bwd", "w2e_cluster_pool_bwd")


def test_float64_oracle_reproduces_the_references_mask_gradients():
    """2e-5: the tolerance test_oracle_golden.py holds the fp32 oracle to against the reference's fp32 results."""
    g = golden("attention_grad")
    _, sd = C.seeded_state_dict()
    x, att_text, _ = M.inputs()
    grads, unused, _ = C.oracle_mask_grads(sd, x, M.feature_maps(), M.SIZE, att_text, attention_layer=M.ATT_LAYER,
                                           cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS)
    # the modulation EqualLinears are never called (input_is_stylespace=True): no gradient in the reference, none in the oracle
    assert sorted(str(n) for n in g["unused"]) == unused
    # the oracle adds a constant zero noise: the strengths' gradient is 0 there (the reference's is sum g_pre * randn: not recorded)
    assert all(not v.any() for n, v in grads.items() if n.endswith("noise.weight"))
    entries = C.fixture_entries(g)
    assert len(entries) >= 40
    worst = 0.0
    for key, name, rows in entries:
        got = grads[name] if rows is None else grads[name][:rows]
        e = rel_err(got, g["grad." + key])
        worst = max(worst, e)
        assert e <= 2e-5, (key, e)
    print(f"float64 oracle vs reference mask gradients: worst rel err {worst:.3e} over {len(entries)} tensors")


def test_backward_entry_points_are_declared_and_prototyped():
    from where2edit_amd import _lib, run_attention
    header = open(os.path.join(ROOT, "include", "w2e_attention.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in _lib._PROTOS, name
    assert "Forward only" not in header
    assert _lib.header_version() == 7  # symbols were added; the ABI version did not move
    # the Python mirror of W2E_ATT_BWD_WORKSPACE
    m = re.search(r"#define W2E_ATT_BWD_WORKSPACE\(n, B, P, sum_channels\)(.*?)\n\n", header, flags=re.S)
    expr = m.group(1).replace("\\\n", " ").replace("(int64_t)", "").replace("/", "//")
    for n, B, P, sum_channels in ((18, 1, 4096, 6080), (3, 2, 256, 800), (1, 5, 100, 32)):
        assert eval(expr) == run_attention.att_bwd_workspace(n, B, P, sum_channels)


def test_built_library_refuses_bad_backward_arguments_without_a_gpu():
    import ctypes
    from where2edit_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    lib.w2e_last_error.restype = ctypes.c_char_p
    lib.w2e_cluster_pool_bwd.argtypes = [ctypes.c_void_p] * 9 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    p = ctypes.c_void_p(64)
    assert lib.w2e_cluster_pool_bwd(p, None, p, p, p, p, p, p, p, 1, 16, 16, 6, None) != 0 and b"null" in lib.w2e_last_error()
    assert lib.w2e_cluster_pool_bwd(p, p, p, p, p, p, p, p, p, 1, 200, 16, 6, None) != 0 and b"size <= 128" in lib.w2e_last_error()
    assert lib.w2e_cluster_pool_bwd(p, p, p, p, p, p, p, p, p, 1, 16, 16, 33, None) != 0 and b"clusters <= 32" in lib.w2e_last_error()


def _mask_flags(net):
    return {n: p.requires_grad for n, p in net.named_parameters() if C.is_mask_param(n)}


def test_train_mask_branch_is_an_opt_in_with_an_undo():
    import where2edit_amd
    from where2edit_amd.run_attention import freeze_mask_branch, train_mask_branch
    net, _ = C.seeded_state_dict()
    assert not getattr(net, "_train_mask", False)  # off by default
    assert where2edit_amd.train_mask_branch.__doc__
    assert where2edit_amd.train_mask_branch(net) is net and net._train_mask
    flags = _mask_flags(net)
    assert flags and all(flags.values())
    assert freeze_mask_branch(net) is net and not net._train_mask and not any(_mask_flags(net).values())
    assert all(p.requires_grad for n, p in net.named_parameters() if not C.is_mask_param(n))
    train_mask_branch(net, enabled=False)
    assert not net._train_mask


def _cpu_trainer(**kw):
    from where2edit_amd.run_attention import RegionAttentionTrainer
    net, _ = C.seeded_state_dict()
    return RegionAttentionTrainer(nn.Identity(), nn.Identity(), net, attention_layer=M.ATT_LAYER, steps=100, device="cpu", **kw)


@pytest.mark.parametrize("bad", [-0.1, float("nan"), "1.15", True, [0.5]])
def test_train_mask_from_is_validated(bad):
    with pytest.raises(ValueError, match="train_mask_from"):
        _cpu_trainer(train_mask_from=bad)


def test_train_mask_from_none_keeps_the_frozen_branch():
    tr = _cpu_trainer()
    assert tr.train_mask_from is None and not any(_mask_flags(tr.mapper).values())
    assert not getattr(tr.mapper, "_train_mask", False)
    assert tr.params and all(p.requires_grad for p in tr.params)
    ids = {id(p) for p in tr.params}
    assert not any(id(p) in ids for n, p in tr.mapper.named_parameters() if C.is_mask_param(n))
    tr.global_step = 99
    assert tr._schedule_mask() is False and not any(_mask_flags(tr.mapper).values())


def test_train_mask_from_reproduces_the_references_schedule():
    """run_attention.py:1076-1083 with T in the place of 1.15: frozen while t < T, trainable from then on."""
    tr = _cpu_trainer(train_mask_from=0.5)
    ids = {id(p) for g in tr.optimizer.param_groups for p in g["params"]}
    assert all(id(p) in ids for p in tr.mapper.parameters())  # the optimizer covers the mask parameters (:1051)
    for step, on in ((0, False), (49, False), (50, True), (51, True), (99, True)):
        tr.global_step = step
        assert tr._schedule_mask() is on
        flags = _mask_flags(tr.mapper)
        assert all(v is on for v in flags.values()), step
        assert bool(getattr(tr.mapper, "_train_mask", False)) is on
        assert all(p.requires_grad for n, p in tr.mapper.named_parameters() if not C.is_mask_param(n))
    assert all(v for v in _mask_flags(_cpu_trainer(train_mask_from=0).mapper).values())       # trainable from the first step
    assert not any(_mask_flags(_cpu_trainer(train_mask_from=1.15).mapper).values())           # the reference's literal: never
