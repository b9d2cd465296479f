"""where2edit_amd.derived on the CPU: when an entry is rebuilt, that `invalidate_caches` reaches the caches a `.data` write leaves
stale (the sites that need no library), that nothing cached enters a state_dict or is served to a deep copy, and the host rules the
two fused optimizers share (where2edit_amd._fused_opt)."""
import copy

import pytest
import torch

import make_golden_attention as M
import seeded
from where2edit_amd.derived import Holder, derived, drop, invalidate
from where2edit_amd.stylegan2 import EqualLinear, Generator, invalidate_caches


class _Counted:
    """A build function that counts its runs and returns a fresh object each time."""

    def __init__(self):
        self.runs = 0

    def __call__(self):
        self.runs += 1
        return object()


def test_build_runs_once_then_again_for_every_change_the_key_sees():
    owner, build = torch.nn.Module(), _Counted()
    w = torch.zeros(4)
    first = derived(owner, "s", [w], build)
    assert derived(owner, "s", [w], build) is first and derived(owner, "s", (w,), build) is first and build.runs == 1
    w.add_(1)
    second = derived(owner, "s", [w], build)
    assert build.runs == 2 and second is not first and derived(owner, "s", [w], build) is second
    w.data = torch.ones(4)
    derived(owner, "s", [w], build)
    assert build.runs == 3
    torch.autograd.graph.increment_version([w])
    derived(owner, "s", [w], build)
    assert build.runs == 4
    w.data.mul_(2)  # the documented gap: a write through .data changes nothing the key holds
    derived(owner, "s", [w], build)
    assert build.runs == 4
    invalidate(owner)
    derived(owner, "s", [w], build)
    assert build.runs == 5
    same_values = w.clone()  # another object with the same contents and version
    derived(owner, "s", [same_values], build)
    assert build.runs == 6


def test_none_entries_and_independent_slots():
    owner, a, b = torch.nn.Module(), _Counted(), _Counted()
    w, bias = torch.zeros(3), torch.zeros(3)
    va = derived(owner, "a", [w, None], a)
    vb = derived(owner, ("b", 0), [w, None], b)
    assert va is not vb and derived(owner, "a", [w, None], a) is va and derived(owner, ("b", 0), [w, None], b) is vb
    assert (a.runs, b.runs) == (1, 1)
    derived(owner, "a", [w, bias], a)  # the bias appeared: slot "a" rebuilds, ("b", 0) does not
    derived(owner, ("b", 0), [w, None], b)
    assert (a.runs, b.runs) == (2, 1)
    derived(owner, "a", [None, w], a)  # None in another place is another key
    assert a.runs == 3
    derived(owner, "a", [None, w, bias], a)  # as is a longer or a shorter list
    derived(owner, "a", [None], a)
    assert a.runs == 5


def test_an_entry_holds_its_tensors_so_a_recycled_address_or_id_is_never_served():
    owner = Holder()
    for _ in range(64):  # the allocator hands freed blocks back: some of these tensors share an address or an id() with an earlier one
        w = torch.zeros(256)
        built = []
        value = derived(owner, "s", [w], lambda: built.append(w) or built)
        assert value is built and value[0] is w, "an entry built from another tensor was served"
        del w, built, value
    drop(owner)
    fresh = []
    assert derived(owner, "s", [torch.zeros(256)], lambda: fresh) is fresh


def test_a_holder_is_dropped_by_invalidate_and_module_state_is_not_touched():
    holder, build = Holder(), _Counted()
    v = torch.zeros(2)
    derived(holder, "rep", [v], build)
    lin = torch.nn.Linear(2, 2)
    derived(lin, "x", [lin.weight], build)
    keys = set(lin.state_dict())
    invalidate(torch.nn.Sequential(lin))
    assert set(lin.state_dict()) == keys == {"weight", "bias"}
    derived(holder, "rep", [v], build)
    assert build.runs == 3


# ------------------------------------------------------------------------------------------- invalidate_caches: the sites without a library
def _halve(p):
    p.data.mul_(0.5)  # the kind of write no key sees


def test_invalidate_caches_is_the_helpers_invalidate():
    assert invalidate_caches is invalidate


def test_equal_linear_scaled_after_a_data_write():
    lin = EqualLinear(8, 8, lr_mul=0.01, activation="fused_lrelu")
    with torch.no_grad():
        w0, b0 = lin._scaled()
        lin.bias.data.add_(1.0)
        _halve(lin.weight)
        assert lin._scaled()[0] is w0, "the gap this test is about has closed: a .data write rebuilt the entry"
        invalidate_caches(lin)
        w1, b1 = lin._scaled()
    assert torch.equal(w1, lin.weight.detach() * lin.scale) and torch.equal(b1, lin.bias.detach() * lin.lr_mul)
    assert not torch.equal(w1, w0) and not torch.equal(b1, b0)
    assert set(lin.state_dict()) == {"weight", "bias"}
    assert lin._scaled()[0].requires_grad, "trained parameters must bypass the cache"


def test_generator_style_pack_after_a_data_write():
    g = Generator(16, 512, 8)
    keys = set(g.state_dict())
    plan = g._layers()
    mods = [m.conv.modulation for m, _, _, _ in plan]
    w0, b0, meta0, widths0 = g._style_pack(plan)
    assert g._style_pack(plan)[0] is w0
    _halve(mods[1].weight)
    _halve(mods[-1].bias)
    assert g._style_pack(plan)[0] is w0
    invalidate_caches(g)
    w1, b1, meta1, widths1 = g._style_pack(plan)
    assert torch.equal(w1, torch.cat([m.weight.detach() * m.scale for m in mods]))
    assert torch.equal(b1, torch.cat([m.bias.detach() * m.lr_mul for m in mods]))
    assert not torch.equal(w1, w0) and not torch.equal(b1, b0) and torch.equal(meta1, meta0) and widths1 == widths0
    assert set(g.state_dict()) == keys


def test_a_deep_copy_is_never_served_the_originals_tensors():
    lin = EqualLinear(8, 8)
    with torch.no_grad():
        w0, _ = lin._scaled()
        twin = copy.deepcopy(lin)
        _halve(twin.weight)  # (a .data write: only a key that tells the copy's parameter from the original's can notice)
        wt, _ = twin._scaled()
        assert lin._scaled()[0] is w0
    assert torch.equal(wt, twin.weight.detach() * twin.scale) and not torch.equal(wt, w0)


@pytest.fixture(scope="module")
def region_net():
    from where2edit_amd.run_attention import FullSpaceMapperFEATClusterLinStyle_Net
    torch.manual_seed(0)
    return FullSpaceMapperFEATClusterLinStyle_Net(M.LAYERS, 1024, 512, attention_layer=M.ATT_LAYER, channel_multiplier=2,
                                                  cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS, cluster_dim=576).requires_grad_(False)


def test_region_net_caches_after_a_data_write(region_net, monkeypatch):
    from where2edit_amd import functional as K
    net = region_net
    keys = set(net.state_dict())
    packs = []
    monkeypatch.setattr(K, "style_affine_all", lambda x, pack: packs.append(pack))  # the launch itself needs the GPU: keep its operand
    src = net._sources(M.ATT_LAYER)
    conv, mods = src[0][0].conv, [aff for _, aff, _ in src] + [net.attention_textca_last]
    noise = src[0][0].noise.weight
    text = seeded.tensor("derived.text", (2, 512))
    with torch.no_grad():
        wsc0 = net._wscaled_t(conv)
        assert net._noise_is_off(noise) is True
        net._text_styles(mods, text)
        noise.data.fill_(0.25)
        _halve(conv.weight)
        _halve(mods[0].weight)
        _halve(mods[-1].bias)
        net._text_styles(mods, text)
        assert net._wscaled_t(conv) is wsc0 and net._noise_is_off(noise) is True and packs[1] is packs[0]
        invalidate_caches(net)
        net._text_styles(mods, text)
        assert torch.equal(net._wscaled_t(conv), (conv.weight[0, :, :, 0, 0] * conv.scale).t()) and not torch.equal(net._wscaled_t(conv), wsc0)
        assert net._noise_is_off(noise) is False
    w, b, _, widths = packs[2]
    assert torch.equal(w, torch.cat([m.weight * m.scale for m in mods])) and torch.equal(b, torch.cat([m.bias * m.lr_mul for m in mods]))
    assert not torch.equal(w, packs[0][0]) and not torch.equal(b, packs[0][1]) and widths == [m.weight.shape[0] for m in mods]
    assert set(net.state_dict()) == keys


# ------------------------------------------------------------------------------------------- the optimizers' shared base
def _params():
    return [torch.nn.Parameter(seeded.tensor(f"derived.p{i}", s)) for i, s in enumerate([(9, 5), (7,)])]


def test_ranger_fused_true_on_cpu_raises_and_fused_false_never_loads_the_library(monkeypatch):
    from where2edit_amd import _lib
    from where2edit_amd.ranger import Ranger
    ps = _params()
    for i, p in enumerate(ps):
        p.grad = seeded.tensor(f"derived.g{i}", p.shape)
    with pytest.raises(RuntimeError, match=r"Ranger\(fused=True\)"):
        Ranger(ps, fused=True).step()
    monkeypatch.setattr(_lib, "load", lambda *a: pytest.fail("fused=False asked for the library"))
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("the kernel was called for CPU tensors"))
    before = [p.detach().clone() for p in ps]
    Ranger(ps, fused=False).step()
    assert all(not torch.equal(p, b) for p, b in zip(ps, before))


def test_both_optimizers_share_one_eligibility_rule_and_name_themselves():
    from where2edit_amd import Adam
    from where2edit_amd.ranger import Ranger
    from where2edit_amd._fused_opt import FusedStep
    assert Adam._fused_applies is FusedStep._fused_applies and Ranger._fused_applies is FusedStep._fused_applies
    assert Adam._fused_call is FusedStep._fused_call and Ranger._fused_call is FusedStep._fused_call
    ps = _params()
    for i, p in enumerate(ps):
        p.grad = seeded.tensor(f"derived.g{i}", p.shape)
    with pytest.raises(RuntimeError, match=r"Adam\(fused=True\)"):
        Adam(ps, fused=True).step()
