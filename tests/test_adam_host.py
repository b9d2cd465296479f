"""where2edit_amd.Adam on CPU tensors (the multi-tensor fallback): torch.optim.Adam's rule and state, so that the two optimizers can
stand in for one another; what it refuses; and that the kernel is never claimed where it cannot run."""
import copy

import numpy as np
import pytest
import torch

import seeded

SHAPES = [(33, 17), (64,), (5, 3, 2), (1,)]


def _params(salt=0):
    return [torch.nn.Parameter(seeded.tensor(f"adamhost.p{i}", s, salt=salt)) for i, s in enumerate(SHAPES)]


def _set_grads(params, it):
    for i, p in enumerate(params):
        p.grad = seeded.tensor(f"adamhost.g{i}", p.shape, salt=it) ** 3


def _ulps(a, b):
    """Largest distance in units in the last place between two float32 tensors (0 = the same bits)."""
    ia = a.detach().numpy().view(np.int32).astype(np.int64)
    ib = b.detach().numpy().view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max()) if ia.size else 0


@pytest.mark.parametrize("weight_decay", [0.0, 0.01], ids=["plain", "weight_decay"])
def test_five_steps_equal_torch_adam(weight_decay):
    from where2edit_amd import Adam
    pa, pb = _params(), _params()
    ours = Adam(pa, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    theirs = torch.optim.Adam(pb, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, foreach=False)
    for it in range(5):
        _set_grads(pa, it), _set_grads(pb, it)
        ours.step(), theirs.step()
        worst = max(_ulps(a, b) for a, b in zip(pa, pb))
        print(f"step {it}, weight_decay {weight_decay}: largest distance to torch.optim.Adam(foreach=False) = {worst} ulp")
        assert worst <= 1
    for a, b in zip(pa, pb):
        sa, sb = ours.state[a], theirs.state[b]
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.is_tensor(sa["step"]) and sa["step"].dtype == sb["step"].dtype and sa["step"].device == sb["step"].device
        assert float(sa["step"]) == float(sb["step"]) == 5.0
        assert _ulps(sa["exp_avg"], sb["exp_avg"]) <= 1 and _ulps(sa["exp_avg_sq"], sb["exp_avg_sq"]) <= 1


def test_state_dict_round_trips_in_both_directions():
    from where2edit_amd import Adam
    pa, pb, pc = _params(), _params(), _params()
    ours, theirs = Adam(pa, lr=0.02, weight_decay=0.01), torch.optim.Adam(pb, lr=0.02, weight_decay=0.01, foreach=False)
    for it in range(3):
        _set_grads(pa, it), _set_grads(pb, it)
        ours.step(), theirs.step()
    # ours -> torch's: a fresh torch.optim.Adam continues from our state exactly as torch's own does
    fresh = torch.optim.Adam(pc, lr=0.5, foreach=False)
    fresh.load_state_dict(copy.deepcopy(ours.state_dict()))
    with torch.no_grad():
        for c, a in zip(pc, pa):
            c.copy_(a)
    # torch's -> ours
    pd = [torch.nn.Parameter(b.detach().clone()) for b in pb]
    back = Adam(pd, lr=0.5)
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert back.param_groups[0]["lr"] == 0.02 and fresh.param_groups[0]["lr"] == 0.02
    for it in range(3, 6):
        for ps in (pa, pb, pc, pd):
            _set_grads(ps, it)
        for o in (ours, theirs, fresh, back):
            o.step()
    for a, b, c, d in zip(pa, pb, pc, pd):
        assert _ulps(c, a) <= 1 and _ulps(c, b) <= 1, "torch.optim.Adam on our state"
        assert _ulps(d, b) <= 1 and torch.equal(d, a), "our Adam on torch's state"
    assert float(back.state[pd[0]]["step"]) == 6.0


def test_a_parameter_without_gradient_is_untouched_and_stateless():
    from where2edit_amd import Adam
    ps = _params()
    before = [p.detach().clone() for p in ps]
    opt = Adam(ps, lr=0.1)
    _set_grads(ps, 0)
    ps[1].grad = None
    opt.step()
    assert torch.equal(ps[1], before[1]) and len(opt.state[ps[1]]) == 0
    assert all(not torch.equal(p, b) for i, (p, b) in enumerate(zip(ps, before)) if i != 1)
    # it joins later at its own step count
    _set_grads(ps, 1)
    opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 1.0, 2.0, 2.0]


def test_amsgrad_and_maximize_are_refused():
    from where2edit_amd import Adam
    with pytest.raises(ValueError, match="amsgrad"):
        Adam(_params(), amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        Adam(_params(), maximize=True)


def test_fused_true_on_cpu_raises_and_fused_false_never_asks_for_the_library(monkeypatch):
    from where2edit_amd import Adam, _lib
    ps = _params()
    _set_grads(ps, 0)
    with pytest.raises(RuntimeError, match="fused=True"):
        Adam(ps, fused=True).step()
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("the kernel was called for CPU tensors"))
    Adam(ps, fused=False).step()
    Adam(_params(1), fused=None).step()


def test_gradscaler_protocol_attributes():
    """GradScaler.step unscales, checks and then calls step() itself unless the optimizer claims to do so: this one does not."""
    from where2edit_amd import Adam
    assert not getattr(Adam(_params()), "_step_supports_amp_scaling", False)
