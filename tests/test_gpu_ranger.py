"""Ranger's one-launch update (csrc/ranger.hip, w2e_ranger_step) through where2edit_amd.ranger.Ranger on the GPU: the 13-step fixture
of mapper/training/ranger.py that tests/test_dist_cpu.py holds the multi-tensor path to, a float64 restatement of the rule for the
state and for shapes the fixture does not have, and the host behaviour around the launch (which path ran, p.grad untouched, skipped
parameters, parameters at different step counts, the state-dict round trip).  Everything is held to the 1e-5 of the CPU test."""
import copy
import math

import pytest
import torch

import seeded
from helpers import assert_close, golden, rel_err
from make_golden import RANGER_SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-5
LR = 0.5


class Ref64:
    """ranger.py's rule (mapper/training/ranger.py:78-164) restated in float64 on the CPU; a gradient of None skips its parameter."""

    def __init__(self, params, lr=LR, alpha=0.5, k=6, threshold=5, betas=(0.95, 0.999), eps=1e-5):
        self.p = [p.detach().double().cpu().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.slow = [p.clone() for p in self.p]
        self.t = [0] * len(self.p)
        self.lr, self.alpha, self.k, self.thr, self.betas, self.eps = lr, alpha, k, threshold, betas, eps

    def step(self, grads):
        b1, b2 = self.betas
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.detach().double().cpu()
            if g.dim() > 1:
                g = g - g.mean(dim=tuple(range(1, g.dim())), keepdim=True)
            self.t[i] += 1
            t = self.t[i]
            self.v[i] = self.v[i] * b2 + (1 - b2) * g * g
            self.m[i] = self.m[i] * b1 + (1 - b1) * g
            b2t = b2 ** t
            n_max = 2 / (1 - b2) - 1
            n_sma = n_max - 2 * t * b2t / (1 - b2t)
            if n_sma > self.thr:
                size = math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - b1 ** t)
                self.p[i] = self.p[i] - size * self.lr * self.m[i] / (self.v[i].sqrt() + self.eps)
            else:
                self.p[i] = self.p[i] - self.lr / (1 - b1 ** t) * self.m[i]
            if t % self.k == 0:
                self.slow[i] = self.slow[i] + self.alpha * (self.p[i] - self.slow[i])
                self.p[i] = self.slow[i].clone()


@pytest.fixture
def fused_calls(monkeypatch):
    """Counts the w2e_ranger_step calls that go through _lib.call."""
    from where2edit_amd import _lib
    seen = []
    real = _lib.call

    def counting(name, *args):
        if name == "w2e_ranger_step":
            seen.append(args[0])  # tensors in the call
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    return seen


def _fixture_params():
    return [torch.nn.Parameter(seeded.tensor("ranger.p." + n, s).to(DEV)) for n, s in RANGER_SHAPES]


def _fixture_grads(it):
    return [seeded.tensor(f"ranger.g.{n}", s, salt=it) for n, s in RANGER_SHAPES]


def _hold_state(opt, params, ref, what):
    for i, p in enumerate(params):
        st = opt.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq", "slow_buffer"}
        assert type(st["step"]) is int and st["step"] == ref.t[i]
        assert_close(st["exp_avg"], ref.m[i], TOL, f"{what} exp_avg {i}")
        assert_close(st["exp_avg_sq"], ref.v[i], TOL, f"{what} exp_avg_sq {i}")
        assert_close(st["slow_buffer"], ref.slow[i], TOL, f"{what} slow_buffer {i}")


def test_fixture_run_takes_the_fused_path_and_matches_the_reference(fused_calls):
    """13 steps at lr 0.5: crosses the rectification threshold near step 6 and two look-ahead syncs."""
    from where2edit_amd.ranger import Ranger
    g = golden("ranger")
    params = _fixture_params()
    opt = Ranger(params, lr=LR)
    ref = Ref64(params)
    for it in range(13):
        grads = _fixture_grads(it)
        for p, gr in zip(params, grads):
            p.grad = gr.to(DEV)
        before = [p.grad.clone() for p in params]
        versions = [p._version for p in params]
        opt.step()
        ref.step(grads)
        assert len(fused_calls) == it + 1 and fused_calls[-1] == len(params), "the fused path was not taken"
        assert all(p._version > v for p, v in zip(params, versions)), "an in-place update must bump the parameter's version (caches key on it)"
        for (n, _), p, b in zip(RANGER_SHAPES, params, before):
            assert torch.equal(p.grad, b), f"step {it}: p.grad of {n} was modified"
            assert_close(p, g[f"step{it}.{n}"], TOL, f"step {it} {n}")
        _hold_state(opt, params, ref, f"step {it}")


def test_multi_tensor_path_on_the_gpu_stays_and_its_distance_is_reported(fused_calls):
    """fused=False keeps the _foreach code; the largest distance between the two paths is printed per step (not asserted)."""
    from where2edit_amd.ranger import Ranger
    g = golden("ranger")
    pa, pb = _fixture_params(), _fixture_params()
    fused, plain = Ranger(pa, lr=LR), Ranger(pb, lr=LR, fused=False)
    for it in range(13):
        for a, b, gr in zip(pa, pb, _fixture_grads(it)):
            a.grad, b.grad = gr.to(DEV), gr.to(DEV)
        fused.step()
        n_fused = len(fused_calls)
        plain.step()
        assert len(fused_calls) == n_fused == it + 1, "fused=False went through the kernel"
        for (n, _), b in zip(RANGER_SHAPES, pb):
            assert_close(b, g[f"step{it}.{n}"], TOL, f"multi-tensor step {it} {n}")
        print(f"step {it}: fused vs multi-tensor, largest rel distance {max(rel_err(a, b) for a, b in zip(pa, pb)):.3e}")


def test_a_parameter_without_gradient_is_skipped_and_step_counts_keep_their_own_scalars(fused_calls):
    from where2edit_amd.ranger import Ranger
    params = [torch.nn.Parameter(seeded.tensor(f"rg.skip.p{i}", s).to(DEV)) for i, s in enumerate([(6, 10), (9,)])]
    opt = Ranger(params, lr=LR)
    ref = Ref64(params)
    for it in range(9):  # parameter 1 joins at step 5: the two are then at different step counts, on either side of the threshold
        grads = [seeded.tensor(f"rg.skip.g{i}", p.shape, salt=it) if (i == 0 or it >= 5) else None for i, p in enumerate(params)]
        for p, gr in zip(params, grads):
            p.grad = None if gr is None else gr.to(DEV)
        untouched = params[1].detach().clone()
        calls = len(fused_calls)
        opt.step()
        ref.step(grads)
        if it < 5:
            assert torch.equal(params[1], untouched) and len(opt.state[params[1]]) == 0, "a parameter without gradient was touched"
            assert fused_calls[calls:] == [1]
        else:
            assert fused_calls[calls:] == [1, 1], "parameters at different step counts must be updated by their own calls"
        for i, p in enumerate(params):
            assert_close(p, ref.p[i], TOL, f"step {it} parameter {i}")
    assert [opt.state[p]["step"] for p in params] == [9, 4]
    _hold_state(opt, params, ref, "after 9 steps")


def test_state_dict_round_trip_continues_bit_for_bit(fused_calls):
    from where2edit_amd.ranger import Ranger

    def run(reload_at):
        params = _fixture_params()
        opt = Ranger(params, lr=LR)
        for it in range(8):
            if it == reload_at:
                opt.load_state_dict(copy.deepcopy(opt.state_dict()))
            for p, gr in zip(params, _fixture_grads(it)):
                p.grad = gr.to(DEV)
            opt.step()
        return params, opt

    (pa, oa), (pb, ob) = run(None), run(7)
    assert len(fused_calls) == 16
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
            assert torch.equal(oa.state[a][key], ob.state[b][key]), key
        assert oa.state[a]["step"] == ob.state[b]["step"] == 8


# a row shorter than a wave; four dimensions with a row of 27; a row longer than a wave keeps in registers (two passes); 1-D (no centralisation)
EXTRA_SHAPES = [(3, 5), (4, 3, 3, 3), (2, 5000), (7,)]


@pytest.mark.parametrize("shape", EXTRA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_extra_shapes_match_float64(fused_calls, shape):
    from where2edit_amd.ranger import Ranger
    key = "rg.extra." + "x".join(map(str, shape))
    params = [torch.nn.Parameter(seeded.tensor(key + ".p", shape).to(DEV))]
    opt = Ranger(params, lr=LR)
    ref = Ref64(params)
    for it in range(7):
        gr = seeded.tensor(key + ".g", shape, salt=it)
        params[0].grad = gr.to(DEV)
        opt.step()
        ref.step([gr])
        assert_close(params[0], ref.p[0], TOL, f"{shape} step {it}")
    assert len(fused_calls) == 7
    _hold_state(opt, params, ref, f"{shape}")


def test_a_fused_step_does_not_leave_the_frozen_path_its_primed_products(fused_calls):
    """EqualLinear under no_grad serves cached weight*scale / bias*lr_mul products (the mapper's stock path reads them): a validation
    pass primes them, a fused step writes the parameters through raw pointers, and the next validation pass must see the new ones."""
    from where2edit_amd.op import fused_leaky_relu
    from where2edit_amd.ranger import Ranger
    from where2edit_amd.stylegan2 import EqualLinear
    lin = EqualLinear(8, 8, lr_mul=0.01, activation="fused_lrelu")
    with torch.no_grad():
        lin.weight.copy_(seeded.tensor("ranger.stale.w", (8, 8)) / 0.01)
        lin.bias.copy_(seeded.tensor("ranger.stale.b", (8,)))
    lin = lin.to(DEV)
    x = seeded.tensor("ranger.stale.x", (2, 8)).to(DEV)
    with torch.no_grad():
        primed = lin(x).clone()
    lin.weight.grad = seeded.tensor("ranger.stale.gw", (8, 8)).to(DEV)
    lin.bias.grad = seeded.tensor("ranger.stale.gb", (8,)).to(DEV)
    Ranger(lin.parameters(), lr=LR).step()
    assert fused_calls == [2], "the kernel was not taken"
    with torch.no_grad():
        after = lin(x)
        live = fused_leaky_relu(torch.nn.functional.linear(x, lin.weight * lin.scale), lin.bias * lin.lr_mul)
    assert torch.equal(after, live), "the no_grad forward did not use the live parameters"
    assert not torch.equal(after, primed), "the step did not change the output: the test shows nothing"
