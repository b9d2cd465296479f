"""Adam's one-launch update (csrc/adam.hip, w2e_adam_step) through where2edit_amd.Adam on the GPU, against a float64 replay of
torch.optim.Adam's rule.  The tolerance is not fixed in advance: the yardstick is the distance of torch.optim.Adam(foreach=False) in
fp32 on the CPU from the same replay on the same inputs, and the kernel may be 4x that (an equally valid fp32 evaluation may round
in another order; 4x stays two orders below a dropped bias correction).  Both distances are printed.  Around the launch: which path
ran, p.grad untouched, skipped parameters, 64 tensors per launch, parameters at different step counts, the state-dict round trip."""
import copy

import pytest
import torch

import seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(512, 1024), (512,), (288, 64), (1,), (0,)]
STEPS = 8
LR, BETAS, EPS = 0.01, (0.9, 0.999), 1e-8


class Ref64:
    """torch/optim/adam.py's rule (no amsgrad, no maximize) in float64 on the CPU; a gradient of None skips its parameter."""

    def __init__(self, params, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0):
        self.p = [p.detach().double().cpu().clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay

    def step(self, grads):
        b1, b2 = self.betas
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = g.detach().double().cpu() + self.wd * self.p[i]
            self.t[i] += 1
            t = self.t[i]
            self.m[i] = b1 * self.m[i] + (1 - b1) * g
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            self.p[i] = self.p[i] - self.lr / (1 - b1 ** t) * self.m[i] / (self.v[i].sqrt() / (1 - b2 ** t) ** 0.5 + self.eps)


def _dist(a, b):
    """max |a - b| / max |b| (0 for an empty tensor)."""
    a, b = a.detach().double().cpu(), b.double()
    return 0.0 if b.numel() == 0 else ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _params(dev, shapes=SHAPES):
    return [torch.nn.Parameter(seeded.tensor(f"adam.p{i}", s).to(dev)) for i, s in enumerate(shapes)]


def _grads(it, shapes=SHAPES):
    return [seeded.tensor(f"adam.g{i}", s, salt=it) ** 3 for i, s in enumerate(shapes)]


@pytest.fixture
def fused_calls(monkeypatch):
    """The tensor counts of the w2e_adam_step calls that go through _lib.call."""
    from where2edit_amd import _lib
    seen, real = [], _lib.call

    def counting(name, *args):
        if name == "w2e_adam_step":
            seen.append(args[0])
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    return seen


@pytest.mark.parametrize("weight_decay", [0.0, 0.01], ids=["plain", "weight_decay"])
def test_eight_steps_within_four_times_torchs_own_distance_to_float64(fused_calls, weight_decay):
    from where2edit_amd import Adam
    gpu, cpu = _params(DEV), _params("cpu")
    ours = Adam(gpu, lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay)
    theirs = torch.optim.Adam(cpu, lr=LR, betas=BETAS, eps=EPS, weight_decay=weight_decay, foreach=False)
    ref = Ref64(cpu, weight_decay=weight_decay)
    for it in range(STEPS):
        grads = _grads(it)
        for p, q, g in zip(gpu, cpu, grads):
            p.grad, q.grad = g.to(DEV), g.clone()
        before = [p.grad.clone() for p in gpu]
        versions = [p._version for p in gpu]
        ours.step(), theirs.step(), ref.step(grads)
        assert all(p._version > v for p, v in zip(gpu, versions)), "an in-place update must bump the parameter's version (caches key on it)"
        assert len(fused_calls) == it + 1 and fused_calls[-1] == len(SHAPES), "the kernel was not taken"
        assert all(torch.equal(p.grad, b) for p, b in zip(gpu, before)), f"step {it}: p.grad was modified"
    # one distance per quantity: the largest per-tensor relative distance.  (Tensor by tensor the yardstick would be a lottery for the
    # 1-element tensor, whose fp32 value sits anywhere within half an ulp of the float64 one; the large tensors set the scale.)
    for what, mine, torchs, refs in (("p", gpu, cpu, ref.p), ("exp_avg", [ours.state[p]["exp_avg"] for p in gpu], [theirs.state[q]["exp_avg"] for q in cpu], ref.m),
                                     ("exp_avg_sq", [ours.state[p]["exp_avg_sq"] for p in gpu], [theirs.state[q]["exp_avg_sq"] for q in cpu], ref.v)):
        d_kernel, d_torch = [_dist(a, r) for a, r in zip(mine, refs)], [_dist(b, r) for b, r in zip(torchs, refs)]
        for s, dk, dt in zip(SHAPES, d_kernel, d_torch):
            print(f"{s} {what} after {STEPS} steps (weight_decay {weight_decay}): kernel {dk:.3e}, torch.optim.Adam fp32 on the CPU {dt:.3e} from float64")
        print(f"{what}: kernel {max(d_kernel):.3e}, yardstick {max(d_torch):.3e}, ratio {max(d_kernel) / max(d_torch):.2f}")
        assert max(d_kernel) <= 4 * max(d_torch), f"{what}: kernel {max(d_kernel):.3e} > 4 x {max(d_torch):.3e}"
    for i in range(len(SHAPES)):
        st = ours.state[gpu[i]]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == STEPS and st["step"].device.type == "cpu"


def test_a_parameter_without_gradient_is_untouched_and_step_counts_get_their_own_calls(fused_calls):
    from where2edit_amd import Adam
    shapes = [(40, 8), (9,), (33,)]
    ps = _params(DEV, shapes)
    ref = Ref64(ps)
    opt = Adam(ps, lr=LR)
    for it in range(3):
        grads = _grads(it, shapes)
        if it == 0:
            grads[1] = None  # joins at the second step: from then on two step counts
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.to(DEV)
        held = ps[1].detach().clone()
        calls = len(fused_calls)
        opt.step()
        ref.step(grads)
        if it == 0:
            assert torch.equal(ps[1], held) and len(opt.state[ps[1]]) == 0, "a parameter without gradient must be left alone"
            assert fused_calls[calls:] == [2]
        else:
            assert sorted(fused_calls[calls:]) == [1, 2], "parameters at different step counts must be updated by their own calls"
    for i in range(3):
        assert _dist(ps[i], ref.p[i]) <= 1e-5, f"parameter {i}"
    assert [float(opt.state[p]["step"]) for p in ps] == [3.0, 2.0, 3.0]


def test_seventy_tensors_take_two_launches_and_every_one_is_updated(fused_calls):
    from where2edit_amd import Adam
    shapes = [(1 + (7 * i) % 50, 3) for i in range(70)]
    ps = _params(DEV, shapes)
    ref = Ref64(ps)
    opt = Adam(ps, lr=LR)
    grads = _grads(0, shapes)
    for p, g in zip(ps, grads):
        p.grad = g.to(DEV)
    opt.step()
    ref.step(grads)
    assert fused_calls == [64, 6]  # 64 tensors per launch, a further launch beyond that
    for i in range(70):
        assert _dist(ps[i], ref.p[i]) <= 1e-5, f"tensor {i} of 70"


def test_fused_false_never_enters_the_kernel_and_fused_true_raises_where_it_cannot(fused_calls):
    from where2edit_amd import Adam
    ps, qs = _params(DEV), _params(DEV)
    plain, fused = Adam(ps, lr=LR, fused=False), Adam(qs, lr=LR, fused=True)
    for it in range(2):
        for p, q, g in zip(ps, qs, _grads(it)):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        plain.step()
        assert len(fused_calls) == it, "fused=False went through the kernel"
        fused.step()
        assert len(fused_calls) == it + 1
    for p, q in zip(ps, qs):
        assert _dist(p, q.detach().double().cpu()) <= 1e-5
    qs[2].grad = qs[2].grad.t().contiguous().t()  # a strided gradient
    with pytest.raises(RuntimeError, match="fused=True"):
        fused.step()


def test_state_round_trips_with_torch_adam(fused_calls):
    from where2edit_amd import Adam
    ps, qs = _params(DEV), _params(DEV)
    ours, theirs = Adam(ps, lr=LR), torch.optim.Adam(qs, lr=LR, foreach=False)
    ref = Ref64(ps)
    for it in range(6):
        grads = _grads(it)
        for p, q, g in zip(ps, qs, grads):
            p.grad, q.grad = g.to(DEV), g.to(DEV)
        ours.step(), theirs.step(), ref.step(grads)
        if it == 2:  # swap the states: each optimizer continues from the other's
            a, b = copy.deepcopy(ours.state_dict()), copy.deepcopy(theirs.state_dict())
            ours.load_state_dict(b), theirs.load_state_dict(a)
            assert ours.state[ps[0]]["step"].device.type == "cpu" and float(ours.state[ps[0]]["step"]) == 3.0
    assert len(fused_calls) == 6
    for i in range(len(SHAPES)):
        assert _dist(ps[i], ref.p[i]) <= 1e-5 and _dist(qs[i], ref.p[i]) <= 1e-5, f"parameter {i} after the swap"
