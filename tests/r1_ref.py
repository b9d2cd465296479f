"""The yardstick of the R1 gradient penalty (disc_hip.r1_penalty): the float64 restatement of the Discriminator (tests/disc64.py)
differentiated twice by stock autograd, and the float64 minibatch-stddev tangent / Hessian-vector product the kernels are held to."""
import functools

import torch

import disc64


def penalty(sd, x, dtype=torch.float64):
    """(r1, {key: d r1 / d param or None}, logits) in `dtype`: g = d sum(D(x)) / dx with create_graph, r1 = mean_b |g_b|^2
    (rosinality's d_r1_loss), then its gradient to every non-kernel key (None where the penalty does not depend on it)."""
    params = {k: v.detach().to(dtype).clone().requires_grad_(not k.endswith(".kernel")) for k, v in sd.items()}
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    y = disc64.forward(params, xx)
    (g,) = torch.autograd.grad(y.sum(), xx, create_graph=True)
    r1 = g.pow(2).reshape(g.shape[0], -1).sum(1).mean()
    keys = [k for k in params if not k.endswith(".kernel")]
    gs = torch.autograd.grad(r1, [params[k] for k in keys], allow_unused=True)
    return r1.detach(), dict(zip(keys, gs)), y.detach()


@functools.lru_cache(maxsize=None)
def case(size, cm, batch, salt=5, device="cpu"):
    """The end-to-end cases share one float64 evaluation each, computed on `device`: (state_dict, images, r1, grads, logits).
    Read-only: the tests that share a case must not write into it."""
    sd = disc64.state_dict(size, cm, salt=salt)
    x = disc64.images(batch, size, salt=salt)
    r1, grads, logits = penalty({k: v.to(device) for k, v in sd.items()}, x.to(device))
    return sd, x, r1, grads, logits


def stddev(x):
    """The stddev channel value per sample [B] of model.py:690-698 (group = min(B, 4)), in x's dtype."""
    b, c, h, w = x.shape
    g = min(b, 4)
    s = x.view(g, -1, 1, c, h, w)
    return torch.sqrt(s.var(0, unbiased=False) + 1e-8).mean([2, 3, 4]).reshape(1, -1).repeat(g, 1).reshape(b)


def stddev_jvp_hvp(x, dx, lam, dtype=torch.float64):
    """(d stddev [B], mu [B,C,h,w]) by stock autograd in `dtype`: the tangent of the stddev channel along dx, and
    mu = d/dx <lam, d stddev(x, dx)> with lam [B] the cotangent of the channel summed over its pixels."""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    ones = torch.ones(x.shape[0], dtype=dtype, requires_grad=True)
    (vjp,) = torch.autograd.grad(stddev(xx), xx, ones, create_graph=True)  # the double-vjp trick: d/d ones <vjp, dx> = J dx
    (jv,) = torch.autograd.grad((vjp * dx.to(dtype)).sum(), ones, create_graph=True)
    (mu,) = torch.autograd.grad((jv * lam.to(dtype)).sum(), xx)
    return jv.detach(), mu
