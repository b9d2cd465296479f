"""tests/region_style_ref.py (the float64 restatement the GPU tests of csrc/region_style.hip are held to) against the stock composition
of new_styles (run_attention.py:811-822) as differentiable torch ops in float64 on the CPU: new codes, loss_delta and every parameter
gradient; and the zero-diff rule (a code whose mapper_all returns the code itself: the norm term's gradient is 0, not NaN)."""
import pytest
import torch

import region_style_ref as R

TOL = 1e-12  # two float64 evaluations of the same sums in different orders


def _close(a, b, what):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)
    assert err <= TOL, f"{what}: {err:.3e}"


@pytest.mark.parametrize("batch,dims,embed", [(3, [512, 256, 128, 64, 32], 512), (2, [64, 32], 32), (1, [32], 30)],
                         ids=["b3_mixed", "b2_tiny_clip", "b1_ragged"])
def test_formulas_equal_the_stock_composition(batch, dims, embed):
    params = R.make_params("rsref", dims, embed)
    x = R.make_inputs("rsref", batch, dims, embed)
    layers = len(dims) + 3  # (mapper_layer need not equal the number of codes passed)
    outs_s, loss_s, grads_s = R.stock_composition(params, x, 0.1, layers, embed)
    outs_f, loss_f, grads_f = R.branch(params, x, 0.1, layers, embed)
    for c, (a, b) in enumerate(zip(outs_f, outs_s)):
        _close(a, b, f"new code {c}")
    _close(loss_f, loss_s, "loss_delta")
    for f in R.FAMILIES:
        for c, ((gw, gb), (gw_s, gb_s)) in enumerate(zip(grads_f[f], grads_s[f])):
            _close(gw, gw_s, f"{f} weight gradient {c}")
            _close(gb, gb_s, f"{f} bias gradient {c}")


def test_lr_mul_enters_weight_scale_and_bias_scale():
    params = R.make_params("rsref.lr", [32], 32, lr_mul=0.01)
    x = R.make_inputs("rsref.lr", 2, [32], 32)
    outs_s, loss_s, grads_s = R.stock_composition(params, x, 0.25, 1, 32, lr_mul=0.01)
    outs_f, loss_f, grads_f = R.branch(params, x, 0.25, 1, 32, lr_mul=0.01)
    _close(outs_f[0], outs_s[0], "new code")
    _close(loss_f, loss_s, "loss_delta")
    for f in R.FAMILIES:
        _close(grads_f[f][0][0], grads_s[f][0][0], f"{f} weight gradient")
        _close(grads_f[f][0][1], grads_s[f][0][1], f"{f} bias gradient")


def zero_diff_case():
    """B = 1, two codes; code 0's mapper_all has zero weight and a bias equal to the code: y == x exactly, ||diff|| == 0."""
    dims, embed = [64, 32], 32
    params = R.make_params("rsref.zero", dims, embed)
    x = R.make_inputs("rsref.zero", 1, dims, embed)
    w, _ = params["all"][0]
    params["all"][0] = (torch.zeros_like(w), x[0][0, 0, embed:].clone())
    return params, x, dims, embed


def test_zero_diff_row_contributes_zero_not_nan():
    params, x, dims, embed = zero_diff_case()
    outs_s, loss_s, grads_s = R.stock_composition(params, x, 0.1, 2, embed)
    outs_f, loss_f, grads_f = R.branch(params, x, 0.1, 2, embed)
    assert torch.equal(outs_f[0], x[0][:, :, embed:].double()), "code 0 must come back unchanged"
    fin = R.finish_fwd([x[0][:, 0, embed:]], [outs_f[0][:, 0]], 0.1, 2)
    assert float(fin["norms"][0]) == 0.0
    _close(loss_f, loss_s, "loss_delta")
    for f in R.FAMILIES:
        for c in range(2):
            for a, b, n in zip(grads_f[f][c], grads_s[f][c], ("weight", "bias")):
                assert torch.isfinite(a).all() and torch.isfinite(b).all(), f"{f} {n} gradient {c} is not finite"
                _close(a, b, f"{f} {n} gradient {c}")
    # the norm term alone: its gradient through a zero row is exactly 0
    gy, _ = R.finish_bwd([x[0][:, 0, embed:]], [outs_f[0][:, 0]], [None], fin["norms"], 1.0, 0.1, 2)
    assert torch.equal(gy[0], torch.zeros_like(gy[0]))
