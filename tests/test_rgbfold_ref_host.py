"""tests/rgbfold_ref.py (the float64 restatement tests/test_gpu_rgbfold.py compares the HIP kernels with) against autograd through
the forward composition it is the backward of: x = lrelu(z + nw * noise + bias) * gain feeds a ToRGB (rgb = sum_o w[b,c,o] x) and
an up-sampling conv (t = s_in * conv_transpose(s_out * x)); with the loss sum(rgb * gy) + sum(t * g), gpre is d/dz, dot is
d/ds_out, the three sums are the pre-activation moment and d/dnw and d/dbias per sample, gw is d/dstyle or d/dw.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from rgbfold_ref import rgbfold_ref


@pytest.mark.parametrize("styled", [True, False])
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("shape", [(2, 5, 7, 3, 4), (1, 8, 4, 2, 2)])
def test_restatement_equals_autograd_of_the_forward(shape, with_noise, styled):
    b, k, n, h, w = shape
    gen = torch.Generator().manual_seed(13 * k + n + with_noise + 2 * styled)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    slope, gain = 0.2, 2 ** 0.5
    z = rnd(b, n, h, w).requires_grad_(True)
    noise = rnd(1, 1, h, w) if with_noise else None
    nw = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    bias = rnd(n).requires_grad_(True)
    s_out = (torch.rand(b, n, generator=gen, dtype=torch.float64) + 0.5).requires_grad_(True)
    s_in = torch.rand(b, k, generator=gen, dtype=torch.float64) + 0.5
    wt = rnd(n, k, 3, 3)
    g, gy = rnd(b, k, 2 * h + 1, 2 * w + 1), rnd(b, 3, h, w)
    if styled:
        wrgb, style = rnd(3, n), rnd(b, n).requires_grad_(True)
        wmod = wrgb[None] * style[:, None, :]
    else:
        wrgb, style = rnd(b, 3, n).requires_grad_(True), None
        wmod = wrgb
    pre = z + (nw * noise if with_noise else 0.0) + bias[None, :, None, None]
    x = F.leaky_relu(pre, slope) * gain
    assert (x > 0).any() and (x < 0).any()
    rgb = torch.einsum("bco,bohw->bchw", wmod, x)
    t = F.conv_transpose2d(x * s_out[:, :, None, None], wt, stride=2) * s_in[:, :, None, None]  # wt [N,K,3,3] as [in, out]
    loss = (rgb * gy).sum() + (t * g).sum()
    leaf = style if styled else wrgb
    gz, gnw, gbias, gso, gleaf = torch.autograd.grad(loss, [z, nw, bias, s_out, leaf], allow_unused=True)
    ref = rgbfold_ref(g, wt, s_in, s_out.detach(), x.detach(), gy, wrgb.detach(), style.detach() if styled else None, noise, slope, gain)
    close = lambda a, c: torch.testing.assert_close(a, c, rtol=1e-10, atol=1e-10)  # noqa: E731
    close(ref["gpre"][0], gz)
    close(ref["dot"][0], gso)
    close(ref["sums3"][0][..., 0], (gz * pre.detach()).sum((2, 3)))
    if with_noise:
        close(ref["sums3"][0][..., 1].sum().reshape(1), gnw)
    else:
        assert ref["sums3"][0][..., 1].abs().max() == 0
    close(ref["sums3"][0][..., 2].sum(0), gbias)
    close(ref["gw"][0], gleaf)
    for name, (val, scale) in ref.items():
        assert val.shape == scale.shape and (scale >= val.abs() * (1 - 1e-12)).all(), name
