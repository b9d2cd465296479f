"""tests/upblur_ref.py (the float64 restatement tests/test_gpu_upblur.py compares the HIP kernels with) against the oracle's
up-sampling StyledConv (oracle/stylegan2.py), both in float64 on the CPU."""
import math

import pytest
import torch

from oracle import ops
from oracle import stylegan2 as OG
from upblur_ref import upblur_ref


@pytest.mark.parametrize("shape", [(2, 5, 6, 4, 7), (1, 3, 2, 9, 5)])
def test_restatement_equals_the_oracles_styled_up_conv(shape):
    b, k, n, h, w = shape
    g = torch.Generator().manual_seed(11 * k + n)
    weight = torch.randn(1, n, k, 3, 3, generator=g, dtype=torch.float64)
    s = torch.rand(b, k, generator=g, dtype=torch.float64) + 0.5
    x = torch.randn(b, k, h, w, generator=g, dtype=torch.float64)
    noise = torch.randn(1, 1, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    nw = torch.tensor([0.3], dtype=torch.float64)
    bias = torch.randn(n, generator=g, dtype=torch.float64)
    kernel = ops.make_kernel([1, 3, 3, 1]).double() * 4  # Blur(..., upsample_factor=2)
    sd = {"c.conv.weight": weight, "c.conv.modulation.weight": None, "c.conv.modulation.bias": None, "c.conv.blur.kernel": kernel,
          "c.noise.weight": nw, "c.activate.bias": bias}
    want, _ = OG.styled_conv(sd, "c", x, s.view(b, 1, k, 1, 1), noise, upsample=True, input_is_stylespace=True)
    # the kernels' factoring: shared weight scale * W, the modulation on the input, the demodulation on the output
    scale = 1.0 / math.sqrt(k * 9)
    wt = scale * weight[0]
    d = torch.rsqrt(((wt[None] * s[:, None, :, None, None]) ** 2).sum((2, 3, 4)) + 1e-8)
    got, term_scale = upblur_ref(x, wt, s, d, kernel, noise, nw, bias)
    assert got.shape == want.shape == (b, n, 2 * h, 2 * w)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    assert (term_scale >= got.abs() * (1 - 1e-12)).all()  # the term scale bounds the result it belongs to
    # without noise and bias: the bare blurred transposed convolution, activated
    sd0 = dict(sd, **{"c.noise.weight": torch.zeros(1, dtype=torch.float64), "c.activate.bias": torch.zeros(n, dtype=torch.float64)})
    want0, _ = OG.styled_conv(sd0, "c", x, s.view(b, 1, k, 1, 1), noise, upsample=True, input_is_stylespace=True)
    got0, _ = upblur_ref(x, wt, s, d, kernel)
    assert (got0 - want0).abs().max() <= 1e-12 * want0.abs().max()
