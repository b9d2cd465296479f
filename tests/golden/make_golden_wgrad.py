"""Golden vectors of the conv-weight gradient (decoder fine-tuning).  Like make_golden.py, runs ONLY where the reference checkout
exists and imports the reference's own models/stylegan2/model.py; the outputs are committed as tests/golden/modconv_wgrad.npz.

    python tests/golden/make_golden_wgrad.py

For the four MODCONV_CASES of make_golden.py (same inputs, same upstream gradient) and one StyledConv with a constant noise
image (same-resolution and up-sampling), it records weight.grad beside the input, latent, noise-strength and bias gradients.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import seeded  # noqa: E402
from make_golden import MODCONV_CASES, _import_reference, _save, modconv_inputs  # noqa: E402

# name, cin, cout, up, B, H  (StyledConv: 3x3, demodulated, NoiseInjection + FusedLeakyReLU with non-zero strength / bias)
STYLED_CASES = [
    ("styled_same", 12, 20, False, 2, 8),
    ("styled_up", 20, 12, True, 2, 5),
]


def styled_inputs(name, cin, cout, b, h, up):
    oh = 2 * h if up else h
    return dict(
        x=seeded.tensor(f"wgrad.{name}.x", (b, cin, h, h)),
        w=seeded.tensor(f"wgrad.{name}.w", (b, 512)),
        weight=seeded.tensor(f"wgrad.{name}.weight", (1, cout, cin, 3, 3)),
        mod_w=seeded.tensor(f"wgrad.{name}.mod_w", (cin, 512)),
        mod_b=seeded.tensor(f"wgrad.{name}.mod_b", (cin,), 0.05, 1.0),
        noise=seeded.tensor(f"wgrad.{name}.noise", (1, 1, oh, oh)),
        noise_w=seeded.tensor(f"wgrad.{name}.noise_w", (1,), 0.1),
        bias=seeded.tensor(f"wgrad.{name}.bias", (cout,), 0.1),
    )


def main():
    ref_model, _, _, _, _ = _import_reference()
    out = {}
    for name, cin, cout, k, demod, up, b, h in MODCONV_CASES:
        i = modconv_inputs(name, cin, cout, k, b, h)
        m = ref_model.ModulatedConv2d(cin, cout, k, 512, demodulate=demod, upsample=up)
        sd = {"weight": i["weight"], "modulation.weight": i["mod_w"], "modulation.bias": i["mod_b"]}
        if up:
            sd["blur.kernel"] = seeded.fir_kernel(gain=4.0)
        m.load_state_dict(sd, strict=True)
        x = i["x"].clone().requires_grad_(True)
        w = i["w"].clone().requires_grad_(True)
        y, _ = m(x, w)
        gy = seeded.tensor(f"modconv.{name}.gy", y.shape)
        gx, gw, gweight = torch.autograd.grad(y, (x, w, m.weight), gy)
        out[f"{name}.gx"], out[f"{name}.gw"], out[f"{name}.gweight"] = gx, gw, gweight
    for name, cin, cout, up, b, h in STYLED_CASES:
        i = styled_inputs(name, cin, cout, b, h, up)
        m = ref_model.StyledConv(cin, cout, 3, 512, upsample=up)
        sd = {"conv.weight": i["weight"], "conv.modulation.weight": i["mod_w"], "conv.modulation.bias": i["mod_b"],
              "noise.weight": i["noise_w"], "activate.bias": i["bias"]}
        if up:
            sd["conv.blur.kernel"] = seeded.fir_kernel(gain=4.0)
        m.load_state_dict(sd, strict=True)
        x = i["x"].clone().requires_grad_(True)
        w = i["w"].clone().requires_grad_(True)
        y, _ = m(x, w, noise=i["noise"])  # (this fork returns (out, style), model.py:336-340)
        gy = seeded.tensor(f"wgrad.{name}.gy", y.shape)
        gx, gw, gweight, gnoise, gbias = torch.autograd.grad(y, (x, w, m.conv.weight, m.noise.weight, m.activate.bias), gy)
        out[f"{name}.y"] = y
        out[f"{name}.gx"], out[f"{name}.gw"], out[f"{name}.gweight"] = gx, gw, gweight
        out[f"{name}.g_noise"], out[f"{name}.g_bias"] = gnoise, gbias
    _save("modconv_wgrad", **out)


if __name__ == "__main__":
    main()
