"""Generates tests/golden/perceptual.npz by running the REFERENCE's VGG16 perceptual loss (criteria/perceptual_loss.py) in this
container.

    python tests/golden/make_golden_perceptual.py        (needs /root/reference; never runs on the GPU box)

criteria/perceptual_loss.py imports torchvision, which is absent from this image.  A stub module stands in for it in sys.modules:
its `models.vgg16(pretrained=True).features` is the published VGG16 configuration-D layer list (Conv2d(., ., 3, padding=1),
ReLU(inplace=True), MaxPool2d(2, 2)) with the seeded weights of `vgg_features_state_dict()` instead of the pretrained file.
`.to('cuda:N')` is the identity, so everything runs on the CPU in fp32.

Two groups of cases:
  * loss.*  PerceptualLoss at stylegan_size 256 (7x up-sample, AvgPool 8 -> 224^2): image1 batch 2 against a target repeated from
            one sample; the loss and d loss / d image1 (at seeded positions, plus its sum and sum of squares: the full gradient
            would not fit the fixture budget);
  * vgg.*   Vgg16 on a [2,3,32,32] input: the four outputs and the input gradient of sum(relu2_2 * r) for a seeded r.
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
import seeded  # noqa: E402

# VGG16 configuration D (torchvision.models.vgg16().features): channel counts, "M" = MaxPool2d(2, 2)
CFG_D = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)  # the ten convolutions of features[:23]
SLICE_OF = {i: 1 if i < 4 else 2 if i < 9 else 3 if i < 16 else 4 for i in CONV_INDICES}
SIZE = 256
LOSS_BATCH = 2
VGG_SHAPE = (2, 3, 32, 32)
GRAD_SAMPLES = 16384


def vgg_features_state_dict():
    """Seeded weights of every convolution of CFG_D in torchvision's layout (`features.{i}.weight` / `.bias`): He-scaled
    (std sqrt(2 / fan_in)) so that activations keep their scale through the ReLUs, and non-zero biases."""
    sd, cin, i = {}, 3, 0
    for v in CFG_D:
        if v == "M":
            i += 1
            continue
        sd[f"features.{i}.weight"] = seeded.tensor(f"vgg.features.{i}.weight", (v, cin, 3, 3), math.sqrt(2.0 / (cin * 9)))
        sd[f"features.{i}.bias"] = seeded.tensor(f"vgg.features.{i}.bias", (v,), 0.05)
        cin, i = v, i + 2
    return sd


def vgg_state_dict():
    """The same weights under Vgg16's own keys (`slice{k}.{i}.weight` / `.bias`, the 20 tensors of features[:23])."""
    sd = vgg_features_state_dict()
    return {f"slice{SLICE_OF[i]}.{i}.{kind}": sd[f"features.{i}.{kind}"] for i in CONV_INDICES for kind in ("weight", "bias")}


def loss_inputs():
    """image1 [2,3,256,256] in (-1, 1) and the target: sample 0 of another batch, repeated (the region-attention loop's first_img)."""
    img1 = torch.tanh(seeded.tensor("perc.img1", (LOSS_BATCH, 3, SIZE, SIZE), 0.8))
    target = torch.tanh(seeded.tensor("perc.img2", (1, 3, SIZE, SIZE), 0.8))
    return img1, target


def vgg_inputs():
    x = torch.tanh(seeded.tensor("perc.vgg_x", VGG_SHAPE, 0.8))
    r = seeded.tensor("perc.vgg_r", (VGG_SHAPE[0], 128, VGG_SHAPE[2] // 2, VGG_SHAPE[3] // 2))
    return x, r


def grad_positions(numel):
    return seeded.sample_positions(numel, GRAD_SAMPLES, "perc.grad_positions")


def _stub_torchvision():
    def vgg16(pretrained=False, **kw):
        layers, cin = [], 3
        for v in CFG_D:
            if v == "M":
                layers.append(torch.nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [torch.nn.Conv2d(cin, v, kernel_size=3, padding=1), torch.nn.ReLU(inplace=True)]
                cin = v
        features = torch.nn.Sequential(*layers)
        features.load_state_dict({k[len("features."):]: v for k, v in vgg_features_state_dict().items()}, strict=True)
        return types.SimpleNamespace(features=features)

    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.vgg16 = vgg16
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tv.models


def import_reference_loss():
    _stub_torchvision()
    torch.nn.Module.to = lambda self, *a, **k: self
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)
    from criteria import perceptual_loss
    return perceptual_loss


def main():
    pl = import_reference_loss()
    torch.manual_seed(0)
    loss_mod = pl.PerceptualLoss(types.SimpleNamespace(gpu=0, stylegan_size=SIZE))
    assert sorted("model." + k for k in vgg_state_dict()) == sorted(loss_mod.state_dict())
    img1, target = loss_inputs()
    x1 = img1.clone().requires_grad_(True)
    loss = loss_mod(x1, target.repeat(LOSS_BATCH, 1, 1, 1))
    (g1,) = torch.autograd.grad(loss, x1)
    pos = grad_positions(g1.numel())
    store = {"loss.value": np.float64(loss.item()), "loss.grad_at": g1.reshape(-1)[pos].numpy(),
             "loss.grad_sum": np.float64(g1.double().sum().item()), "loss.grad_sumsq": np.float64(g1.double().pow(2).sum().item()),
             "keys": np.asarray(sorted(loss_mod.state_dict()))}
    vgg = pl.Vgg16(requires_grad=False)
    x, r = vgg_inputs()
    xg = x.clone().requires_grad_(True)
    out = vgg(xg)
    (gx,) = torch.autograd.grad((out.relu2_2 * r).sum(), xg)
    for name in out._fields:
        store["vgg." + name] = getattr(out, name).detach().numpy()
    store["vgg.grad"] = gx.numpy()
    path = os.path.join(HERE, "perceptual.npz")
    np.savez_compressed(path, **store)
    print("saved", path, os.path.getsize(path), "bytes; loss", loss.item(), "grad max", g1.abs().max().item())


if __name__ == "__main__":
    main()
