"""Decoder fine-tuning, host side (no GPU): the conv-weight-gradient fixture against the oracle's float64 autograd, the
train_conv_weights / freeze_conv_weights opt-in, and the K1d entry points of the C ABI (version 7)."""
import ctypes
import os
import re

import pytest
import torch

import seeded
from helpers import assert_close, golden
from make_golden import MODCONV_CASES, modconv_inputs
from make_golden_wgrad import STYLED_CASES, styled_inputs
from oracle import stylegan2 as OG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("w2e_modconv_wgrad_plan", "w2e_modconv_wgrad", "w2e_modconv_wgrad_finish", "w2e_modconv_wsq")


def _d(t):
    return t.to(torch.float64)


@pytest.mark.parametrize("case", MODCONV_CASES, ids=[c[0] for c in MODCONV_CASES])
def test_oracle_float64_weight_gradient_reproduces_the_fixture(case):
    name, cin, cout, k, demod, up, b, h = case
    g = golden("modconv_wgrad")
    i = modconv_inputs(name, cin, cout, k, b, h)
    weight = _d(i["weight"]).requires_grad_(True)
    x, w = _d(i["x"]).requires_grad_(True), _d(i["w"]).requires_grad_(True)
    y, _ = OG.modulated_conv2d(x, w, weight, _d(i["mod_w"]), _d(i["mod_b"]), demodulate=demod, upsample=up,
                               blur_kernel=_d(seeded.fir_kernel(gain=4.0)) if up else None)
    gy = _d(seeded.tensor(f"modconv.{name}.gy", y.shape))
    gx, gw, gweight = torch.autograd.grad(y, (x, w, weight), gy)
    assert_close(gweight, g[f"{name}.gweight"], 1e-5, f"{name} gweight")
    assert_close(gx, g[f"{name}.gx"], 1e-5, f"{name} gx")
    assert_close(gw, g[f"{name}.gw"], 1e-5, f"{name} gw")


@pytest.mark.parametrize("case", STYLED_CASES, ids=[c[0] for c in STYLED_CASES])
def test_oracle_float64_styled_conv_gradients_reproduce_the_fixture(case):
    name, cin, cout, up, b, h = case
    g = golden("modconv_wgrad")
    i = {k: _d(v) for k, v in styled_inputs(name, cin, cout, b, h, up).items()}
    sd = {"l.conv.weight": i["weight"].requires_grad_(True), "l.conv.modulation.weight": i["mod_w"], "l.conv.modulation.bias": i["mod_b"],
          "l.noise.weight": i["noise_w"].requires_grad_(True), "l.activate.bias": i["bias"].requires_grad_(True)}
    if up:
        sd["l.conv.blur.kernel"] = _d(seeded.fir_kernel(gain=4.0))
    x, w = i["x"].requires_grad_(True), i["w"].requires_grad_(True)
    y, _ = OG.styled_conv(sd, "l", x, w, i["noise"], upsample=up, input_is_stylespace=False)
    gy = _d(seeded.tensor(f"wgrad.{name}.gy", y.shape))
    grads = torch.autograd.grad(y, (x, w, sd["l.conv.weight"], sd["l.noise.weight"], sd["l.activate.bias"]), gy)
    assert_close(y, g[f"{name}.y"], 1e-5, f"{name} y")
    for got, key in zip(grads, ("gx", "gw", "gweight", "g_noise", "g_bias")):
        assert_close(got, g[f"{name}.{key}"], 1e-5, f"{name} {key}")


def _conv_weights(g):
    from where2edit_amd.stylegan2 import ModulatedConv2d
    return {id(m.weight) for m in g.modules() if isinstance(m, ModulatedConv2d)}


def test_train_and_freeze_conv_weights_touch_exactly_the_conv_weights():
    import where2edit_amd
    from where2edit_amd.stylegan2 import Generator, ModulatedConv2d, freeze_conv_weights, train_conv_weights
    assert where2edit_amd.train_conv_weights.__doc__
    g = Generator(16, 512, 2)
    g.requires_grad_(False)
    conv = _conv_weights(g)
    assert len(conv) == 5 + 3  # 5 styled convs + 3 ToRGB at 16^2
    assert where2edit_amd.train_conv_weights(g) is g
    for p in g.parameters():
        assert p.requires_grad == (id(p) in conv)
    assert all(m._train_weight for m in g.modules() if isinstance(m, ModulatedConv2d))
    g.requires_grad_(True)
    freeze_conv_weights(g)
    for p in g.parameters():
        assert p.requires_grad == (id(p) not in conv)
    assert not any(m._train_weight for m in g.modules() if isinstance(m, ModulatedConv2d))
    train_conv_weights(g.convs[0])  # a sub-module: only its own layer
    assert [m._train_weight for m in g.modules() if isinstance(m, ModulatedConv2d)].count(True) == 1


def test_trainable_weight_without_the_opt_in_is_still_refused():
    from where2edit_amd.stylegan2 import ModulatedConv2d, freeze_conv_weights, train_conv_weights
    m = ModulatedConv2d(8, 8, 3, 512)
    x, w = torch.randn(1, 8, 4, 4), torch.randn(1, 512)
    with pytest.raises(RuntimeError, match="freeze_conv_weights.*train_conv_weights"):
        m(x, w)
    train_conv_weights(m)
    freeze_conv_weights(m)
    m.weight.requires_grad_(True)  # requires grad again, but the opt-in was cleared
    with pytest.raises(RuntimeError, match="freeze_conv_weights"):
        m(x, w)
    train_conv_weights(m)
    with pytest.raises(RuntimeError, match="GPU only"):  # opted in: the kernels' door, no CPU path
        m(x, w)


def test_new_entry_points_are_declared_prototyped_and_exported():
    from where2edit_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "w2e.h")).read()
    lib = ctypes.CDLL(build.build(verbose=False))
    for n in NEW:
        assert re.search(rf"^int\s+{n}\s*\(", header, re.M), n
        assert n in _lib._PROTOS, n
        assert hasattr(lib, n), n


def test_abi_version_is_7():
    from where2edit_amd import _lib, build
    assert _lib.header_version() == 7
    assert ctypes.CDLL(build.build(verbose=False)).w2e_version() == 7
