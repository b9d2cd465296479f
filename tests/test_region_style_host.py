"""The style branch on HIP (csrc/region_style.hip, region_style_hip.py), the parts that need no GPU: the new symbols are declared,
prototyped and exported at ABI version 7; every entry point refuses bad arguments before any launch; `applies` says no to what the
node does not take, and `new_styles` then gives the stock composition's result."""
import ctypes
import os
import re

import pytest
import torch

import region_style_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLE_SYMBOLS = ("w2e_rstyle_linear_fwd", "w2e_rstyle_linear_dgrad", "w2e_rstyle_linear_wgrad", "w2e_rstyle_finish_fwd", "w2e_rstyle_finish_bwd")


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib
    return _lib.load()


def test_symbols_are_declared_prototyped_and_exported_at_version_7(lib):
    from where2edit_amd import _lib
    att = open(os.path.join(ROOT, "include", "w2e_attention.h")).read()
    main = open(os.path.join(ROOT, "include", "w2e.h")).read()
    for name in STYLE_SYMBOLS:
        assert re.search(r"^int\s+" + name + r"\(", att, re.M), f"{name} is not declared in include/w2e_attention.h"
        assert name in _lib._PROTOS, f"{name} has no ctypes prototype"
        assert getattr(lib, name).argtypes == _lib._PROTOS[name][1]
    assert re.search(r"^int\s+w2e_adam_step\(", main, re.M) and "w2e_adam_step" in _lib._PROTOS
    assert lib.w2e_adam_step.argtypes == _lib._PROTOS["w2e_adam_step"][1]
    assert lib.w2e_version() == _lib.header_version() == 7


def _arrays(groups=1, k0=32, k1=0, n=32):
    """Plausible (never dereferenced) arguments: the checks run before any launch."""
    P = lambda v=4096: (ctypes.c_void_p * groups)(*[v] * groups)  # noqa: E731
    I = lambda v: (ctypes.c_int * groups)(*[v] * groups)  # noqa: E731
    F = (ctypes.c_float * groups)(*[1.0] * groups)
    return P, I, F


def _refused(lib, rc, *words):
    assert rc != 0
    msg = lib.w2e_last_error().decode()
    assert all(w in msg for w in words), msg


def test_argument_errors_return_codes_and_messages_without_a_gpu(lib):
    P, I, F = _arrays()
    fwd = lambda groups=1, batch=1, src0=P(), k0=I(32), n=I(32), w=P(): lib.w2e_rstyle_linear_fwd(  # noqa: E731
        groups, batch, src0, P(0), k0, I(0), I(32), I(0), w, P(), P(), n, F, 1.0, I(0), None)
    _refused(lib, fwd(batch=17), "rstyle_linear_fwd", "batch 17")
    _refused(lib, fwd(batch=0), "batch 0")
    _refused(lib, fwd(groups=33), "33 groups")
    _refused(lib, fwd(groups=0), "0 groups")
    _refused(lib, fwd(k0=I(0)), "k0 0")
    _refused(lib, fwd(n=I(-3)), "n -3")
    _refused(lib, fwd(src0=P(0)), "null pointer")
    _refused(lib, fwd(w=None), "null argument")
    dgrad = lambda batch=1, gy=P(), gx0=P(), n=I(32): lib.w2e_rstyle_linear_dgrad(1, batch, gy, P(), P(), gx0, P(0), I(32), I(0), n, F, I(0), None)  # noqa: E731
    _refused(lib, dgrad(batch=17), "rstyle_linear_dgrad", "batch 17")
    _refused(lib, dgrad(gy=P(0)), "null pointer")
    _refused(lib, dgrad(gx0=P(0)), "asks for no gradient")
    _refused(lib, dgrad(batch=16, n=I(4096)), "does not fit")
    wgrad = lambda batch=1, gw=P(), k0=I(32): lib.w2e_rstyle_linear_wgrad(1, batch, P(), P(), P(), P(0), k0, I(0), I(32), I(0), gw, P(), I(32),  # noqa: E731
                                                                          F, 1.0, I(0), None)
    _refused(lib, wgrad(batch=17), "rstyle_linear_wgrad", "batch 17")
    _refused(lib, wgrad(gw=P(0)), "null pointer")
    _refused(lib, wgrad(k0=I(64)), "row stride")
    ffwd = lambda batch=1, dims=I(32), norms=4096, layers=1: lib.w2e_rstyle_finish_fwd(1, batch, P(), I(64), P(), P(), dims, 0.1, layers, norms, 4096, None)  # noqa: E731
    _refused(lib, ffwd(batch=17), "rstyle_finish_fwd", "batch 17")
    _refused(lib, ffwd(dims=I(0)), "width 0")
    _refused(lib, ffwd(norms=None), "norms")
    _refused(lib, ffwd(layers=0), "layers")
    fbwd = lambda batch=1, norms=4096, x=P(): lib.w2e_rstyle_finish_bwd(1, batch, x, I(64), P(), P(0), norms, None, P(), I(32), 0.1, 1, None)  # noqa: E731
    _refused(lib, fbwd(batch=17), "rstyle_finish_bwd", "batch 17")
    _refused(lib, fbwd(norms=None), "norms")
    _refused(lib, fbwd(x=P(0)), "null pointer")
    one = (ctypes.c_void_p * 1)(4096)
    n1 = (ctypes.c_int64 * 1)(8)
    _refused(lib, lib.w2e_adam_step(1, None, one, one, one, n1, 0.9, 0.999, 1e-8, 1e-3, 1.0, 0.0, None), "adam_step", "null argument")
    _refused(lib, lib.w2e_adam_step(1, one, one, (ctypes.c_void_p * 1)(0), one, n1, 0.9, 0.999, 1e-8, 1e-3, 1.0, 0.0, None), "null pointer")
    _refused(lib, lib.w2e_adam_step(1, one, one, one, one, (ctypes.c_int64 * 1)(-1), 0.9, 0.999, 1e-8, 1e-3, 1.0, 0.0, None), "elements")
    _refused(lib, lib.w2e_adam_step(1, one, one, one, one, n1, 0.9, 0.999, 1e-8, 1e-3, 0.0, 0.0, None), "bias_correction2_sqrt")
    assert lib.w2e_adam_step(0, None, None, None, None, None, 0.9, 0.999, 1e-8, 1e-3, 1.0, 0.0, None) == 0  # nothing to do is no error


def _cpu_lrelu(monkeypatch):
    """The stock modules' fused bias + LeakyReLU is a GPU op; its torch spelling lets the stock composition run on the CPU."""
    from where2edit_amd import stylegan2
    monkeypatch.setattr(stylegan2, "fused_leaky_relu",
                        lambda x, b, negative_slope=0.2, scale=2 ** 0.5: torch.nn.functional.leaky_relu(x + b, negative_slope) * scale)


def _case(batch=2, dims=(64, 32), embed=32, extra=1):
    params = R.make_params("rshost", dims, embed)
    x = R.make_inputs("rshost", batch, dims, embed, extra)
    return params, x, R.style_net(params, dims, embed, len(dims))


def test_applies_says_no_and_new_styles_is_then_the_stock_result(monkeypatch):
    from where2edit_amd import region_style_hip as RS
    _cpu_lrelu(monkeypatch)
    params, x, net = _case()
    x_text = x[0][:, 0, :32]
    assert RS.applies(net, x, x_text) is None, "CPU tensors"
    # the conditions that are about shapes and structure hold whatever the device (tests/test_gpu_region_style.py repeats them on the GPU)
    p17, x17, net17 = _case(batch=17)
    assert RS.applies(net17, x17, x17[0][:, 0, :32]) is None, "B = 17"
    d33 = [32] * 33
    par33 = R.make_params("rshost33", d33, 32)
    x33 = R.make_inputs("rshost33", 1, d33, 32)
    assert RS.applies(R.style_net(par33, d33, 32, 33), x33, x33[0][:, 0, :32]) is None, "33 codes"
    xg = [t.clone().requires_grad_() for t in x]
    assert RS.applies(net, xg, x_text) is None, "an input that requires grad"
    foreign = R.style_net(params, (64, 32), 32, 2)
    foreign.mapper_text_1 = torch.nn.Linear(32, 512)
    assert RS.applies(foreign, x, x_text) is None, "a module with a foreign structure"
    assert RS.new_styles(net, x, x_text, 0.1) is None
    out, loss = net.new_styles(x, x_text, 0.1)
    ref_out, ref_loss, _ = R.stock_composition(params, x, 0.1, 2, 32, dtype=torch.float32)
    assert len(out) == 3 and [tuple(o.shape) for o in out] == [(2, 1, 64, 1, 1), (2, 1, 32, 1, 1), (2, 1, 32, 1, 1)]
    for o, r in zip(out[:2], ref_out):
        torch.testing.assert_close(o[..., 0, 0], r, rtol=1e-5, atol=1e-6)
    assert torch.equal(out[2][..., 0, 0], x[2][:, :, 32:]), "a code at or above mapper_layer passes through"
    torch.testing.assert_close(loss, ref_loss, rtol=1e-5, atol=1e-7)


def test_stock_switch_is_read_at_call_time(monkeypatch):
    """W2E_RSTYLE_STOCK=1 makes `applies` say no before it looks at anything else (the GPU test checks that no kernel is then called)."""
    from where2edit_amd import region_style_hip as RS
    looked = []
    monkeypatch.setattr(RS.torch, "is_tensor", lambda t: looked.append(1) or True)
    params, x, net = _case()
    monkeypatch.setenv("W2E_RSTYLE_STOCK", "1")
    assert RS.applies(net, x, x[0][:, 0, :32]) is None and not looked
    monkeypatch.delenv("W2E_RSTYLE_STOCK")
    assert RS.applies(net, x, x[0][:, 0, :32]) is None and looked  # (CPU tensors: still no, but now because it looked)
