"""CPU tests of the R1 gradient penalty's surface: the new C entry points refuse bad arguments before any HIP call, the header, the
exports and the ctypes table agree on them, r1_penalty has no CPU path, and the float64 yardstick (tests/r1_ref.py) is itself what
rosinality's d_r1_loss computes."""
import ctypes
import os
import re

import pytest
import torch

import disc64
import r1_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["w2e_fromrgb_jvp", "w2e_mbstd_hvp", "w2e_mbstd_jvp", "w2e_sumsq_rows", "w2e_sumsq_rows_parts"]


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in NEW:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


def test_header_exports_and_prototypes_agree(lib):
    from where2edit_amd import _lib
    header = open(os.path.join(ROOT, "include", "w2e.h")).read()
    declared = re.findall(r"^\s*int\s+(w2e_(?:fromrgb_jvp|mbstd_jvp|mbstd_hvp|sumsq_rows\w*))\s*\(([^;]*)\);", header, flags=re.M | re.S)
    assert sorted(n for n, _ in declared) == NEW
    for name, args in declared:
        assert hasattr(lib, name) and name in _lib._PROTOS
        assert len(_lib._PROTOS[name][1]) == len(args.split(",")), name  # one ctypes type per declared argument


def test_entries_refuse_bad_arguments_without_a_gpu(lib):
    d = ctypes.c_void_p(4096)  # a non-null dummy address: every refusal comes before any HIP call
    err = lambda: lib.w2e_last_error()  # noqa: E731
    # null tensors
    assert lib.w2e_fromrgb_jvp(None, d, d, d, 1, 32, 64, 1.0, None) != 0 and b"fromrgb_jvp: null" in err()
    assert lib.w2e_fromrgb_jvp(d, d, d, None, 1, 32, 64, 1.0, None) != 0 and b"fromrgb_jvp: null" in err()
    assert lib.w2e_mbstd_jvp(d, None, d, 4, 512, 16, None) != 0 and b"mbstd_jvp: null" in err()
    assert lib.w2e_mbstd_hvp(d, d, d, None, 4, 512, 16, None) != 0 and b"mbstd_hvp: null" in err()
    assert lib.w2e_sumsq_rows(d, None, d, 4, 64, None) != 0 and b"sumsq_rows: null" in err()
    # a batch that is not a multiple of its stddev group
    for b in (6, 10):
        assert lib.w2e_mbstd_jvp(d, d, d, b, 512, 16, None) != 0 and b"mbstd_jvp: batch" in err() and b"multiple of the stddev group" in err()
        assert lib.w2e_mbstd_hvp(d, d, d, d, b, 512, 16, None) != 0 and b"mbstd_hvp: batch" in err() and b"multiple of the stddev group" in err()
    # non-positive sizes (and more channels than fromRGB's table holds)
    for b, c, hw in ((0, 32, 64), (1, 0, 64), (1, 32, 0), (-1, 32, 64), (1, 513, 64)):
        assert lib.w2e_fromrgb_jvp(d, d, d, d, b, c, hw, 1.0, None) != 0 and b"fromrgb_jvp: bad dims" in err()
    for b, c, hw in ((0, 512, 16), (4, 0, 16), (4, 512, 0), (4, -512, 16)):
        assert lib.w2e_mbstd_jvp(d, d, d, b, c, hw, None) != 0 and b"mbstd_jvp: bad dims" in err()
        assert lib.w2e_mbstd_hvp(d, d, d, d, b, c, hw, None) != 0 and b"mbstd_hvp: bad dims" in err()
    for b, n in ((0, 64), (4, 0), (4, -3), (-1, 64)):
        assert lib.w2e_sumsq_rows(d, d, d, b, n, None) != 0 and b"sumsq_rows: bad dims" in err()
    assert lib.w2e_sumsq_rows_parts(0) == 0 and lib.w2e_sumsq_rows_parts(-5) == 0
    assert lib.w2e_sumsq_rows_parts(1) == 1 and lib.w2e_sumsq_rows_parts(3 * 1024 * 1024) == 768


def test_r1_penalty_has_no_cpu_path():
    import where2edit_amd
    from where2edit_amd import disc_hip
    from where2edit_amd.stylegan2 import Discriminator
    d = Discriminator(8, 2)
    x = torch.zeros(4, 3, 8, 8)
    for fn in (d.r1_penalty, lambda t: disc_hip.r1_penalty(d, t), lambda t: where2edit_amd.r1_penalty(d, t)):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(x)
    with pytest.raises(ValueError, match="multiple of the stddev group"):  # the batch rule of the stddev layer, before any kernel
        d.r1_penalty(torch.zeros(6, 3, 8, 8))
    with pytest.raises(ValueError, match=r"\[B,3,S,S\]"):
        d.r1_penalty(torch.zeros(4, 1, 8, 8))


def test_yardstick_is_the_reference_loss_and_its_zero_biases():
    """r1_ref.penalty against the loss written out the way rosinality's d_r1_loss writes it, at a size the CPU does in a blink; the
    two biases behind the stddev layer get exact zeros and final_linear.1.bias is unused."""
    size, cm, b = 8, 2, 4
    sd = disc64.state_dict(size, cm, salt=5)
    x = disc64.images(b, size, salt=5)
    r1, grads, _ = r1_ref.penalty(sd, x)
    xx = x.double().requires_grad_(True)
    (g,) = torch.autograd.grad(outputs=disc64.forward(sd, xx).sum(), inputs=xx, create_graph=True)
    assert torch.equal(r1, g.pow(2).reshape(g.shape[0], -1).sum(1).mean().detach())
    assert grads["final_linear.1.bias"] is None
    for k in ("final_conv.1.bias", "final_linear.0.bias"):
        assert grads[k] is None or int(torch.count_nonzero(grads[k])) == 0, k
    assert all(grads[k] is not None and float(grads[k].abs().max()) > 0 for k in grads if not k.endswith(".bias"))
    assert float(grads["convs.0.1.bias"].abs().max()) > 0  # the stddev layer's second-order term reaches the earlier biases


def test_stddev_tangent_helper_matches_finite_differences():
    x = torch.randn(4, 3, 4, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    dx = torch.randn(4, 3, 4, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    lam = torch.randn(4, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    jv, mu = r1_ref.stddev_jvp_hvp(x, dx, lam)
    eps = 1e-6
    fd = (r1_ref.stddev(x + eps * dx) - r1_ref.stddev(x - eps * dx)) / (2 * eps)
    assert float((fd - jv).abs().max()) <= 1e-8 * max(1.0, float(jv.abs().max()))
    probe = torch.randn(4, 3, 4, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    jp, _ = r1_ref.stddev_jvp_hvp(x + eps * probe, dx, lam)
    jm, _ = r1_ref.stddev_jvp_hvp(x - eps * probe, dx, lam)
    assert abs(float(((jp - jm) * lam).sum() / (2 * eps)) - float((mu * probe).sum())) <= 1e-6 * max(1.0, float(mu.abs().max()))
