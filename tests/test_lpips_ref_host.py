"""LPIPS-VGG v0.1 without a GPU: the float64 restatement the GPU tests compare against (tests/lpips_ref.py) checked against
autograd, a hand-computed case and its own symmetries; the module surface of where2edit_amd.lpips (state_dict keys, the accepted file
layouts, every refusal that needs no GPU); the argument checks of the two C entry points; and the fact the whole-module gradient
comparison rests on: the seeded network produces no zero-norm pixel at the sizes the GPU tests use."""
import ctypes

import pytest
import torch

import lpips_ref as R
import seeded
from helpers import rel_err

HEAD_SHAPES = [(64, 1, 1), (64, 3, 5), (128, 17, 23), (256, 8, 8), (512, 2, 2), (512, 14, 14)]


def _features(key, c, h, w, batch=2):
    return torch.relu(seeded.tensor(key, (batch, c, h, w))).double()


def _lin(key, c):
    return seeded.tensor(key, (c,)).abs().double() / c


@pytest.fixture(scope="module")
def seeded_model():
    from where2edit_amd.lpips import LPIPS
    return LPIPS()


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_closed_form_head_gradient_equals_float64_autograd(shape):
    c, h, w = shape
    f0 = (_features(f"lp.h.f0{shape}", c, h, w) + 0.05).requires_grad_(True)  # (+0.05: no zero-norm pixel, autograd is defined)
    f1 = (_features(f"lp.h.f1{shape}", c, h, w) + 0.05).requires_grad_(True)
    lin, gout = _lin(f"lp.h.w{shape}", c), seeded.tensor(f"lp.h.g{shape}", (2,)).double()
    a0, a1 = torch.autograd.grad((R.head(f0, f1, lin) * gout).sum(), [f0, f1])
    g0, g1 = R.head_grad(f0.detach(), f1.detach(), lin, gout)
    assert rel_err(g0, a0) <= 1e-10 and rel_err(g1, a1) <= 1e-10
    # a broadcast f1: its gradient is the sum over the batch
    fb = f1.detach()[:1].clone().requires_grad_(True)
    a0, ab = torch.autograd.grad((R.head(f0, fb, lin) * gout).sum(), [f0, fb])
    g0, gb = R.head_grad(f0.detach(), fb.detach(), lin, gout)
    assert rel_err(g0, a0) <= 1e-10 and rel_err(gb, ab) <= 1e-10


def test_head_by_hand_one_pixel_two_channels():
    """f0 = (3, 4), f1 = (0, 2), w = (1, 1/2): u0 = (.6, .8), u1 = (0, 1), e = (.6, -.2), d = .36 + .02 = .38;
    q = 2 w e = (1.2, -.2), sum q f0 = 2.8, sum q f1 = -.4:
    d/df0 = q / 5 - f0 2.8 / 125 = (.1728, -.1296)  (orthogonal to f0);  d/df1 = -q / 2 + f1 (-.4) / 8 = (-.6, 0)."""
    f0 = torch.tensor([3.0, 4.0], dtype=torch.float64).reshape(1, 2, 1, 1)
    f1 = torch.tensor([0.0, 2.0], dtype=torch.float64).reshape(1, 2, 1, 1)
    lin = torch.tensor([1.0, 0.5], dtype=torch.float64)
    assert abs(R.head(f0, f1, lin).item() - 0.38) <= 1e-9
    assert abs(R.head_expansion(f0, f1, lin).item() - 0.38) <= 1e-9
    g0, g1 = R.head_grad(f0, f1, lin, torch.ones(1, dtype=torch.float64))
    assert torch.allclose(g0.reshape(-1), torch.tensor([0.1728, -0.1296], dtype=torch.float64), rtol=0, atol=1e-9)
    assert torch.allclose(g1.reshape(-1), torch.tensor([-0.6, 0.0], dtype=torch.float64), rtol=0, atol=1e-9)


def test_head_is_zero_on_equal_inputs_symmetric_and_finite_at_zero_norm():
    f0, f1 = _features("lp.sym.f0", 64, 5, 7), _features("lp.sym.f1", 64, 5, 7)
    lin = _lin("lp.sym.w", 64)
    assert torch.all(R.head(f0, f0, lin) == 0)
    assert torch.equal(R.head(f0, f1, lin), R.head(f1, f0, lin))
    # planted zero-norm pixels: u = 0 there, the gradient's second term is 0 by convention, everything stays finite
    f0[:, :, 0, 0] = 0
    f1[:, :, 0, 1] = 0
    f0[:, :, 1, 1] = f1[:, :, 1, 1] = 0
    d = R.head(f0, f1, lin)
    g0, g1 = R.head_grad(f0, f1, lin, torch.ones(2, dtype=torch.float64))
    assert torch.isfinite(d).all() and torch.isfinite(g0).all() and torch.isfinite(g1).all()
    assert not (g0 * (f0 > 0))[:, :, 0, 0].any() and not (g1 * (f1 > 0))[:, :, 0, 1].any()
    assert not g0[:, :, 1, 1].any() and not g1[:, :, 1, 1].any()
    # where only f0 vanishes, u1 alone is left: that pixel contributes sum_c w_c u1_c^2 / pixels
    u1 = R.unit(f1)[0]
    only = (lin.reshape(1, -1) * u1[:, :, 0, 0] ** 2).sum(1) / 35
    rest0, rest1 = f0.clone(), f1.clone()
    rest0[:, :, 0, 0] = rest1[:, :, 0, 0] = 0
    assert torch.allclose(d - R.head(rest0, rest1, lin), only, rtol=1e-9, atol=1e-15)


@pytest.mark.parametrize("shape", [(64, 17, 23), (512, 14, 14), (512, 1, 1)])
def test_difference_form_holds_in_fp32_where_the_expansion_cancels(shape):
    """Why the kernels use sum w (u0 - u1)^2: on near-equal inputs, evaluated in fp32, it stays within 1e-6 of float64 and the
    expansion does not."""
    c, h, w = shape
    f0 = torch.relu(seeded.tensor(f"lp.near.f0{shape}", (2, c, h, w)))
    f1 = torch.relu(f0 + 0.01 * seeded.tensor(f"lp.near.n{shape}", (2, c, h, w)))
    lin = _lin(f"lp.near.w{shape}", c)
    ref = R.head(f0.double(), f1.double(), lin)
    diff = rel_err(R.head(f0, f1, lin.float()), ref)
    expansion = rel_err(R.head_expansion(f0, f1, lin.float()), ref)
    print(f"{shape}: difference form {diff:.2e}, expansion {expansion:.2e} from float64")
    assert diff <= 1e-6 and expansion > 10 * diff


def test_scaling_constants():
    from where2edit_amd import lpips as L
    assert L.SHIFT == R.SHIFT == (-.030, -.088, -.188) and L.SCALE == R.SCALE == (.458, .448, .450)
    x = torch.zeros(1, 3, 2, 2, dtype=torch.float64)
    assert torch.allclose(R.scaling(x)[0, :, 0, 0], torch.tensor([.030 / .458, .088 / .448, .188 / .450], dtype=torch.float64), rtol=1e-15, atol=0)


def test_lpips_of_an_image_with_itself_is_zero_and_the_distance_is_symmetric(seeded_model):
    sd = {k: v.double() for k, v in seeded_model.state_dict().items()}
    x = torch.tanh(seeded.tensor("lp.ref.x", (2, 3, 16, 16), 0.8)).double()
    y = torch.tanh(seeded.tensor("lp.ref.y", (2, 3, 16, 16), 0.8)).double()
    assert torch.all(R.lpips(sd, x, x)[0] == 0)
    dxy, dyx = R.lpips(sd, x, y)[0], R.lpips(sd, y, x)[0]
    assert torch.all(dxy > 0) and torch.allclose(dxy, dyx, rtol=1e-12, atol=0)
    assert torch.allclose(R.lpips(sd, x, y[:1])[0][0], dxy[0], rtol=1e-12, atol=0)  # a batch-1 in1 is broadcast


@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (2, 3, 32, 32), (2, 3, 33, 47), (1, 3, 64, 48)])
def test_seeded_network_has_no_zero_norm_pixel(seeded_model, shape):
    """The premise of the GPU tests' whole-module gradient comparison (autograd and the convention differ only at such pixels), on
    the very inputs those tests use."""
    sd = seeded_model.state_dict()
    assert R.zero_norm_pixels(sd, torch.cat(R.inputs(shape))) == [0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- the module surface
KEYS = [
    "scaling_layer.shift", "scaling_layer.scale",
    "net.slice1.0.weight", "net.slice1.0.bias", "net.slice1.2.weight", "net.slice1.2.bias",
    "net.slice2.5.weight", "net.slice2.5.bias", "net.slice2.7.weight", "net.slice2.7.bias",
    "net.slice3.10.weight", "net.slice3.10.bias", "net.slice3.12.weight", "net.slice3.12.bias", "net.slice3.14.weight", "net.slice3.14.bias",
    "net.slice4.17.weight", "net.slice4.17.bias", "net.slice4.19.weight", "net.slice4.19.bias", "net.slice4.21.weight", "net.slice4.21.bias",
    "net.slice5.24.weight", "net.slice5.24.bias", "net.slice5.26.weight", "net.slice5.26.bias", "net.slice5.28.weight", "net.slice5.28.bias",
    "lin0.model.1.weight", "lin1.model.1.weight", "lin2.model.1.weight", "lin3.model.1.weight", "lin4.model.1.weight",
]


def test_state_dict_keys_shapes_and_seeded_weights(seeded_model):
    from where2edit_amd import LPIPS as exported
    from where2edit_amd.lpips import LPIPS, state_dict_keys
    assert exported is LPIPS
    sd = seeded_model.state_dict()
    assert list(sd) == KEYS == state_dict_keys()
    assert tuple(sd["scaling_layer.shift"].shape) == tuple(sd["scaling_layer.scale"].shape) == (1, 3, 1, 1)
    for k, c in enumerate((64, 128, 256, 512, 512)):
        w = sd[f"lin{k}.model.1.weight"]
        assert tuple(w.shape) == (1, c, 1, 1) and torch.all(w >= 0)
    assert tuple(sd["net.slice5.28.weight"].shape) == (512, 512, 3, 3) and tuple(sd["net.slice1.0.weight"].shape) == (64, 3, 3, 3)
    assert not any(p.requires_grad for p in seeded_model.parameters()) and not seeded_model.training
    w = sd["net.slice2.7.weight"]  # torchvision's init: kaiming_normal_ (fan_out, relu), zero bias
    assert torch.all(sd["net.slice2.7.bias"] == 0) and abs(w.std().item() - (2.0 / (128 * 9)) ** 0.5) < 0.05 * (2.0 / (128 * 9)) ** 0.5
    again, other = LPIPS().state_dict(), LPIPS(seed=1).state_dict()
    assert all(torch.equal(sd[k], again[k]) for k in KEYS) and not torch.equal(sd["lin4.model.1.weight"], other["lin4.model.1.weight"])


def _synthetic_files():
    lin = {f"lin{k}.model.1.weight": seeded.tensor(f"lp.file.lin{k}", (1, c, 1, 1)).abs() for k, c in enumerate((64, 128, 256, 512, 512))}
    convs = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256), 17: (256, 512),
             19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
    tv = {}
    for i, (cin, cout) in convs.items():
        tv[f"features.{i}.weight"] = seeded.tensor(f"lp.file.w{i}", (cout, cin, 3, 3), 0.05)
        tv[f"features.{i}.bias"] = seeded.tensor(f"lp.file.b{i}", (cout,), 0.1)
    tv["classifier.0.bias"] = torch.zeros(8)
    return lin, tv


def test_every_accepted_file_layout_round_trips(tmp_path):
    from where2edit_amd.lpips import LPIPS, vgg_state_dict
    lin, tv = _synthetic_files()
    own = vgg_state_dict(tv)
    assert sorted(own) == sorted(k for k in KEYS if k.startswith("net."))
    layouts = {
        "package": lin,                                                              # weights/v0.1/vgg.pth
        "lins": {k.replace("lin", "lins.", 1): v for k, v in lin.items()},           # the ModuleList alias
    }
    for name, sd in layouts.items():
        torch.save(sd, tmp_path / f"{name}.pth")
        got = LPIPS(model_path=str(tmp_path / f"{name}.pth")).state_dict()
        assert all(torch.equal(got[k], lin[k]) for k in lin), name
        assert torch.equal(got["net.slice1.0.weight"], LPIPS().state_dict()["net.slice1.0.weight"])  # the convs keep their init
    for name, sd in (("tv", tv), ("own", own), ("bare", {k[len("net."):]: v for k, v in own.items()})):
        torch.save(sd, tmp_path / f"{name}.pth")
        got = LPIPS(model_path=str(tmp_path / "package.pth"), vgg_weights=str(tmp_path / f"{name}.pth")).state_dict()
        assert list(got) == KEYS and all(torch.equal(got[k], own[k]) for k in own) and all(torch.equal(got[k], lin[k]) for k in lin), name
    # a whole-module state_dict through model_path (with the package's duplicated `lins.*` entries and its scaling buffers)
    whole = dict(got)
    whole.update({k.replace("lin", "lins.", 1): v for k, v in lin.items()})
    torch.save(whole, tmp_path / "whole.pth")
    again = LPIPS(model_path=str(tmp_path / "whole.pth")).state_dict()
    assert all(torch.equal(again[k], got[k]) for k in KEYS)
    # missing and misshapen tensors say what was looked for
    missing = dict(lin)
    del missing["lin3.model.1.weight"]
    torch.save(missing, tmp_path / "missing.pth")
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight.*lins\.3\.model\.1\.weight"):
        LPIPS(model_path=str(tmp_path / "missing.pth"))
    bad = dict(lin)
    bad["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match=r"lin1\.model\.1\.weight has shape"):
        LPIPS(model_path=str(tmp_path / "bad.pth"))
    short = dict(tv)
    del short["features.26.bias"]
    torch.save(short, tmp_path / "short.pth")
    with pytest.raises(KeyError, match=r"net\.slice5\.26\.bias \(looked for features\.26\.bias"):
        LPIPS(vgg_weights=str(tmp_path / "short.pth"))
    wrong = dict(tv)
    wrong["features.24.weight"] = torch.zeros(512, 256, 3, 3)
    torch.save(wrong, tmp_path / "wrong.pth")
    with pytest.raises(RuntimeError, match=r"features\.24\.weight has shape"):
        LPIPS(vgg_weights=str(tmp_path / "wrong.pth"))


def test_refusals_that_need_no_gpu(seeded_model):
    from where2edit_amd.lpips import LPIPS
    for kwargs, word in (({"net": "alex"}, "net"), ({"net": "squeeze"}, "net"), ({"version": "0.0"}, "version"), ({"spatial": True}, "spatial"),
                         ({"lpips": False}, "lpips")):
        with pytest.raises(ValueError, match=word):
            LPIPS(**kwargs)
    x = torch.zeros(2, 3, 32, 32)
    for bad, name in ((torch.zeros(2, 3, 15, 32), "in0"), (torch.zeros(2, 1, 32, 32), "in0"), (torch.zeros(3, 32, 32), "in0")):
        with pytest.raises(ValueError, match=name):
            seeded_model(bad, bad)
    with pytest.raises(ValueError, match="in1"):
        seeded_model(x, torch.zeros(2, 3, 32, 15))
    with pytest.raises(ValueError, match="in1"):  # neither in0's batch nor 1
        seeded_model(torch.zeros(3, 3, 32, 32), x)
    with pytest.raises(ValueError, match="in1"):  # another size
        seeded_model(x, torch.zeros(2, 3, 32, 48))
    with pytest.raises(RuntimeError, match="broadcast"):
        seeded_model(x, torch.zeros(1, 3, 32, 32, requires_grad=True))
    with pytest.raises(RuntimeError, match="GPU only"):  # no CPU path, no stock-op fallback: CPU tensors stop at _lib.ptr
        seeded_model(x, x)
    trainable = LPIPS()
    trainable.lin2.requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"frozen critic.*requires_grad_\(False\)"):
        trainable(x, x)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU only"):  # without grad mode the weights' flags do not matter
        trainable(x, x)


def test_lpips_distance_refuses_bad_arguments_before_touching_the_gpu():
    from where2edit_amd.evaluation import lpips_distance
    a = torch.zeros(3, 32, 32, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="3 .* 2"):
        lpips_distance(a, a[:2], model=object())
    with pytest.raises(ValueError, match="uint8"):
        lpips_distance(a.float(), a.float(), model=object())
    with pytest.raises(ValueError, match="batch"):
        lpips_distance(a, a, model=object(), batch=0)


# ---------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("w2e_lpips_head_fwd", "w2e_lpips_head_bwd"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


def test_argument_errors_of_the_head_entry_points_need_no_gpu(lib):
    d = ctypes.c_void_p(64)  # never dereferenced: every check runs before a launch
    assert lib.w2e_lpips_head_fwd(d, None, d, 2, 2, 64, 16, d, 2048, d, None) != 0 and b"null" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_fwd(d, d, d, 0, 1, 64, 16, d, 2048, d, None) != 0 and b"bad size" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_fwd(d, d, d, 2, 2, 0, 16, d, 2048, d, None) != 0 and b"bad size" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_fwd(d, d, d, 2, 2, 64, 0, d, 2048, d, None) != 0 and b"bad size" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_fwd(d, d, d, 3, 2, 64, 16, d, 3072, d, None) != 0 and b"neither" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_fwd(d, d, d, 2, 2, 64, 16, d, 2047, d, None) != 0 and b"partials slab holds 2047 floats, needs 2048" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_bwd(d, d, d, None, 2, 2, 64, 16, d, None, 0, 1, None) != 0 and b"null" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_bwd(d, d, d, d, 2, 2, 64, 16, None, None, 0, 1, None) != 0 and b"null" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_bwd(d, d, d, d, 2, 3, 64, 16, d, None, 0, 1, None) != 0 and b"neither" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_bwd(d, d, d, d, 2, 1, 64, 16, d, d, 0, 1, None) != 0 and b"equal batches" in lib.w2e_last_error()
    assert lib.w2e_lpips_head_bwd(d, d, d, d, 2, 2, 64, -1, d, None, 0, 1, None) != 0 and b"bad size" in lib.w2e_last_error()
