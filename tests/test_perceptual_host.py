"""The VGG16 perceptual loss (criteria/perceptual_loss.py, where2edit_amd.perceptual_loss) without a GPU: the float64 / fp32
restatement the GPU tests compare against, checked here against the fixture captured from the reference's own module
(tests/golden/perceptual.npz, make_golden_perceptual.py); the module surface (state_dict keys, both checkpoint layouts, the
refusal of trainable weights); argument errors of the new C ABI entry points."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

import make_golden_perceptual as P
from helpers import assert_close, golden

POOLS = (4, 9, 16)
SLICES = (range(0, 4), range(4, 9), range(9, 16), range(16, 23))


def ref_vgg(sd, x, slices=4, route=None):
    """Vgg16.forward (perceptual_loss.py:42-53) on stock ops in x's dtype: the outputs of the first `slices` slices.

    `route`: {conv index: a post-ReLU activation of that conv} from another evaluation (the GPU tests pass the HIP forward's own).
    The discrete decisions of the network are then taken from it -- each listed ReLU's mask from the signs of its activation, and
    each pool's window arg-max from the activation in front of it (pool1: relu1_2 = route[2]) -- while every value stays this
    evaluation's.  A pre-activation within rounding
    of 0, or a near-tie window, otherwise sends the gradient somewhere else between two evaluations orders (fp32 autograd of
    this network carries the same discrete noise as the generator's LeakyReLU kinks)."""
    route = route or {}
    outs, h = [], x
    for k in range(slices):
        for i in SLICES[k]:
            if i in POOLS:
                if i - 2 in route:  # the conv in front of the pool
                    _, idx = F.max_pool2d(route[i - 2].to(h), 2, 2, return_indices=True)
                    h = h.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
                else:
                    h = F.max_pool2d(h, 2, 2)
            elif f"slice{k + 1}.{i}.weight" in sd:
                pre = F.conv2d(h, sd[f"slice{k + 1}.{i}.weight"].to(x), sd[f"slice{k + 1}.{i}.bias"].to(x), padding=1)
                h = pre * (route[i].to(h) > 0).to(h) if i in route else F.relu(pre)
        outs.append(h)
    return outs


def ref_activations(sd, x, slices=2):
    """{conv index: post-ReLU activation} of every convolution in the first `slices` slices (a `route` for ref_vgg)."""
    acts, h = {}, x
    for k in range(slices):
        for i in SLICES[k]:
            if i in POOLS:
                h = F.max_pool2d(h, 2, 2)
            elif f"slice{k + 1}.{i}.weight" in sd:
                h = acts[i] = F.relu(F.conv2d(h, sd[f"slice{k + 1}.{i}.weight"].to(x), sd[f"slice{k + 1}.{i}.bias"].to(x), padding=1))
    return acts


def ref_preprocess(img, size):
    """avg_pool(upsample(img)) of perceptual_loss.py:16-17, literally."""
    return F.avg_pool2d(F.interpolate(img, scale_factor=7, mode="nearest"), size // 32)


def ref_preprocess_matrix(img, size):
    """The same map as A img A^T, A [224, size] the row weights of the 7x nearest up-sample followed by the size/32 average pool
    (exact: each output pixel averages a k x k block of the up-sampled image, k = size / 32).  Never materialises the 49x image."""
    k = size // 32
    a = torch.zeros(7 * size // k, size, dtype=img.dtype)
    for o in range(a.shape[0]):
        for p in range(o * k, o * k + k):
            a[o, p // 7] += 1.0 / k
    return torch.einsum("oh,bchw,pw->bcop", a, img, a)


def ref_loss(sd, img1, img2, size, route=None):
    """PerceptualLoss.forward (perceptual_loss.py:15-22): MSE of relu2_2 over every element; a batch-1 img2 is repeated."""
    if img2.shape[0] != img1.shape[0]:
        img2 = img2.expand(img1.shape[0], -1, -1, -1)
    b = img1.shape[0]
    pre = ref_preprocess_matrix if size > 256 else ref_preprocess
    f = ref_vgg(sd, torch.cat([pre(img1, size), pre(img2, size)]), 2, route)[1]
    return ((f[:b] - f[b:]) ** 2).mean()


def test_restatement_matches_the_reference_fixture():
    g = golden("perceptual")
    sd = P.vgg_state_dict()
    img1, target = P.loss_inputs()
    with torch.no_grad():  # the fp32 forward's ReLU masks and pool1 routing for the float64 run (3 relu1_1 signs differ here)
        acts = ref_activations(sd, ref_preprocess(torch.cat([img1, target.expand(P.LOSS_BATCH, -1, -1, -1)]), P.SIZE))
    for dtype, tol in ((torch.float32, 2e-5), (torch.float64, 1e-4)):
        x1 = img1.to(dtype).requires_grad_(True)
        loss = ref_loss(sd, x1, target.to(dtype), P.SIZE, route=acts if dtype == torch.float64 else None)
        (g1,) = torch.autograd.grad(loss, x1)
        assert abs(loss.item() - float(g["loss.value"])) <= tol * abs(float(g["loss.value"])), (dtype, loss.item())
        assert_close(g1.reshape(-1)[P.grad_positions(g1.numel())], g["loss.grad_at"], tol, f"d loss / d image1 ({dtype})")
        gs = g1.double()
        assert abs(gs.sum().item() - float(g["loss.grad_sum"])) <= tol * gs.abs().sum().item()
        assert abs(gs.pow(2).sum().item() - float(g["loss.grad_sumsq"])) <= tol * float(g["loss.grad_sumsq"])
        if dtype == torch.float64:  # the closed form restates the literal chain
            assert_close(ref_preprocess_matrix(x1.detach(), P.SIZE), ref_preprocess(x1.detach(), P.SIZE), 1e-12, "preprocess matrix form")
        x, r = P.vgg_inputs()
        xg = x.to(dtype).requires_grad_(True)
        outs = ref_vgg(sd, xg, route=ref_activations(sd, x) if dtype == torch.float64 else None)
        for name, o in zip(("relu1_2", "relu2_2", "relu3_3", "relu4_3"), outs):
            assert_close(o.detach(), g["vgg." + name], tol, f"{name} ({dtype})")
        (gx,) = torch.autograd.grad((outs[1] * r.to(dtype)).sum(), xg)
        assert_close(gx, g["vgg.grad"], tol, f"Vgg16 input gradient ({dtype})")


def test_state_dict_keys_are_the_references():
    from where2edit_amd.perceptual_loss import PerceptualLoss, Vgg16, normalize_batch
    g = golden("perceptual")
    loss = PerceptualLoss(types.SimpleNamespace(stylegan_size=256))
    assert sorted(loss.state_dict()) == [str(k) for k in g["keys"]] and len(g["keys"]) == 20
    assert isinstance(loss.model, Vgg16) and isinstance(loss.upsample, torch.nn.Upsample) and loss.upsample.scale_factor == 7
    assert isinstance(loss.avg_pool, torch.nn.AvgPool2d) and loss.avg_pool.kernel_size == 8
    assert not any(p.requires_grad for p in loss.parameters())
    x = torch.randn(2, 3, 4, 4)
    assert normalize_batch(x) is x  # the reference's ImageNet normalisation is commented out (perceptual_loss.py:58-65)
    # torchvision's published init when no weights are given: kaiming_normal_ (fan_out, relu), zero bias
    w = loss.model.slice2._modules["7"].weight
    assert torch.all(loss.model.slice2._modules["7"].bias == 0) and abs(w.std().item() - (2.0 / (128 * 9)) ** 0.5) < 0.05 * (2.0 / (128 * 9)) ** 0.5


def test_checkpoints_load_in_either_layout(tmp_path):
    from where2edit_amd.perceptual_loss import PerceptualLoss
    tv = P.vgg_features_state_dict()  # torchvision layout, conv5 block included
    tv["classifier.0.weight"] = torch.zeros(4096, 25088)[:8]
    tv["classifier.0.bias"] = torch.zeros(8)
    own = P.vgg_state_dict()
    for name, sd in (("tv", tv), ("own", own), ("prefixed", {"model." + k: v for k, v in own.items()})):
        path = tmp_path / f"{name}.pth"
        torch.save(sd, path)
        loss = PerceptualLoss(types.SimpleNamespace(stylegan_size=256, vgg_weights=str(path)))
        got = loss.model.state_dict()
        assert sorted(got) == sorted(own)
        assert all(torch.equal(got[k], own[k]) for k in own), name
    missing = dict(tv)
    del missing["features.19.bias"]
    torch.save(missing, tmp_path / "missing.pth")
    with pytest.raises(KeyError, match="slice4.19.bias"):
        PerceptualLoss(types.SimpleNamespace(stylegan_size=256, vgg_weights=str(tmp_path / "missing.pth")))
    bad = dict(tv)
    bad["features.5.weight"] = torch.zeros(128, 32, 3, 3)
    torch.save(bad, tmp_path / "bad.pth")
    with pytest.raises(RuntimeError, match="features.5.weight has shape"):
        PerceptualLoss(types.SimpleNamespace(stylegan_size=256, vgg_weights=str(tmp_path / "bad.pth")))


def test_trainable_weights_and_cpu_tensors_are_refused():
    from where2edit_amd.perceptual_loss import PerceptualLoss, Vgg16
    vgg = Vgg16(requires_grad=True)
    with pytest.raises(RuntimeError, match=r"requires_grad_\(False\)"):
        vgg(torch.zeros(1, 3, 32, 32))
    loss = PerceptualLoss(types.SimpleNamespace(stylegan_size=256), model=vgg)
    with pytest.raises(RuntimeError, match="Vgg16\\(requires_grad=False\\)"):
        loss(torch.zeros(1, 3, 256, 256), torch.zeros(1, 3, 256, 256))
    with pytest.raises(RuntimeError, match="GPU only"):  # no stock-op fallback: CPU tensors stop at _lib.ptr
        Vgg16()(torch.zeros(1, 3, 32, 32))


def test_trainer_refuses_two_identity_terms():
    from where2edit_amd.run_attention import RegionAttentionTrainer
    with pytest.raises(ValueError, match="not both"):
        RegionAttentionTrainer(None, None, None, identity_loss=object(), perceptual_loss=object(), device="cpu")


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("w2e_maxpool2x2_fwd", "w2e_maxpool2x2_relu_bwd", "w2e_mse_relu_fwd"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


def test_argument_errors_of_the_new_entry_points_need_no_gpu(lib):
    d = ctypes.c_void_p(64)  # never dereferenced: every check runs before a launch
    assert lib.w2e_maxpool2x2_fwd(None, d, 1, 4, 4, None) != 0 and b"null" in lib.w2e_last_error()
    assert lib.w2e_maxpool2x2_fwd(d, d, 1, 1, 8, None) != 0 and b"no 2x2 window" in lib.w2e_last_error()
    assert lib.w2e_maxpool2x2_fwd(d, d, 1, 8, 1, None) != 0
    assert lib.w2e_maxpool2x2_fwd(d, d, 0, 4, 4, None) == 0  # nothing to do
    assert lib.w2e_maxpool2x2_relu_bwd(d, None, d, 1, 4, 4, 1, None) != 0 and b"null" in lib.w2e_last_error()
    assert lib.w2e_maxpool2x2_relu_bwd(d, d, d, 1, 4, 1, 1, None) != 0 and b"no 2x2 window" in lib.w2e_last_error()
    assert lib.w2e_mse_relu_fwd(d, None, 2, 2, 16, None, None, d, 1024, d, None) != 0 and b"null" in lib.w2e_last_error()
    assert lib.w2e_mse_relu_fwd(d, d, 2, 2, 16, None, None, d, 1023, d, None) != 0 and b"partials slab holds 1023" in lib.w2e_last_error()
    assert lib.w2e_mse_relu_fwd(d, d, 3, 2, 16, None, None, d, 1024, d, None) != 0 and b"neither" in lib.w2e_last_error()
    assert lib.w2e_mse_relu_fwd(d, d, 2, 1, 16, d, d, d, 1024, d, None) != 0 and b"equal batches" in lib.w2e_last_error()
    assert lib.w2e_mse_relu_fwd(d, d, 0, 1, 16, None, None, d, 1024, d, None) != 0 and b"bad size" in lib.w2e_last_error()
