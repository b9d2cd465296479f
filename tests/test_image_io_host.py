"""Image I/O, host side (no GPU): the numpy restatement (tests/imageio_ref.py) against Pillow, against the recorded Pillow outputs of
tests/golden/image_io.npz and against the torch CPU op sequence of torchvision 0.8.2's make_grid / save_image; image_io's coefficient
tables against the restatement's; the C ABI of csrc/image.hip (declared, prototyped, exported, argument errors, the plan); and
image_io's refusal of CPU tensors."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import imageio_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("w2e_image_resize_plan", "w2e_image_resize", "w2e_image_quantize")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "image_io.npz"))


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


def _pil_resize(batch, out_h, out_w, filter):
    Image = pytest.importorskip("PIL.Image")
    resample = getattr(getattr(Image, "Resampling", Image), filter.upper())
    out = []
    for img in batch:
        pil = Image.fromarray(img[..., 0], "L") if img.shape[2] == 1 else Image.fromarray(img, "RGB")
        r = np.asarray(pil.resize((out_w, out_h), resample))
        out.append(r[..., None] if r.ndim == 2 else r)
    return np.stack(out)


@pytest.mark.parametrize("filter", ["bilinear", "nearest"])
@pytest.mark.parametrize("index", range(len(R.SHAPES)))
def test_ref_resize_equals_pillow(index, filter):
    """Every case of SHAPES, the 1024^2 and 512^2 ones included, seeded random bytes; the small cases also on the checkerboard and on
    all 255 (the patterns the GPU test adds)."""
    shape = R.SHAPES[index]
    small = shape in R.SMALL_SHAPES
    for name in (R.PATTERNS if small else ("random",)):
        x = R.pattern(name, shape, index)
        want = _pil_resize(x, shape[4], shape[5], filter)
        got = R.resize(x, shape[4], shape[5], filter)
        assert got.shape == want.shape and np.array_equal(got, want), (shape, name, int((got != want).sum()))


def test_ref_resize_equals_pillow_on_the_block_label():
    x = R.block_label(R.label_grid(), 32)[None, :, :, None]
    for filter in ("bilinear", "nearest"):
        assert np.array_equal(R.resize(x, 64, 64, filter), _pil_resize(x, 64, 64, filter))


def test_ref_resize_equals_the_recorded_pillow_outputs(golden):
    assert len(R.SMALL_SHAPES) == 8
    for i, shape in enumerate(R.SMALL_SHAPES):
        assert R.SHAPES.index(shape) == i  # (the fixture's seeds are the positions in SHAPES)
        x = R.pattern("random", shape, i)
        assert int(x.sum()) == int(golden[f"sum_{i}"]), "the seeded input is not the one the fixture was recorded from"
        for key, filter in (("bil", "bilinear"), ("nea", "nearest")):
            got = R.resize(x, shape[4], shape[5], filter)
            assert np.array_equal(got, golden[f"{key}_{i}"]), (shape, filter)
    assert np.array_equal(R.label_grid(), golden["label_grid"])
    label = R.block_label(golden["label_grid"], 32)[None, :, :, None]
    assert label.shape == (1, 512, 512, 1) and label.max() <= 18
    bil, nea = R.resize(label, 64, 64, "bilinear")[0, :, :, 0], R.resize(label, 64, 64, "nearest")[0, :, :, 0]
    assert np.array_equal(bil, golden["label_bil"]) and np.array_equal(nea, golden["label_nea"])
    # 512 / 64 = 8 divides the 32-pixel blocks: the bilinear window (16 taps) straddles a block border in one output column / row of
    # four, where ids blend; nearest keeps the ids
    assert np.array_equal(nea, R.block_label(golden["label_grid"], 4))
    assert 0.2 < float((bil != nea).mean()) < 0.6


def test_resample_tables_equal_the_ref_for_every_axis_of_shapes():
    from where2edit_amd.image_io import resample_tables
    pairs = sorted({(s[2], s[4]) for s in R.SHAPES} | {(s[3], s[5]) for s in R.SHAPES})
    for in_size, out_size in pairs:
        for filter in ("bilinear", "nearest"):
            k, b = resample_tables(in_size, out_size, filter)
            rk, rb = R.axis_tables(in_size, out_size, filter)
            assert k.dtype == torch.int32 and b.dtype == torch.int32 and not k.is_cuda
            assert tuple(k.shape) == rk.shape and tuple(b.shape) == (out_size, 2)
            assert np.array_equal(k.numpy(), rk) and np.array_equal(b.numpy(), rb), (in_size, out_size, filter)
            assert int(k.sum(1).max()) < 2 ** 23 and int((b[:, 0] + b[:, 1]).max()) <= in_size and int(b.min()) >= 0
    with pytest.raises(ValueError, match="bicubic"):
        resample_tables(8, 4, "bicubic")
    with pytest.raises(ValueError, match="1..16384"):
        resample_tables(0, 4)


def test_normalize_table_is_totensor_then_normalize():
    from where2edit_amd.image_io import normalize_table
    for mean, std in ((0.5, 0.5), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))):
        lut = normalize_table(mean, std, 3)
        v = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).repeat(1, 1, 3)  # an HWC "image" holding every byte
        t = v.permute(2, 0, 1).contiguous().to(torch.float32).div(255)             # ToTensor
        m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
        t = t.sub_(m.expand(3)[:, None, None]).div_(s.expand(3)[:, None, None])    # Normalize
        assert torch.equal(lut, t[:, 0, :])
        assert np.array_equal(lut.numpy(), R.normalize_table(mean, std, 3))


def _torch_save_image_bytes(x, lo, hi):
    """make_grid(normalize=True, range=(lo, hi)) norm_ip + save_image's conversion, as torchvision 0.8.2 writes them."""
    t = torch.from_numpy(x).clone()
    t.clamp_(min=lo, max=hi)
    t.add_(-lo).div_(hi - lo + 1e-5)
    return t.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()


@pytest.mark.parametrize("lo,hi", [(-1, 1), (0, 1)])
def test_ref_quantise_equals_the_torch_cpu_op_sequence_on_the_boundary_set(lo, hi):
    x = R.boundary_set(lo, hi)
    assert x.dtype == np.float32 and x.size == 256 * 7 + 7 + 100000
    finite = x[~np.isnan(x)]  # (a NaN -> uint8 conversion is undefined on the host; the specification says 0)
    got = R.quantise(finite, lo, hi)
    assert np.array_equal(got, _torch_save_image_bytes(finite, lo, hi))
    assert set(np.unique(got)) == set(range(256))
    assert R.quantise(np.array([np.nan], np.float32), lo, hi)[0] == 0


def test_ref_grid_layout_is_make_grid():
    """torchvision 0.8.2 utils.make_grid's layout, restated with torch ops on the normalised floats, then save_image's conversion."""
    rng = np.random.RandomState(3)
    for b, c, nrow, padding, pad_value in ((1, 3, 8, 2, 0.0), (2, 3, 8, 2, 0.0), (3, 3, 2, 2, 0.0), (3, 1, 2, 2, 0.0), (2, 3, 8, 2, 1.0), (5, 1, 3, 1, 0.25)):
        h, w = 6, 10
        x = rng.uniform(-1.2, 1.2, size=(b, c, h, w)).astype(np.float32)
        t = torch.from_numpy(x).clone()
        if c == 1:
            t = torch.cat((t, t, t), 1)
        t.clamp_(min=-1, max=1)
        t.add_(1).div_(1 - (-1) + 1e-5)
        if b == 1:
            grid = t.squeeze(0)
        else:
            xmaps = min(nrow, b)
            ymaps = int(math.ceil(float(b) / xmaps))
            height, width = h + padding, w + padding
            grid = t.new_full((3, height * ymaps + padding, width * xmaps + padding), pad_value)
            k = 0
            for y in range(ymaps):
                for xg in range(xmaps):
                    if k >= b:
                        break
                    grid.narrow(1, y * height + padding, height - padding).narrow(2, xg * width + padding, width - padding).copy_(t[k])
                    k += 1
        want = grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
        got = R.to_bytes(x, -1, 1, nrow=nrow, padding=padding, pad_value=pad_value)
        assert got.shape == want.shape and np.array_equal(got, want), (b, c, nrow)
    x = rng.uniform(-1, 1, size=(2, 1, 6, 10)).astype(np.float32)
    assert R.to_bytes(x, grid=False).shape == (2, 6, 10, 1)


def test_entry_points_are_declared_prototyped_and_exported(lib):
    from where2edit_amd import _lib
    header = open(os.path.join(ROOT, "include", "w2e_image.h")).read()
    want = {"*": ctypes.c_void_p, "float": ctypes.c_float, "int": ctypes.c_int}
    for name in SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M)
        assert m, f"{name} is not declared in include/w2e_image.h"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            assert a is want["*" if "*" in p else p.split()[0]], (name, p, a)
        assert hasattr(lib, name)
    assert _lib.header_version() == 7 and "w2e_image_quantize" in open(os.path.join(ROOT, "include", "w2e.h")).read()


def _plan(lib, *dims):
    plan = (ctypes.c_int64 * 8)()
    rc = lib.w2e_image_resize_plan(*dims, plan)
    return rc, list(plan)


def test_plan_picks_the_form_from_the_sizes(lib):
    rc, p = _plan(lib, 1, 3, 300, 200, 7, 11)
    assert rc == 0 and p[0] == 1 and p[1] == 1 * 300 * 11 * 3, p   # the two-launch form, its intermediate image as workspace
    assert p[2] == 2 * math.ceil(200 / 11) + 1 and p[3] == 2 * math.ceil(300 / 7) + 1
    for dims, ks in (((2, 3, 1024, 1024, 256, 256), 9), ((2, 1, 512, 512, 64, 64), 17)):
        rc, p = _plan(lib, *dims)
        assert rc == 0 and p[0] == 0 and p[1] == 0 and p[2] == p[3] == ks and 0 < p[6] <= 64 * 1024, (dims, p)
    for shape in R.SHAPES:  # every fused plan stays within 64 KB of LDS; a skipped axis has no table
        rc, p = _plan(lib, *shape)
        assert rc == 0 and p[6] <= 64 * 1024 and (p[0] == 0) == (p[6] > 0)
        assert (p[2] == 0) == (shape[3] == shape[5]) and (p[3] == 0) == (shape[2] == shape[4])
        assert p[2] == (R.axis_tables(shape[3], shape[5])[0].shape[1] if p[2] else 0)
    assert [s for s in R.SHAPES if _plan(lib, *s)[1][0] == 1] == [(1, 3, 300, 200, 7, 11)]
    rc, p = _plan(lib, 4, 3, 300, 200, 7, 200)  # one axis only: no workspace in either form
    assert rc == 0 and p[1] == 0


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    err = lib.w2e_last_error

    def resize(src=p, batch=1, channels=3, in_h=8, in_w=8, out_h=4, out_w=4, kx=p, bx=p, ksx=5, ky=p, by=p, ksy=5, lut=None, dst=p, work=None):
        return lib.w2e_image_resize(src, batch, channels, in_h, in_w, out_h, out_w, kx, bx, ksx, ky, by, ksy, lut, dst, work, None)

    assert resize(src=None) != 0 and b"null" in err()
    assert resize(dst=None) != 0 and b"null" in err()
    assert resize(kx=None) != 0 and b"horizontal" in err()
    assert resize(by=None) != 0 and b"vertical" in err()
    assert resize(channels=2) != 0 and b"channels" in err()
    assert resize(in_h=0) != 0 and b"1..16384" in err()
    assert resize(out_w=16385) != 0 and b"1..16384" in err()
    assert resize(batch=-1) != 0
    assert resize(ksx=6) != 0 and b"ksize_x" in err()
    assert resize(ksy=0) != 0 and b"ksize_y" in err()
    assert resize(in_h=300, in_w=200, out_h=7, out_w=11, ksx=1, ksy=1) != 0 and b"workspace" in err()  # form 1 without its workspace
    assert resize(batch=0) == 0                                                  # an empty batch: nothing to launch
    assert resize(batch=0, in_h=4, in_w=4, kx=None, bx=None, ky=None, by=None) == 0  # no axis passed: no tables needed

    plan = (ctypes.c_int64 * 8)()
    assert lib.w2e_image_resize_plan(1, 3, 8, 8, 4, 4, None) != 0 and b"null" in err()
    assert lib.w2e_image_resize_plan(1, 2, 8, 8, 4, 4, plan) != 0 and b"channels" in err()
    assert lib.w2e_image_resize_plan(1, 3, 0, 8, 4, 4, plan) != 0
    assert lib.w2e_image_resize_plan(1, 3, 8, 16385, 4, 4, plan) != 0 and b"1..16384" in err()
    assert lib.w2e_image_resize_plan(0, 1, 16384, 16384, 1, 1, plan) == 0 and plan[0] == 1

    def quant(src=p, batch=1, channels=3, h=4, w=4, lo=-1.0, hi=1.0, d=2.0, nrow=8, padding=2, pad=0.0, grid=1, dst=p):
        return lib.w2e_image_quantize(src, batch, channels, h, w, lo, hi, d, nrow, padding, pad, grid, dst, None)

    assert quant(src=None) != 0 and b"null" in err()
    assert quant(dst=None) != 0 and b"null" in err()
    assert quant(channels=2) != 0 and b"channels" in err()
    assert quant(h=0) != 0 and quant(w=16385) != 0
    assert quant(lo=float("nan")) != 0 and b"NaN" in err()
    assert quant(hi=float("nan")) != 0 and b"NaN" in err()
    assert quant(d=float("nan")) != 0 and b"NaN" in err()
    assert quant(lo=1.0, hi=1.0) != 0 and b"lo < hi" in err()
    assert quant(nrow=0) != 0 and b"nrow" in err()
    assert quant(padding=-1) != 0 and b"padding" in err()
    assert quant(dst=ctypes.c_void_p(66)) != 0 and b"aligned" in err()
    assert quant(batch=0) == 0


def test_cpu_tensors_wrong_dtypes_and_wrong_ranks_are_refused():
    import where2edit_amd as W
    from where2edit_amd import image_io as I
    assert W.to_tensor is I.to_tensor and W.to_bytes is I.to_bytes and W.resize_u8 is I.resize_u8 and W.label_ids is I.label_ids
    assert W.resample_tables is I.resample_tables
    u8, f32 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 3, 8, 8)
    gpu_msg = r"must be on the GPU.*\.to\('cuda'\)"
    with pytest.raises(RuntimeError, match=gpu_msg):
        I.resize_u8(u8, 4)
    with pytest.raises(RuntimeError, match=gpu_msg):
        I.to_tensor(u8, 4)
    with pytest.raises(RuntimeError, match=gpu_msg):
        I.label_ids(u8[..., 0], 4)
    with pytest.raises(RuntimeError, match=gpu_msg):
        I.to_bytes(f32)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        I.to_bytes(np.zeros((1, 3, 8, 8), np.float32))
    with pytest.raises(RuntimeError, match="must be torch.uint8"):
        I.to_tensor(f32, 4)
    with pytest.raises(RuntimeError, match="must be torch.uint8"):
        I.label_ids(torch.zeros(1, 8, 8, dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match="must be torch.float32"):
        I.to_bytes(u8)
    with pytest.raises(RuntimeError, match="4 dimensions"):
        I.to_tensor(u8[0], 4)
    with pytest.raises(RuntimeError, match="3 dimensions"):
        I.label_ids(u8, 4)
    with pytest.raises(RuntimeError, match="3 or 4 dimensions"):
        I.resize_u8(u8[0, 0], 4)
    with pytest.raises(RuntimeError, match="4 dimensions"):
        I.to_bytes(f32[0])


def test_grid_shape_is_the_refs_canvas():
    from where2edit_amd.image_io import grid_shape
    for b, nrow, padding in ((1, 8, 2), (2, 8, 2), (3, 2, 2), (9, 8, 0), (5, 3, 1)):
        x = np.zeros((b, 3, 6, 10), np.float32)
        assert grid_shape(b, 6, 10, nrow, padding) == R.to_bytes(x, nrow=nrow, padding=padding).shape[:2]
