"""The PNG encoder on the GPU (where2edit_amd/image_io.py, csrc/png_encode.hip, csrc/png_deflate_core.h): exact equality everywhere.
The filtered rows are Pillow's (tests/png_encode_ref.py: filter_rows, which tests/test_png_encode_host.py holds to Pillow); the zlib
streams are the ones the core makes on the host with one lane, recorded in tests/golden/png_encode.npz -- so the kernel's 64 lanes, its
LDS ordering and its atomics must give the one-lane bytes -- and every stream inflates with zlib to its input.

Shapes (tests/png_encode_ref.py: gpu_images, corpus): one row, one column, rows that are no multiple of 4 bytes, all four channel
counts, filtered sizes of exactly 32767, 32768 and 32769 bytes (the chunk is 32768), two and three chunks; buffers of 0 bytes, 1 byte
and 2 * 32768 + 1."""
import functools
import hashlib
import io
import os
import zlib

import numpy as np
import pytest
import torch

import png_encode_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "png_encode.npz"))
    blob, offsets = g["blob"].tobytes(), g["offsets"]
    return {str(n): (int(g["lengths"][i]), str(g["sha256"][i]), blob[offsets[i]:offsets[i + 1]]) for i, n in enumerate(g["names"])}


@functools.lru_cache(maxsize=None)
def _inputs():
    return E.recorded_inputs()


@functools.lru_cache(maxsize=None)
def _images():
    return E.gpu_images()


@functools.lru_cache(maxsize=None)
def _files():
    """to_png of every image of the test, each on its own: computed once."""
    from where2edit_amd import image_io as I
    return {name: I.to_png(torch.from_numpy(a).to(DEV)) for name, a in _images().items()}


def _is_recorded(name, z):
    length, sha, whole = _golden()[name]
    assert (len(z), hashlib.sha256(z).hexdigest()) == (length, sha), name
    assert not whole or whole == z, name


def test_png_deflate_equals_the_one_lane_recording():
    from where2edit_amd import image_io as I
    inputs = _inputs()
    assert list(inputs) == list(_golden())
    streams = I.png_deflate(list(inputs.values()))  # ONE batch: buffers of 0 to 262656 bytes, one to nine chunks
    assert len(streams) == len(inputs)
    for (name, data), z in zip(inputs.items(), streams):
        assert isinstance(z, bytes) and zlib.decompress(z) == data, name
        assert len(z) <= E.stored_bound(len(data)), name
        _is_recorded(name, z)


def test_png_deflate_takes_tensors_and_is_the_same_alone_and_twice():
    from where2edit_amd import image_io as I
    inputs = _inputs()
    for name in ("empty", "one_byte", "zeros_65537", "photo_32769", "noise_40000"):
        t = torch.frombuffer(bytearray(inputs[name]), dtype=torch.uint8).to(DEV) if inputs[name] else torch.empty(0, dtype=torch.uint8, device=DEV)
        (z,), (again,) = I.png_deflate([t]), I.png_deflate([t])
        assert z == again, name
        _is_recorded(name, z)
    assert I.png_deflate([]) == []


@pytest.mark.parametrize("channels", (1, 2, 3, 4))
def test_png_filter_equals_the_reference_and_pillow(channels):
    from where2edit_amd import image_io as I
    cases = {n: a for n, a in list(E.filter_cases().items()) + list(_images().items()) if a.shape[2] == channels}
    assert any(a.shape[0] == 1 for a in cases.values()) and any(a.shape[1] == 1 for a in cases.values())
    assert any((a.shape[1] * channels + 1) % 4 for a in cases.values())
    pillow = None
    try:
        import PIL  # noqa: F401
        pillow = E.pillow_rows
    except ImportError:
        pass
    for name, a in cases.items():
        rows = I.png_filter(torch.from_numpy(a).to(DEV))
        assert rows.dtype == torch.uint8 and rows.is_cuda and tuple(rows.shape) == (a.shape[0] * (1 + a.shape[1] * channels),), name
        got = rows.cpu().numpy().tobytes()
        assert got == E.filter_rows(a), name
        assert pillow is None or got == pillow(a), name
    # a batch is its images one by one; a non-contiguous input is taken as its values
    same = [a for n, a in cases.items() if n.endswith(f"_13x16x{channels}")]
    batch = I.png_filter(torch.from_numpy(np.stack(same)).to(DEV))
    assert tuple(batch.shape) == (len(same), 13 * (1 + 16 * channels))
    for i, a in enumerate(same):
        assert batch[i].cpu().numpy().tobytes() == E.filter_rows(a)
    t = torch.from_numpy(np.stack(same)).to(DEV).transpose(1, 2)
    assert I.png_filter(t)[0].cpu().numpy().tobytes() == E.filter_rows(same[0].transpose(1, 0, 2))


def test_to_png_round_trips_and_holds_pillows_rows():
    from where2edit_amd import image_io as I
    for name, a in _images().items():
        f = _files()[name]
        assert isinstance(f, bytes), name
        payload, chunks = E.idat_payload(f)  # (the CRCs are checked)
        assert chunks == ["IHDR", "IDAT", "IEND"], name
        assert zlib.decompress(payload) == E.filter_rows(a), name
        _is_recorded("rows_" + name, payload)
        assert f == E.png_file(a, payload), name
        back = I.from_png(f, mode="raw")
        assert np.array_equal(back.cpu().numpy().reshape(a.shape), a), name
    Image = pytest.importorskip("PIL.Image")
    for name, a in _images().items():
        image = Image.open(io.BytesIO(_files()[name]))
        assert image.mode == E.MODE_OF_CHANNELS[a.shape[2]] and image.size == (a.shape[1], a.shape[0]), name
        assert np.array_equal(np.asarray(image).reshape(a.shape), a), name
        assert zlib.decompress(E.idat_payload(_files()[name])[0]) == E.pillow_rows(a), name


def test_batch_equals_single_calls_and_two_runs_agree():
    from where2edit_amd import image_io as I
    h, w = 97, 113  # 97 * 340 = 32980 bytes: two chunks, the second short
    images = [E.photo_like(h, w, name="b0"), E.graphic(h, w, name="b1"), E.noise(h, w, name="b2")]
    batch = torch.from_numpy(np.stack(images)).to(DEV)
    files = I.to_png(batch)
    assert isinstance(files, list) and len(files) == 3 and all(isinstance(f, bytes) for f in files)
    for i, a in enumerate(images):
        single = I.to_png(batch[i])
        assert isinstance(single, bytes) and single == files[i], i
        assert zlib.decompress(E.idat_payload(single)[0]) == E.filter_rows(a), i
    assert I.to_png(batch) == files
    assert len(E.idat_payload(files[2])[0]) > 32980 * 5 // 8 + 1024  # the noise took the second copy
    assert I.to_png(batch[:0]) == []
    one = I.to_png(batch[:1])
    assert isinstance(one, list) and one == files[:1]


def test_argument_errors_come_before_any_launch():
    from where2edit_amd import image_io as I
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    for fn in (I.to_png, I.png_filter):
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            fn(u8.cpu())
        with pytest.raises(RuntimeError, match="must be torch.uint8"):
            fn(u8.float())
        with pytest.raises(RuntimeError, match="3 or 4 dimensions"):
            fn(u8[0, 0])
        with pytest.raises(RuntimeError, match="C = 1"):
            fn(torch.zeros((8, 8, 5), dtype=torch.uint8, device=DEV))
        with pytest.raises(RuntimeError, match="C = 1"):
            fn(torch.zeros((8, 8, 0), dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="16384"):
            fn(torch.zeros((1, 16385, 1), dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("nrow", (1, 2))
def test_save_png_is_to_bytes_canvas(nrow, tmp_path):
    from where2edit_amd import image_io as I
    x = torch.from_numpy(np.random.RandomState(5).randn(3, 3, 21, 17).astype(np.float32)).to(DEV)
    canvas = I.to_bytes(x, nrow=nrow, padding=3, pad_value=0.25, grid=True).cpu().numpy()
    buf = io.BytesIO()
    I.save_png(x, buf, nrow=nrow, padding=3, pad_value=0.25)
    path = tmp_path / "grid.png"
    I.save_png(x, path, nrow=nrow, padding=3, pad_value=0.25)
    assert path.read_bytes() == buf.getvalue()
    assert np.array_equal(I.from_png(buf.getvalue(), mode="raw").cpu().numpy(), canvas)
    assert np.array_equal(I.load_png(str(path)).cpu().numpy(), canvas)
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(np.asarray(Image.open(path)), canvas)
    grey = I.to_bytes(x[:, :1], nrow=nrow, padding=3, grid=True).cpu().numpy()  # a 1-channel batch is replicated to RGB, as torchvision does
    buf = io.BytesIO()
    I.save_png(x[:, :1], buf, nrow=nrow, padding=3)
    assert np.array_equal(np.asarray(Image.open(buf)), grey)
