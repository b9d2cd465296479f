"""The PNG decoder on the GPU (where2edit_amd/image_io.py, csrc/png.hip, csrc/png_core.h): exact equality everywhere.  PNG is
lossless, so the expected pixels of a file that tests/png_ref.py's writer made are the array the writer was given; the expected bytes
of a zlib stream are zlib.decompress's; the recorded Pillow files (tests/golden/png.npz) come with Pillow's own pixels.  The streams are
the case list of tests/png_ref.py, of which tests/test_png_host.py asserts from a census that they show what an inflate can get wrong.

Shapes: images are tens of pixels on a side; heights straddle the band of stage 2 (W2E_PNG_BAND rows per wave: band - 1, band, band + 1,
2 band + 2), widths 1, 2 and 67 (more than the 64 steps that the last lane of a band lags behind the first), sub-byte palettes at widths
that end inside a byte (1, 5, 9)."""
import functools
import os
import zlib

import numpy as np
import pytest
import torch

import png_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = P.BAND
COLOURS = ((0, 8), (2, 8), (4, 8), (6, 8), (3, 8), (3, 4), (3, 2), (3, 1))


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "png.npz"))
    blob, offsets = g["blob"].tobytes(), g["offsets"]
    return {str(k): (blob[offsets[i]:offsets[i + 1]], g["rgb_" + str(k)], g["raw_" + str(k)]) for i, k in enumerate(g["keys"])}


def _image(seed, h, w, colour, depth):
    """(pixels as the writer takes them, palette or None): noise, so that every filter and every byte value occurs."""
    rng = np.random.default_rng(seed)
    if colour == 3:
        n = 1 << depth
        return rng.integers(0, n, (h, w), dtype=np.uint8), rng.integers(0, 256, (min(n, 200), 3), dtype=np.uint8)
    c = P.CHANNELS[colour]
    return rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8), None


def _expected(pixels, palette, colour, depth, mode):
    return P.colour_step(P.pack_rows(pixels, colour, depth), pixels.shape[1], colour, depth, palette, mode)


def _eq(t, a):
    assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == a.shape, (t.dtype, tuple(t.shape), a.shape)
    return np.array_equal(t.cpu().numpy(), a)


# ---- stage 1 ----
@pytest.mark.parametrize("name", list(P.valid_cases()))
def test_png_inflate_equals_zlib(name):
    from where2edit_amd import png_inflate
    z, data = P.valid_cases()[name]
    assert zlib.decompress(z) == data
    out = png_inflate(z, len(data), device=DEV)
    assert out.cpu().numpy().tobytes() == data


def test_png_inflate_of_a_batch_of_different_lengths():
    from where2edit_amd import png_inflate
    cases = P.valid_cases()
    out = png_inflate([z for z, _ in cases.values()], [len(d) for _, d in cases.values()], device=DEV)
    assert len({len(z) for z, _ in cases.values()}) > 8
    for (name, (_, data)), t in zip(cases.items(), out):
        assert t.cpu().numpy().tobytes() == data, name


# ---- stage 2 ----
def _pixels_case(h, w, colour, depth, filters, seed=0):
    from where2edit_amd import png_pixels
    pixels, palette = _image(seed, h, w, colour, depth)
    rows = P.pack_rows(pixels, colour, depth)
    bpp = P.filter_bpp(colour, depth)
    data = P.filter_rows(rows, bpp, filters)
    assert np.array_equal(P.unfilter(data, h, rows.shape[1], bpp), rows)  # the restatement undoes the test's own filtering
    raw = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    before = raw.clone()
    for mode in ("RGB", "raw"):
        out = png_pixels(raw, h, w, colour, depth, palette=None if palette is None else torch.from_numpy(palette), mode=mode)
        assert _eq(out, _expected(pixels, palette, colour, depth, mode)), (h, w, colour, depth, filters, mode)
    assert torch.equal(raw, before)


@pytest.mark.parametrize("filt", [0, 1, 2, 3, 4])
def test_png_pixels_every_filter_on_the_first_row_and_on_later_rows(filt):
    for colour, depth in ((0, 8), (4, 8), (2, 8), (6, 8)):  # bpp 1, 2, 3, 4
        _pixels_case(9, 13, colour, depth, filt, seed=filt)


def test_png_pixels_a_mix_of_filters_per_row():
    rng = np.random.default_rng(11)
    for colour, depth in ((0, 8), (4, 8), (2, 8), (6, 8), (3, 4)):
        _pixels_case(23, 19, colour, depth, rng.integers(0, 5, 23).tolist(), seed=colour)


@pytest.mark.parametrize("h", [1, BAND - 1, BAND, BAND + 1, 2 * BAND + 2])
def test_png_pixels_heights_around_the_band(h):
    rng = np.random.default_rng(h)
    for w in (1, 2, 67):
        _pixels_case(h, w, 2, 8, rng.integers(0, 5, h).tolist(), seed=h + w)
    _pixels_case(h, 67, 0, 8, rng.integers(1, 5, h).tolist(), seed=h)


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_png_pixels_sub_byte_palettes(depth):
    rng = np.random.default_rng(depth)
    for w in (1, 5, 9):
        _pixels_case(BAND + 3, w, 3, depth, rng.integers(0, 5, BAND + 3).tolist(), seed=w)


# ---- end to end ----
@pytest.mark.parametrize("colour,depth", COLOURS)
def test_from_png_equals_the_writers_input(colour, depth):
    from where2edit_amd import from_png
    h, w = 70, 37
    pixels, palette = _image(colour * 10 + depth, h, w, colour, depth)
    rng = np.random.default_rng(5)
    data = P.write_png(pixels, colour, depth, palette=palette, filters=rng.integers(0, 5, h).tolist(), idat=97, level=6)
    for mode in ("RGB", "raw"):
        assert _eq(from_png(data, mode=mode, device=DEV), _expected(pixels, palette, colour, depth, mode)), mode


@pytest.mark.parametrize("key", list(_golden()))
def test_from_png_equals_pillows_pixels(key):
    from where2edit_amd import from_png
    data, rgb, raw = _golden()[key]
    assert _eq(from_png(data, device=DEV), rgb)
    assert _eq(from_png(data, mode="raw", device=DEV), raw)


def test_from_png_of_a_mixed_list_and_stacked():
    from where2edit_amd import from_png
    golden = _golden()
    files = [golden[k][0] for k in ("RGB", "L", "RGBA", "P4", "RGB_level1", "L_level9", "P8")]
    want = [golden[k][1] for k in ("RGB", "L", "RGBA", "P4", "RGB_level1", "L_level9", "P8")]
    out = from_png(files, device=DEV)
    assert len(out) == len(files) and all(_eq(t, a) for t, a in zip(out, want))
    stacked = from_png(files, device=DEV, stack=True)  # one size, one mode: [B, H, W, 3]
    assert _eq(stacked, np.stack(want))
    labels = from_png([golden["L"][0], golden["P8"][0], golden["L_level9"][0]], mode="raw", device=DEV, stack=True)
    assert _eq(labels, np.stack([golden[k][2] for k in ("L", "P8", "L_level9")]))
    with pytest.raises(ValueError, match="stack=True"):
        from_png([golden["L"][0], golden["RGB"][0]], mode="raw", device=DEV, stack=True)
    assert from_png([], device=DEV) == []


def test_read_image_and_load_png(tmp_path):
    from where2edit_amd import from_jpeg, load_png, read_image
    data, rgb, raw = _golden()["P_trns"]
    path = tmp_path / "portrait.png"
    path.write_bytes(data)
    assert _eq(read_image(path, device=DEV), rgb)
    assert _eq(load_png(str(path), device=DEV), rgb) and _eq(load_png(path, mode="raw", device=DEV), raw)
    with open(path, "rb") as f:
        assert _eq(load_png(f, device=DEV), rgb)
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"))
    jpeg = g["pil_blob"].tobytes()[g["pil_offsets"][0]:g["pil_offsets"][1]]
    jpath = tmp_path / "photo.jpg"
    jpath.write_bytes(jpeg)
    assert torch.equal(read_image(jpath, device=DEV), from_jpeg(jpeg, device=DEV))


def test_celebamask_samples(tmp_path):
    from where2edit_amd import celebamask_samples, label_ids
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"))
    blob, offsets = g["pil_blob"].tobytes(), g["pil_offsets"]
    jpeg = blob[offsets[0]:offsets[1]]
    (tmp_path / "img").mkdir(), (tmp_path / "label").mkdir()
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 19, (3, 6, 5), dtype=np.uint8).repeat(8, 1).repeat(8, 2)  # 48 x 40 labels of 8 x 8 regions
    for i in range(3):
        (tmp_path / "img" / f"{i}.jpg").write_bytes(jpeg)
        (tmp_path / "label" / f"{i}.png").write_bytes(P.write_png(ids[i], 0, filters=[0, 1, 2, 3, 4][i], level=9))
    batches = list(celebamask_samples(tmp_path / "img", tmp_path / "label", batch=2, device=DEV))
    assert [tuple(x.shape[:1]) for x, _ in batches] == [(2,), (1,)]
    for first, (x, label) in zip((0, 2), batches):
        assert x.dtype == torch.uint8 and x.ndim == 4 and x.shape[3] == 3 and x.is_cuda
        assert _eq(label, ids[first:first + label.shape[0]])
        want = label_ids(torch.from_numpy(ids[first:first + label.shape[0]]).to(DEV), 16, "bilinear")
        assert torch.equal(label_ids(label, 16, "bilinear"), want)


def test_the_same_call_gives_the_same_tensors():
    from where2edit_amd import from_png
    golden = _golden()
    files = [golden[k][0] for k in golden]
    a, b = from_png(files, device=DEV), from_png(files, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c, d = from_png(files, mode="raw", device=DEV), from_png(files, mode="raw", device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(c, d))


# ---- corrupt streams: the status word (tests/test_png_host.py runs the same list through the same decoder core on the host first, under
# the sanitizers; this list is here to show that the status reaches the caller, not to look for a fault) ----
def test_a_corrupt_stream_is_an_error_that_names_its_status():
    from where2edit_amd import from_png, png_inflate
    z_ok, data_ok = P.valid_cases()["dynamic_many"]
    for name, z, size, status in P.corrupt_cases():
        with pytest.raises(ValueError, match="corrupt stream") as e:
            png_inflate(z, size, device=DEV)
        if status is not None:
            assert f"(status {P.STATUS[status]})" in str(e.value), (name, str(e.value))
        assert png_inflate(z_ok, len(data_ok), device=DEV).cpu().numpy().tobytes() == data_ok, name  # the next decode is still right
    z, h, w = P.corrupt_filter()
    with pytest.raises(ValueError, match=f"status {P.STATUS['FILTER']}"):
        from_png(P.wrap_idat(z, h, w), device=DEV)
    # inside a batch: the error names the image, the others are none the worse
    pixels, _ = _image(1, 12, 9, 0, 8)
    good = P.write_png(pixels, 0, filters=4)
    bad = P.wrap_idat(P.corrupt_cases()[0][1][:40] , 12, 9)
    with pytest.raises(ValueError, match="image 1 has a corrupt stream"):
        from_png([good, bad, good], device=DEV)
    assert _eq(from_png(good, mode="raw", device=DEV), pixels)
