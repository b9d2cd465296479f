"""The JPEG encoder on the GPU (where2edit_amd/image_io.py, csrc/jpeg.hip) against the numpy restatement of tests/jpeg_ref.py, which
tests/test_jpeg_host.py holds against Pillow, and against Pillow's recorded files (tests/golden/jpeg_pillow.npz): exact equality
everywhere, coefficients and bytes.

Sizes (H x W) and what each breaks:
    1 x 1               a single block
    8 x 8               one real Y block, three dummies, even H under 16
    16 x 16             exactly one MCU
    17 x 23             odd and odd, dummies on both edges
    70 x 38             even H not a multiple of 16 (chroma rows repeat the last DOWN-SAMPLED row)
    33 x 16             odd H (one full-resolution row is repeated before the down-sampling)
    40 x 10, 10 x 40    a chroma block narrower than its Y
    130 x 262           several strips of 8 MCUs per MCU row, a ragged last one
    2054 x 30           the grid canvas of two 1024-row images, at a width that keeps it cheap
    3 x (40 x 56)       batching
    264 x 520           3366 blocks: past three 1024-block tiles of the prefix sum
    48 x 40             the other qualities (1, 30, 95, 100)
Contents: jpeg_ref.PATTERNS (random, ramp, constant, the two checkerboards -- also at quality 100 --, mixed)."""
import functools
import hashlib
import io
import os

import numpy as np
import pytest
import torch

import jpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.cases()


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pillow.npz"))
    keys = [str(k) for k in g["keys"]]
    recorded = [str(k) for k in g["recorded"]]
    blob, offsets = g["blob"].tobytes(), g["offsets"]
    return {"sha256": dict(zip(keys, (str(s) for s in g["sha256"]))), "files": {k: blob[offsets[i]:offsets[i + 1]] for i, k in enumerate(recorded)}}


@functools.lru_cache(maxsize=None)
def _input(case):
    h, w, name, quality, seed = case
    x = R.pattern(name, h, w, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref_coefficients(case):
    c = R.coefficients(_input(case), case[3])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _ref_file(case):
    """The restatement's file of a case: computed once, shared by the tests below."""
    return R.header(case[0], case[1], case[3]) + R.segment(_ref_coefficients(case)).replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def _gpu(x):
    return torch.from_numpy(np.array(x)).to(DEV)  # (a copy: the cached inputs are read-only)


def _first_difference(a, b):
    n = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), min(len(a), len(b)))
    return f"{len(a)} bytes against {len(b)}, first difference at byte {n}"


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_jpeg_coefficients_equal_the_reference(size):
    from where2edit_amd.image_io import jpeg_coefficients, jpeg_plan
    for case in CASES:
        if case[:2] != size:
            continue
        want = _ref_coefficients(case)
        got = jpeg_coefficients(_gpu(_input(case)), case[3])
        assert got.dtype == torch.int16 and tuple(got.shape) == want.shape == (jpeg_plan(1, *size)["blocks"], 64) and got.is_contiguous()
        bad = np.argwhere(got.cpu().numpy() != want)
        assert len(bad) == 0, f"{case}: {len(bad)} coefficients differ, the first at (block, k) = {tuple(bad[0])}"


def test_jpeg_coefficients_of_a_batch_and_of_an_odd_address():
    from where2edit_amd.image_io import jpeg_coefficients
    b, h, w = R.BATCH_SIZE
    names = ("random", "mixed", "ramp")
    x = np.stack([R.pattern(n, h, w, 20 + i) for i, n in enumerate(names)])
    got = jpeg_coefficients(_gpu(x)).cpu().numpy()
    assert got.shape == (b, R.geometry(h, w)[2], 64)
    for i in range(b):
        assert np.array_equal(got[i], R.coefficients(x[i])), names[i]
    # rows that start at every residue modulo 16, the first byte of the buffer not the image's: the ragged chunks of the staging
    case = (17, 23, "random", 75, R.ALL_SIZES.index((17, 23)))
    flat = torch.zeros(17 * 23 * 3 + 5, dtype=torch.uint8, device=DEV)
    for shift in (1, 5):
        view = flat[shift:shift + 17 * 23 * 3].view(17, 23, 3)
        view.copy_(_gpu(_input(case)))
        assert view.data_ptr() % 4 == shift % 4 and view.is_contiguous()
        assert np.array_equal(jpeg_coefficients(view).cpu().numpy(), _ref_coefficients(case))


@pytest.mark.parametrize("size", [s for s in R.ALL_SIZES if s != R.SCAN_SIZE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_to_jpeg_equals_the_reference_and_the_recorded_pillow_files(size, golden):
    from where2edit_amd.image_io import to_jpeg
    for case in CASES:
        if case[:2] != size:
            continue
        got = to_jpeg(_gpu(_input(case)), case[3])
        assert isinstance(got, bytes)
        want = _ref_file(case)
        assert got == want, f"{case}: {_first_difference(got, want)}"
        key = R.case_key(*case)
        assert hashlib.sha256(got).hexdigest() == golden["sha256"][key], case
        if size[0] * size[1] <= R.RECORDED_PIXELS:
            assert got == golden["files"][key], case


def test_to_jpeg_past_the_scan_tile(golden):
    """264 x 520 is 17 x 33 MCUs = 3366 blocks; the prefix sum walks an image in tiles of 1024 blocks (W2E_JPEG_SCAN_TILE), so this is
    three whole tiles and 294 blocks of a fourth: the carry crosses a tile border three times."""
    from where2edit_amd.image_io import jpeg_plan, to_jpeg
    plan = jpeg_plan(1, *R.SCAN_SIZE)
    assert plan["blocks"] == 3366 and plan["scan_tile"] == 1024 and plan["blocks"] > 3 * plan["scan_tile"]
    for case in CASES:
        if case[:2] != R.SCAN_SIZE:
            continue
        got, want = to_jpeg(_gpu(_input(case)), case[3]), _ref_file(case)
        assert got == want, f"{case}: {_first_difference(got, want)}"
        assert hashlib.sha256(got).hexdigest() == golden["sha256"][R.case_key(*case)], case


def test_to_jpeg_of_a_batch_and_the_second_copy():
    from where2edit_amd import image_io as I
    b, h, w = R.BATCH_SIZE
    names = ("random", "constant", "mixed")
    x = np.stack([R.pattern(n, h, w, 20 + i) for i, n in enumerate(names)])
    got = I.to_jpeg(_gpu(x))
    assert isinstance(got, list) and len(got) == b
    for i in range(b):
        assert got[i] == R.encode(x[i]), names[i]
    assert I.to_jpeg(_gpu(x[:0])) == []
    # noise at quality 100 codes to more than the 4 bits per pixel the first copy takes: the rest comes in a second one
    h, w = 130, 262
    x = R.pattern("random", h, w, 31)
    want = R.encode(x, 100)
    assert len(want) - 623 > h * w // I._JPEG_GUESS_DIVISOR + 1024
    assert I.to_jpeg(_gpu(x), 100) == want


def test_the_same_call_gives_the_same_bytes():
    from where2edit_amd import _lib
    from where2edit_amd.image_io import to_jpeg
    x = _gpu(np.stack([R.pattern("mixed", 130, 262, 40), R.pattern("random", 130, 262, 41)]))
    first = to_jpeg(x)
    assert to_jpeg(x) == first
    before = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        assert to_jpeg(x) == first and to_jpeg(x) == first
    finally:
        _lib.set_option("deterministic", before)


def test_save_image_end_to_end(tmp_path):
    from where2edit_amd.image_io import save_image, to_bytes
    rng = np.random.RandomState(50)
    for b, nrow in ((1, 8), (3, 2)):
        yy, xx = np.meshgrid(np.linspace(-1.2, 1.2, 24), np.linspace(-1, 1, 40), indexing="ij")
        x = np.stack([np.stack([yy * (i + 1) / b, xx, yy * xx]) for i in range(b)]) + rng.normal(0, 0.05, size=(b, 3, 24, 40))
        x = torch.from_numpy(x.astype(np.float32)).to(DEV)
        canvas = to_bytes(x, nrow=nrow).cpu().numpy()
        assert canvas.shape == ((24, 40, 3) if b == 1 else (2 * 26 + 2, 2 * 42 + 2, 3))
        want = R.encode(canvas)
        path = tmp_path / f"batch{b}.jpg"
        save_image(x, str(path), nrow=nrow)
        assert path.read_bytes() == want
        buf = io.BytesIO()
        save_image(x, buf, nrow=nrow)
        assert buf.getvalue() == want
    save_image(x, tmp_path / "q.JPEG", nrow=2, quality=30)
    assert (tmp_path / "q.JPEG").read_bytes() == R.encode(canvas, 30)


def test_the_reference_size():
    """One 1024 x 1024 smooth-plus-noise image: against Pillow where it imports, and against the restatement (whose entropy coder
    lays all tokens down with one cumulative sum: about a second at this size)."""
    from where2edit_amd.image_io import to_jpeg
    x = R.photo(1024, 1024)
    got = to_jpeg(_gpu(x))
    want = R.encode(x)
    assert got == want, _first_difference(got, want)
    try:
        from PIL import Image
    except ImportError:
        return
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, format="JPEG")
    assert got == buf.getvalue()
