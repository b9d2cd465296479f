"""JPEG encoding, host side (no GPU): the numpy restatement (tests/jpeg_ref.py) against Pillow and against the recorded Pillow files of
tests/golden/jpeg_pillow.npz; image_io's header and quantisation tables against Pillow's file; the C ABI of csrc/jpeg.hip (declared,
prototyped, exported, the plan's numbers, argument errors); and image_io's refusal of what it does not take."""
import ctypes
import functools
import hashlib
import io
import os
import re

import numpy as np
import pytest
import torch

import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("w2e_jpeg_plan", "w2e_jpeg_coefficients", "w2e_jpeg_entropy")
CASES = R.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_pillow.npz"))


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


@functools.lru_cache(maxsize=None)
def _encoded(case):
    """The restatement's file for a case: computed once, shared by the tests below."""
    h, w, name, quality, seed = case
    return R.encode(R.pattern(name, h, w, seed), quality)


def _pillow(x, quality=None):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, format="JPEG", **({} if quality is None else {"quality": quality}))
    return buf.getvalue()


def test_the_case_list_covers_what_the_kernels_can_get_wrong():
    sizes = {c[:2] for c in CASES}
    assert sizes == set(R.ALL_SIZES) and len(R.ALL_SIZES) == 13
    assert {c[2] for c in CASES} == set(R.PATTERNS)
    assert {c[3] for c in CASES if c[:2] == R.QUALITY_SIZE} == {1, 30, 75, 95, 100}
    assert all((h, w, n, 100, s) in CASES for h, w, n, q, s in CASES if n in ("checker", "colour_checker"))
    assert len({R.case_key(*c) for c in CASES}) == len(CASES)
    assert R.geometry(*R.SCAN_SIZE) == (33, 17, 3366)


@pytest.mark.parametrize("size", R.ALL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ref_encode_equals_pillow(size):
    """Every content at quality 75 (named, and as the default the reference's save_image takes), the checkerboards at 100, and the
    other qualities on QUALITY_SIZE."""
    for case in CASES:
        if case[:2] != size:
            continue
        h, w, name, quality, seed = case
        x = R.pattern(name, h, w, seed)
        want = _pillow(x, quality)
        assert _encoded(case) == want, case
        if quality == 75:
            assert want == _pillow(x), "Pillow's default is no longer quality 75"


def test_ref_encode_equals_the_recorded_pillow_files(golden):
    keys = [str(k) for k in golden["keys"]]
    assert keys == [R.case_key(*c) for c in CASES], "the fixture was recorded from another case list: run tests/golden/make_golden_jpeg.py"
    recorded = [str(k) for k in golden["recorded"]]
    assert recorded == [R.case_key(*c) for c in CASES if c[0] * c[1] <= R.RECORDED_PIXELS] and len(recorded) >= 60
    blob, offsets = golden["blob"].tobytes(), golden["offsets"]
    files = {k: blob[offsets[i]:offsets[i + 1]] for i, k in enumerate(recorded)}
    for i, case in enumerate(CASES):
        h, w, name, quality, seed = case
        assert int(R.pattern(name, h, w, seed).sum()) == int(golden["sum"][i]), "the seeded input is not the one the fixture was recorded from"
        got = _encoded(case)
        assert hashlib.sha256(got).hexdigest() == str(golden["sha256"][i]), case
        if keys[i] in files:
            assert got == files[keys[i]], case


def test_the_stages_of_the_ref_hang_together():
    x = R.pattern("mixed", 17, 23, 3)
    coef = R.coefficients(x)
    mx, my, blocks = R.geometry(17, 23)
    assert (mx, my, blocks) == (2, 2, 24) and coef.shape == (24, 64) and coef.dtype == np.int16
    c = coef.reshape(2, 2, 6, 64)
    # 17 x 23: three Y block rows, three Y block columns: the right half of the right MCUs and the bottom half of the bottom MCUs are dummies
    for m_y, m_x, j in ((0, 1, 1), (0, 1, 3), (1, 0, 2), (1, 0, 3), (1, 1, 1), (1, 1, 2), (1, 1, 3)):
        assert not c[m_y, m_x, j, 1:].any() and c[m_y, m_x, j, 0] == c[m_y, m_x, j - 1, 0]
    assert c[0, 0, :, 1:].any(axis=1).all()
    seg = R.segment(coef)
    assert R.encode(x) == R.header(17, 23) + seg.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    # the constant image: after the first MCU every block is a zero difference and an end-of-block: 4 * 6 + 2 * 4 bits per MCU
    k = R.coefficients(R.pattern("constant", 64, 64))
    assert not k[:, 1:].any()
    assert len(R.segment(k)) == len(R.segment(k[:6])) + 15 * 4


def test_photo_at_the_reference_size_equals_pillow_and_is_quick():
    x = R.photo(1024, 1024)
    got = R.encode(x)
    assert got == _pillow(x)
    assert len(got) < 1024 * 1024 // 2  # (the first copy of to_jpeg, 4 bits per pixel, holds an image like this several times over)


@pytest.mark.parametrize("quality", [1, 30, 50, 75, 95, 100])
def test_header_and_tables_equal_pillows_file(quality):
    from where2edit_amd.image_io import jpeg_code_table, jpeg_header, jpeg_tables
    h, w = 37, 300
    head = jpeg_header(h, w, quality)
    want = _pillow(R.pattern("random", h, w), quality)
    assert head == want[:len(head)] and head == R.header(h, w, quality)
    assert head[-14:-12] == b"\xff\xda" and len(head) == 623
    luma, chroma = jpeg_tables(quality)
    assert luma.dtype == torch.int32 and tuple(luma.shape) == (64,) and not luma.is_cuda
    # Pillow's own DQT bytes: two segments of 2 + 2 + 1 + 64 bytes after SOI and the 18-byte APP0, zigzag order
    for k, t in enumerate((luma, chroma)):
        seg = want[20 + 69 * k:20 + 69 * (k + 1)]
        assert seg[:5] == bytes([0xFF, 0xDB, 0, 67, k])
        assert t.numpy()[R.ZIGZAG].tolist() == list(seg[5:])
        assert np.array_equal(t.numpy(), R.tables(quality)[k])
    assert jpeg_tables(quality)[0] is luma  # cached
    table = jpeg_code_table()
    assert table.dtype == torch.int32 and tuple(table.shape) == (4, 256)
    for t, (_, bits, vals) in enumerate(R.HUFFMAN):
        codes = R.huffman_codes(bits, vals)
        want_row = [(codes[s][0] << 5 | codes[s][1]) if s in codes else 0 for s in range(256)]
        assert table[t].tolist() == want_row


def test_header_without_pillow(golden):
    from where2edit_amd.image_io import jpeg_header
    recorded = [str(k) for k in golden["recorded"]]
    blob, offsets = golden["blob"].tobytes(), golden["offsets"]
    seen = set()
    for h, w, name, quality, seed in CASES:
        key = R.case_key(h, w, name, quality, seed)
        if key in recorded:
            i = recorded.index(key)
            head = jpeg_header(h, w, quality)
            assert blob[offsets[i]:offsets[i] + len(head)] == head, key
            seen.add(quality)
    assert seen == {1, 30, 75, 95, 100}


def test_entry_points_are_declared_prototyped_and_exported(lib):
    import where2edit_amd as W
    from where2edit_amd import _lib, image_io
    header = open(os.path.join(ROOT, "include", "w2e_jpeg.h")).read()
    want = {"*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M)
        assert m, f"{name} is not declared in include/w2e_jpeg.h"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            assert a is want["*" if "*" in p else p.split()[0]], (name, p, a)
        assert hasattr(lib, name)
    assert _lib.header_version() == 7 and "w2e_jpeg_entropy" in open(os.path.join(ROOT, "include", "w2e.h")).read()
    for name in ("jpeg_tables", "jpeg_header", "jpeg_coefficients", "to_jpeg", "save_image"):
        assert name in W._IMAGE_IO and getattr(W, name) is getattr(image_io, name)
    assert os.path.exists(os.path.join(ROOT, "where2edit_amd", "csrc", "jpeg.hip"))


def _plan(lib, batch, h, w):
    plan = (ctypes.c_int64 * 8)()
    return lib.w2e_jpeg_plan(batch, h, w, plan), list(plan)


def test_plan_numbers_by_hand(lib):
    # 1 x 1: one MCU, six blocks; workspace = offsets (7 * 8) + slots (6 * 208) + lengths (6 * 4)
    assert _plan(lib, 1, 1, 1) == (0, [6, 1, 1, 56 + 1248 + 24, 1248, 384, 1, 1024])
    # 17 x 23: 2 x 2 MCUs; a batch of three
    assert _plan(lib, 3, 17, 23) == (0, [24, 2, 2, 3 * (25 * 8 + 24 * 208 + 24 * 4), 24 * 208, 24 * 64, 3 * 2 * 1, 1024])
    # 264 x 520: 33 x 17 MCUs, 3366 blocks: three tiles of the prefix sum and 294 blocks; 5 strips of 8 MCUs per MCU row
    rc, p = _plan(lib, 1, 264, 520)
    assert rc == 0 and p[:3] == [3366, 33, 17] and p[0] > 3 * p[7] and p[6] == 17 * 5
    # the reference's size, and the largest
    rc, p = _plan(lib, 8, 1024, 1024)
    assert rc == 0 and p[0] == 24576 and p[4] == 24576 * 208 and p[6] == 8 * 64 * 8
    rc, p = _plan(lib, 1, 16384, 16384)
    assert rc == 0 and p[0] == 6 * 1024 * 1024 and p[3] == 8 * (p[0] + 1) + 212 * p[0]
    assert _plan(lib, 0, 8, 8) == (0, [6, 1, 1, 0, 1248, 384, 0, 1024])
    for h, w in R.ALL_SIZES:
        mx, my, blocks = R.geometry(h, w)
        assert _plan(lib, 1, h, w)[1][:3] == [blocks, mx, my]
    from where2edit_amd.image_io import jpeg_plan
    assert jpeg_plan(2, 70, 38) == {"blocks": 90, "mcus": (5, 3), "workspace": 2 * (91 * 8 + 90 * 212), "segment": 90 * 208, "coefficients": 90 * 64,
                                    "strips": 10, "scan_tile": 1024}


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    err = lib.w2e_last_error
    plan = (ctypes.c_int64 * 8)()
    assert lib.w2e_jpeg_plan(1, 8, 8, None) != 0 and b"null" in err()
    assert lib.w2e_jpeg_plan(-1, 8, 8, plan) != 0 and b"batch" in err()
    assert lib.w2e_jpeg_plan(1, 0, 8, plan) != 0 and b"1..16384" in err()
    assert lib.w2e_jpeg_plan(1, 8, 16385, plan) != 0 and b"1..16384" in err()

    def coefficients(src=p, batch=1, h=8, w=8, quality=75, coef=p):
        return lib.w2e_jpeg_coefficients(src, batch, h, w, quality, coef, None)

    assert coefficients(src=None) != 0 and b"null" in err()
    assert coefficients(coef=None) != 0 and b"null" in err()
    assert coefficients(batch=-1) != 0 and b"batch" in err()
    assert coefficients(h=0) != 0 and coefficients(w=16385) != 0 and b"1..16384" in err()
    assert coefficients(quality=0) != 0 and b"quality" in err()
    assert coefficients(quality=101) != 0 and b"quality" in err()
    assert coefficients(coef=ctypes.c_void_p(68)) != 0 and b"aligned" in err()
    assert coefficients(batch=0) == 0  # an empty batch: nothing to launch

    def entropy(coef=p, batch=1, h=8, w=8, huff=p, out=p, stride=1248, lengths=p, work=p):
        return lib.w2e_jpeg_entropy(coef, batch, h, w, huff, out, stride, lengths, work, None)

    for name in ("coef", "huff", "out", "lengths"):
        assert entropy(**{name: None}) != 0 and b"null" in err()
    assert entropy(work=None) != 0 and b"workspace" in err()
    assert entropy(batch=-1) != 0 and entropy(h=0) != 0 and entropy(w=16385) != 0
    assert entropy(stride=1244) != 0 and b"out_stride" in err()
    assert entropy(stride=1250) != 0 and b"multiples of 4" in err()
    assert entropy(out=ctypes.c_void_p(66)) != 0 and b"multiples of 4" in err()
    assert entropy(work=ctypes.c_void_p(68)) != 0 and b"8-byte" in err()
    assert entropy(lengths=ctypes.c_void_p(68)) != 0 and b"8-byte" in err()
    assert entropy(batch=65536) != 0 and b"65535" in err()
    assert entropy(batch=0) == 0


def test_python_side_refuses_what_it_does_not_take(tmp_path):
    from where2edit_amd import image_io as I
    u8 = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    gpu_msg = r"must be on the GPU.*\.to\('cuda'\)"
    for fn in (I.to_jpeg, I.jpeg_coefficients):
        with pytest.raises(RuntimeError, match=gpu_msg):
            fn(u8)
        with pytest.raises(RuntimeError, match=gpu_msg):
            fn(u8[0])
        with pytest.raises(RuntimeError, match="must be a tensor"):
            fn(np.zeros((8, 8, 3), np.uint8))
        with pytest.raises(RuntimeError, match="must be torch.uint8"):
            fn(torch.zeros(8, 8, 3))
        with pytest.raises(RuntimeError, match="3 or 4 dimensions"):
            fn(u8[0, 0])
    with pytest.raises(RuntimeError, match=gpu_msg):
        I.save_image(torch.zeros(1, 3, 8, 8), str(tmp_path / "a.jpg"))
    with pytest.raises(ValueError, match="PNG"):
        I.save_image(torch.zeros(1, 3, 8, 8), str(tmp_path / "a.png"))
    with pytest.raises(ValueError, match="PNG"):
        I.save_image(torch.zeros(1, 3, 8, 8), tmp_path / "a")
    with pytest.raises(ValueError, match="write"):
        I.save_image(torch.zeros(1, 3, 8, 8), 3)
    with pytest.raises(ValueError, match="1..100"):
        I.save_image(torch.zeros(1, 3, 8, 8), str(tmp_path / "a.jpg"), quality=0)
    assert not list(tmp_path.iterdir())
    for q in (0, 101, 75.0, None, True):
        with pytest.raises(ValueError, match="1..100"):
            I.jpeg_tables(q)
        with pytest.raises(ValueError, match="1..100"):
            I.jpeg_header(8, 8, q)
    with pytest.raises(ValueError, match="1..16384"):
        I.jpeg_header(0, 8)
    with pytest.raises(ValueError, match="1..16384"):
        I.jpeg_header(8, 16385)
