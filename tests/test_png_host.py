"""The PNG decoder without a GPU: the restatement of tests/png_ref.py against its sources (zlib, the recorded Pillow pixels of
tests/golden/png.npz, Pillow itself where it imports); the census of the case list -- what every stream is in the list for, asserted
from what the restatement's inflate saw; image_io.png_parse; the plan and the argument checks of the C ABI; and the decoder's core
(csrc/png_core.h, the very text the kernels compile) as a stand-alone host program under AddressSanitizer and
UndefinedBehaviorSanitizer on the valid list and on the corrupt list."""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("w2e_png_plan", "w2e_png_inflate", "w2e_png_pixels")
NAMES = ("png_parse", "png_plan", "png_inflate", "png_pixels", "from_png", "load_png", "read_image")


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "png.npz"))

    def files(prefix):
        blob, offsets = g[prefix + "blob"].tobytes(), g[prefix + "offsets"]
        return {str(k): blob[offsets[i]:offsets[i + 1]] for i, k in enumerate(g[prefix + "keys"])}

    return {"files": files(""), "refused": files("refused_"), "rgb": {k: g["rgb_" + k] for k in files("")}, "raw": {k: g["raw_" + k] for k in files("")},
            "pillow": str(g["pillow"])}


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


@pytest.fixture(scope="module")
def censuses():
    out = {}
    for name, (z, data) in P.valid_cases().items():
        inflated, census = P.inflate(z)
        assert inflated == data == zlib.decompress(z), name  # the restatement's inflate equals zlib on the whole list
        out[name] = census
    return out


# ---- the restatement against its sources ----
def test_the_case_list_shows_what_an_inflate_can_get_wrong(censuses):
    c = censuses
    cases = P.valid_cases()
    assert c["stored_two"]["blocks"] == {0: 2, 1: 0, 2: 0} and len(cases["stored_two"][1]) > 65535  # two stored blocks
    assert c["stored_empty"]["empty_stored"] == 1                     # Z_SYNC_FLUSH in mid-stream: an empty stored block
    assert c["fixed"]["blocks"] == {0: 0, 1: 1, 2: 0}                 # strategy Z_FIXED
    assert c["dynamic_many"]["blocks"][2] >= 10                       # many dynamic blocks in one stream: the tables are rebuilt
    assert c["huffman_only"]["huffman_only"] and c["huffman_only"]["blocks"][2] == 1 and c["huffman_only"]["longest_match"] == 0
    assert c["run258"]["run258"] >= 100 and c["run258"]["overlaps"] == {1}  # run-length copies: length 258 at distance 1
    assert {2, 3} <= c["period2_3"]["overlaps"]                       # distances 2 and 3 below their length
    assert c["long_codes"]["longest_code"] >= 14                      # a code past the direct tables, by far
    assert c["far"]["largest_distance"] > 32000
    assert c["wbits9"]["wbits"] == 9
    assert len(cases["ring_wrap"][1]) > 70000 and c["ring_wrap"]["wraps"] >= 2  # matches across the wrap of a 32 KiB ring
    assert {len(z) % 8 for z, _ in cases.values()} == set(range(8))   # stream lengths of every residue mod 8
    h = c["hand_built"]                                               # what zlib never emits
    assert h["longest_code"] == 15 and h["largest_distance"] == 32768 and h["longest_match"] == 258 and h["blocks"] == {0: 1, 1: 0, 2: 1}
    z, data = P.valid_cases()["hand_built"]
    assert data[-258:] == data[14:14 + 258]


def test_the_corrupt_list_is_corrupt_in_the_way_it_says():
    reasons = {"TYPE": "type", "STORED": "stored", "LENGTHS": "lengths", "CODE": "code", "DISTANCE": "distance", "INPUT": "input", "ADLER": "adler"}
    for name, z, size, status in P.corrupt_cases():
        try:  # zlib refuses it too, unless only the size is wrong
            inflated = zlib.decompress(z)
        except zlib.error:
            inflated = None
        assert (inflated is None) == (status not in ("LONG", "SHORT")) and (inflated is None or len(inflated) != size), name
        if status in reasons:
            with pytest.raises(P.Corrupt, match=reasons[status]):
                P.inflate(z)
        elif status in ("LONG", "SHORT"):
            assert (len(P.inflate(z)[0]) > size) == (status == "LONG")
    z, h, w = P.corrupt_filter()
    with pytest.raises(P.Corrupt, match="filter"):
        P.unfilter(zlib.decompress(z), h, w, 1)


def test_ref_decode_equals_the_recorded_pillow_pixels(golden):
    assert set(golden["files"]) == {"L", "P8", "P4", "P_trns", "RGB", "RGBA", "LA", "RGB_optimize", "RGB_level1", "L_level9"}
    depths = {k: f[24] for k, f in golden["files"].items()}
    assert depths["P4"] == 4 and depths["P8"] == 8 and b"tRNS" in golden["files"]["P_trns"]
    for key, data in golden["files"].items():
        assert np.array_equal(P.decode(data, "RGB"), golden["rgb"][key]), key
        assert np.array_equal(P.decode(data, "raw"), golden["raw"][key]), key


def test_ref_decode_equals_pillow(golden):
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(0)
    files = list(golden["files"].values())
    for colour, depth in ((0, 8), (2, 8), (4, 8), (6, 8), (3, 8), (3, 4), (3, 2), (3, 1)):
        px = rng.integers(0, 1 << depth if colour == 3 else 256, (11, 13) + ((P.CHANNELS[colour],) if P.CHANNELS[colour] > 1 else ()), dtype=np.uint8)
        pal = rng.integers(0, 256, (min(1 << depth, 200), 3), dtype=np.uint8) if colour == 3 else None
        files.append(P.write_png(px, colour, depth, palette=pal, filters=rng.integers(0, 5, 11).tolist(), idat=50))
    for data in files:
        assert np.array_equal(P.decode(data, "RGB"), np.asarray(Image.open(io.BytesIO(data)).convert("RGB")))
        assert np.array_equal(P.decode(data, "raw"), np.asarray(Image.open(io.BytesIO(data))))


def test_the_writer_round_trips_through_the_restatement():
    rng = np.random.default_rng(1)
    for colour, depth in ((0, 8), (2, 8), (4, 8), (6, 8), (3, 8), (3, 4), (3, 2), (3, 1)):
        c = P.CHANNELS[colour]
        px = rng.integers(0, 1 << depth if colour == 3 else 256, (9, 7) + ((c,) if c > 1 else ()), dtype=np.uint8)
        pal = rng.integers(0, 256, (1 << depth, 3), dtype=np.uint8) if colour == 3 else None
        data = P.write_png(px, colour, depth, palette=pal, filters=[0, 1, 2, 3, 4, 4, 3, 2, 1], idat=31, level=9)
        assert np.array_equal(P.decode(data, "raw"), px), (colour, depth)


# ---- png_parse ----
def test_png_parse_every_colour_type_and_depth():
    from where2edit_amd.image_io import png_parse
    rng = np.random.default_rng(2)
    for colour, depth in ((0, 8), (2, 8), (4, 8), (6, 8), (3, 8), (3, 4), (3, 2), (3, 1)):
        c = P.CHANNELS[colour]
        px = rng.integers(0, 1 << depth if colour == 3 else 256, (6, 10) + ((c,) if c > 1 else ()), dtype=np.uint8)
        pal = rng.integers(0, 256, (min(1 << depth, 5), 3), dtype=np.uint8) if colour == 3 else None
        data = P.write_png(px, colour, depth, palette=pal, extra=((b"tRNS", b"\0\1"), (b"tEXt", b"k\0v")), wbits=9 if colour == 2 else 15)
        got = png_parse(data)
        assert (got["h"], got["w"], got["colour"], got["depth"]) == (6, 10, colour, depth)
        assert zlib.decompress(got["stream"]) == P.filter_rows(P.pack_rows(px, colour, depth), P.filter_bpp(colour, depth), 0)
        if colour == 3:
            want = [int(r) | int(g) << 8 | int(b) << 16 for r, g, b in pal] + [0] * (256 - len(pal))
            assert got["palette"].tolist() == want
        else:
            assert got["palette"] is None
        split = png_parse(P.write_png(px, colour, depth, palette=pal, idat=7, wbits=9 if colour == 2 else 15))  # a split IDAT: the same stream
        assert split["stream"] == got["stream"] and len(list(P.chunks(P.write_png(px, colour, depth, palette=pal, idat=7)))) > 4
        assert png_parse(bytearray(data))["stream"] == got["stream"]


def test_png_parse_refuses_what_is_out_of_scope(golden):
    from where2edit_amd.image_io import png_parse
    px = np.arange(30, dtype=np.uint8).reshape(5, 6)
    good = P.write_png(px, 0)
    for key, word in (("interlaced", "interlaced"), ("16bit", "16-bit"), ("1bit_grey", "1-bit grey")):
        with pytest.raises(ValueError, match=word + r".*decode it with Pillow$"):
            png_parse(golden["refused"][key])
    with pytest.raises(ValueError, match=r"APNG.*decode it with Pillow$"):
        png_parse(P.write_png(px, 0, extra=((b"acTL", struct.pack(">II", 1, 0)),)))
    with pytest.raises(ValueError, match=r"preset dictionary.*decode it with Pillow$"):
        co = zlib.compressobj(zdict=b"abcdefgh")
        png_parse(P.wrap_idat(co.compress(bytes(35)) + co.flush(), 5, 6))
    big = P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", 16385, 4, 8, 0, 0, 0, 0)) + P.chunk(b"IDAT", zlib.compress(b"\0")) + P.chunk(b"IEND", b"")
    with pytest.raises(ValueError, match=r"1\.\.16384.*decode it with Pillow$"):
        png_parse(big)
    with pytest.raises(ValueError, match=r"no PNG.*decode it with Pillow$"):
        png_parse(b"\xff\xd8\xff\xe0" + bytes(20))
    at = good.index(b"IDAT") + 6
    with pytest.raises(ValueError, match="CRC of the IDAT chunk"):  # a damaged byte: Pillow raises too
        png_parse(good[:at] + bytes([good[at] ^ 1]) + good[at + 1:])
    with pytest.raises(ValueError, match="CRC of the IHDR chunk"):
        png_parse(good[:17] + bytes([good[17] ^ 1]) + good[18:])
    for cut in (len(good) - 5, good.index(b"IDAT") + 7, 20, 10):
        with pytest.raises(ValueError, match="cut inside"):
            png_parse(good[:cut])
    with pytest.raises(ValueError, match="zlib header"):
        png_parse(P.wrap_idat(b"\x00\x01abcd", 5, 6))
    with pytest.raises(ValueError, match="without a PLTE"):
        png_parse(P.write_png(px % 4, 3, 2))
    with pytest.raises(ValueError, match="without an IDAT"):
        png_parse(P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", 6, 5, 8, 0, 0, 0, 0)) + P.chunk(b"IEND", b""))
    with pytest.raises(ValueError, match="bytes of a PNG file"):
        png_parse("name.png")


def test_the_jpeg_side_still_refuses_a_png_and_the_python_side_checks_its_arguments():
    from where2edit_amd import image_io
    good = P.write_png(np.zeros((4, 4), np.uint8), 0)
    for fn in (image_io.jpeg_parse, image_io.from_jpeg):
        with pytest.raises(ValueError, match="a PNG.*decode it with Pillow"):
            fn(good)
    with pytest.raises(ValueError, match="mode must be one of"):
        image_io.from_png(good, mode="L")
    with pytest.raises(ValueError, match="path or an object with read"):
        image_io.load_png(7)
    with pytest.raises(ValueError, match="path or an object with read"):
        image_io.read_image(None)
    with pytest.raises(ValueError, match="one size"):
        image_io.png_inflate([zlib.compress(b"a")], [1, 2])
    with pytest.raises(ValueError, match="zlib header"):
        image_io.png_inflate(b"\x00\x00", 1)
    with pytest.raises(RuntimeError, match="device must be a GPU"):
        image_io.from_png(good, device="cpu")
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        import torch
        image_io.png_pixels(torch.zeros(20, dtype=torch.uint8), 4, 4, 0)


# ---- the C ABI ----
def test_entry_points_are_declared_prototyped_and_exported(lib):
    import where2edit_amd as W
    from where2edit_amd import _lib, evaluation, image_io
    header = open(os.path.join(ROOT, "include", "w2e_png.h")).read()
    want = {"*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name in SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", header, flags=re.M)
        assert m, f"{name} is not declared in include/w2e_png.h"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for p, a in zip(params, args):
            assert a is want["*" if "*" in p else p.split()[0]], (name, p, a)
        assert hasattr(lib, name)
        assert name == "w2e_png_plan" or params[-1] == "void* stream"
    assert _lib.header_version() == 7 and lib.w2e_version() == 7 and "w2e_png_pixels" in open(os.path.join(ROOT, "include", "w2e.h")).read()
    for name in NAMES:
        assert name in W._IMAGE_IO and getattr(W, name) is getattr(image_io, name)
    assert W.celebamask_samples is evaluation.celebamask_samples
    for name in ("png.hip", "png_core.h"):
        assert os.path.exists(os.path.join(ROOT, "where2edit_amd", "csrc", name))
    define = lambda n: int(re.search(r"#define\s+W2E_PNG_" + n + r"\s+(\d+)", header).group(1))
    assert define("BAND") == P.BAND and [define("MODE_" + m.upper()) for m in image_io.PNG_MODES] == [0, 1]
    assert {n: define("STATUS_" + n) for n in P.STATUS} == P.STATUS
    assert sorted(bit for bit, _ in image_io._PNG_STATUS) == sorted(P.STATUS.values())


def _plan(lib, batch, h, w, colour, depth, mode):
    plan = (ctypes.c_int64 * 8)()
    return lib.w2e_png_plan(batch, h, w, colour, depth, mode, plan), list(plan)


def test_plan_numbers_by_hand(lib):
    # 3 x 5 RGB: rows of 1 + 15 bytes, 48 in all
    assert _plan(lib, 1, 3, 5, 2, 8, 0) == (0, [16, 48, 48, 3, 45, 3, 40960, 64])
    assert _plan(lib, 1, 3, 5, 2, 8, 1)[1][3:5] == [3, 45]
    # 3 x 5 grey: rows of 6 bytes, 18 in all, 20 with the pitch's padding; one channel raw, three as RGB
    assert _plan(lib, 7, 3, 5, 0, 8, 1) == (0, [6, 18, 20, 1, 15, 1, 40960, 64])
    assert _plan(lib, 7, 3, 5, 0, 8, 0)[1][3:6] == [3, 45, 1]
    assert _plan(lib, 1, 3, 5, 4, 8, 1)[1][:6] == [11, 33, 36, 2, 30, 2] and _plan(lib, 1, 3, 5, 6, 8, 1)[1][:6] == [21, 63, 64, 4, 60, 4]
    # palettes: 9 pixels at 1, 2, 4, 8 bits are 2, 3, 5, 9 bytes
    assert [_plan(lib, 1, 2, 9, 3, d, 1)[1][0] for d in (1, 2, 4, 8)] == [3, 4, 6, 10]
    assert _plan(lib, 1, 2, 9, 3, 4, 1)[1][3:6] == [1, 18, 1] and _plan(lib, 1, 2, 9, 3, 4, 0)[1][3:6] == [3, 54, 1]
    # the workloads: a 512 x 512 label and a 1024 x 1024 RGB image
    assert _plan(lib, 90, 512, 512, 0, 8, 1)[1][:3] == [513, 512 * 513, 512 * 513]
    assert _plan(lib, 8, 1024, 1024, 2, 8, 0)[1][:5] == [3073, 1024 * 3073, 1024 * 3073, 3, 3 << 20]
    assert _plan(lib, 1, 16384, 16384, 6, 8, 0)[1][1] == 16384 * 65537
    from where2edit_amd.image_io import png_plan
    assert png_plan(2, 3, 4, 3, 2, "raw") == {"row_bytes": 2, "size": 6, "pitch": 8, "channels": 1, "out_bytes": 12, "bpp": 1, "lds": 40960, "band": 64}


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    err = lib.w2e_last_error
    plan = (ctypes.c_int64 * 8)()

    def planned(batch=1, h=8, w=8, colour=2, depth=8, mode=0, out=plan):
        return lib.w2e_png_plan(batch, h, w, colour, depth, mode, out)

    assert planned() == 0 and planned(batch=0) == 0 and planned(batch=65535) == 0
    assert planned(out=None) != 0 and b"null" in err()
    assert planned(batch=-1) != 0 and planned(batch=65536) != 0 and b"batch" in err()
    assert planned(h=0) != 0 and planned(w=16385) != 0 and b"1..16384" in err()
    for colour, depth in ((1, 8), (5, 8), (7, 8), (0, 1), (0, 4), (0, 16), (2, 16), (2, 4), (3, 16), (3, 3), (6, 1)):
        assert planned(colour=colour, depth=depth) != 0 and b"out of scope" in err(), (colour, depth)
    assert planned(mode=2) != 0 and planned(mode=-1) != 0 and b"mode" in err()

    def inflate(streams=p, meta=p, sizes=p, stream_bytes=8, batch=1, raw=p, pitch=8, status=p):
        return lib.w2e_png_inflate(streams, meta, sizes, stream_bytes, batch, raw, pitch, status, None)

    for name in ("streams", "meta", "sizes", "raw", "status"):
        assert inflate(**{name: None}) != 0 and b"null" in err()
    assert inflate(batch=-1) != 0 and inflate(batch=65536) != 0 and b"batch" in err()
    assert inflate(stream_bytes=6) != 0 and inflate(stream_bytes=-4) != 0 and b"stream_bytes" in err()
    assert inflate(pitch=0) != 0 and inflate(pitch=6) != 0 and b"raw_pitch" in err()
    for name, bad in (("streams", 66), ("raw", 65), ("status", 66), ("meta", 68), ("sizes", 68)):
        assert inflate(**{name: ctypes.c_void_p(bad)}) != 0 and b"aligned" in err(), name
    assert inflate(batch=0) == 0  # an empty batch: nothing to launch

    def pixels(raw=p, pitch=1 << 20, palette=p, batch=1, h=8, w=8, colour=2, depth=8, mode=0, out=p, status=p):
        return lib.w2e_png_pixels(raw, pitch, palette, batch, h, w, colour, depth, mode, out, status, None)

    for name in ("raw", "out", "status"):
        assert pixels(**{name: None}) != 0 and b"null" in err()
    assert pixels(palette=None, colour=3) != 0 and b"palette" in err()
    assert pixels(palette=None, batch=0) == 0 and pixels(palette=None, colour=3, mode=1, batch=0) == 0
    assert pixels(batch=-1) != 0 and pixels(h=0) != 0 and pixels(w=16385) != 0 and pixels(colour=1) != 0 and pixels(depth=4) != 0 and b"out of scope" in err()
    assert pixels(mode=3) != 0 and b"mode" in err()
    assert pixels(pitch=8 * 25 - 1) != 0 and b"raw_pitch" in err() and pixels(pitch=8 * 25, batch=0) == 0
    assert pixels(status=ctypes.c_void_p(66)) != 0 and pixels(palette=ctypes.c_void_p(66)) != 0 and b"aligned" in err()


# ---- the core under the sanitizers ----
def test_decoder_core_under_asan_and_ubsan(tmp_path):
    from where2edit_amd import build
    src = os.path.join(ROOT, "tests", "png_core_host.cpp")
    exe, corpus = str(tmp_path / "png_core_host"), str(tmp_path / "corpus.bin")
    valid, corrupt = P.write_corpus(corpus)
    assert valid == len(P.valid_cases()) + 5 and corrupt == len(P.corrupt_cases()) == 12
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    cc = subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", *san, "-x", "hip", src, "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert cc.returncode == 0, cc.stdout
    run = subprocess.run([exe, corpus], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "png_core_host: ok" in run.stdout, run.stdout
    assert f"png_core_host: {valid} valid and {corrupt} corrupt streams" in run.stdout
