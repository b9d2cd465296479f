"""JPEG decoding, host side (no GPU): the numpy restatement (tests/jpeg_decode_ref.py) against Pillow and against the recorded digests of
Pillow's pixels (tests/golden/jpeg_decode.npz); the relaxation model against the sequential decoder; the C ABI of csrc/jpeg_decode.hip
(declared, prototyped, exported, the plan's numbers, argument errors); image_io.jpeg_parse against the restatement's parser, and its
refusal of what the decoder does not take."""
import ctypes
import functools
import hashlib
import io
import os
import re

import numpy as np
import pytest
import torch

import jpeg_decode_ref as D
import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("w2e_jpeg_decode_plan", "w2e_jpeg_decode_sync", "w2e_jpeg_decode_coefficients", "w2e_jpeg_pixels")
NAMES = ("jpeg_parse", "jpeg_decode_states", "jpeg_decode_coefficients", "jpeg_pixels", "from_jpeg", "load_image")
SIZES = R.ALL_SIZES + (D.PHOTO_SIZE,)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"))

    def files(prefix):
        blob, offsets = g[prefix + "_blob"].tobytes(), g[prefix + "_offsets"]
        return {str(k): blob[offsets[i]:offsets[i + 1]] for i, k in enumerate(g[prefix + "_keys"])}

    sha = dict(zip((str(k) for k in g["enc_keys"]), (str(s) for s in g["enc_sha256"])))
    sha.update(zip((str(k) for k in g["pil_keys"]), (str(s) for s in g["pil_sha256"])))
    return {"enc_keys": [str(k) for k in g["enc_keys"]], "pil_keys": [str(k) for k in g["pil_keys"]], "files": files("pil"), "refused": files("refused"),
            "sha256": sha}


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in SYMBOLS:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


def _all_cases(golden):
    out = {key: (h, w, make) for key, h, w, make in D.encode_cases()}
    out.update({c[0]: (c[1], c[2], functools.partial(golden["files"].__getitem__, c[0])) for c in D.pillow_cases()})
    return out


def test_the_case_list_covers_what_the_decoder_can_get_wrong(golden):
    assert golden["enc_keys"] == [c[0] for c in D.encode_cases()], "the fixture was recorded from another case list: run tests/golden/make_golden_jpeg_decode.py"
    assert golden["pil_keys"] == [c[0] for c in D.pillow_cases()] and len(golden["pil_keys"]) == len(D.PILLOW_SIZES) * len(D.PILLOW_VARIANTS) * len(D.PILLOW_PATTERNS)
    assert len(golden["enc_keys"]) == len(R.cases()) + 2 == 128
    assert {(1, 1), (8, 8), (16, 16), (17, 23), (33, 16), (40, 56)} <= set(D.PILLOW_SIZES) and max(h * w for h, w in D.PILLOW_SIZES) <= 40 * 56
    samplings = {D.parse(golden["files"][k])["sampling"] for k in golden["pil_keys"]}
    assert samplings == {"420", "444", "grey"}
    annex_k = {(tuple(b), bytes(v)) for _, b, v in R.HUFFMAN}
    own = [k for k in golden["pil_keys"] if not {t for c in D.parse(golden["files"][k])["dht"] for t in c} <= annex_k]
    assert own and all("opt" in k for k in own)  # optimize=True files carry their own Huffman tables
    assert tuple(golden["refused"]) == D.REFUSED
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz")) < 400 * 1024


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ref_decode_equals_pillow_and_the_recorded_digests(size, golden):
    """Every file of the size: the restatement's pixels against the recorded SHA-256 of Pillow's, always; against Pillow itself where
    it imports."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    seen = 0
    for key, (h, w, make) in _all_cases(golden).items():
        if (h, w) != tuple(size):
            continue
        data = make()
        got = D.decode(data)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        assert hashlib.sha256(got.tobytes()).hexdigest() == golden["sha256"][key], key
        if Image is not None:
            assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))), key
        seen += 1
    assert seen >= (2 if size == D.PHOTO_SIZE else 8)


def test_ref_coefficients_equal_the_encoders():
    """On jpeg_ref.encode's files the decoder restatement returns jpeg_ref.coefficients, also through the three passes of the kernels
    (count, place, write) at every subsequence length."""
    for case in R.cases()[::5]:
        h, w, name, quality, seed = case
        x = R.pattern(name, h, w, seed)
        parsed = D.parse(R.encode(x, quality))
        want = R.coefficients(x, quality)
        got, status = D.coefficients(parsed)
        assert status == 0 and got.dtype == np.int16 and np.array_equal(got, want), case
        if h * w <= 48 * 40:
            for sub_bits in (32, 128, 1024):
                got, status = D.coefficients(parsed, sub_bits)
                assert status == 0 and np.array_equal(got, want), (case, sub_bits)


def _streams(golden):
    mixed = R.encode(R.pattern("mixed", 70, 38, 4))
    checker = R.encode(R.pattern("checker", 48, 40, 12), 100)
    constant = R.encode(R.pattern("constant", 130, 262, 8))
    return {"mixed": mixed, "checker": checker, "constant": constant, "444opt": golden["files"]["pil_444opt95_40x56_random"],
            "1x1": R.encode(R.pattern("random", 1, 1, 0))}


@pytest.mark.parametrize("sub_bits", [32, 64, 128, 1024])
def test_the_relaxation_reaches_the_sequential_states(sub_bits, golden):
    for name, data in _streams(golden).items():
        stream = D.Stream(D.parse(data))
        want = D.sequential_states(stream, sub_bits)
        n = stream.subsequences(sub_bits)
        assert want.shape == (n, 3) and (want[:, 0] >= np.arange(n) * sub_bits).all() and tuple(want[0]) == (0, 0, 0)
        got, rounds = D.relax(stream, sub_bits)
        assert np.array_equal(got, want) and 1 <= rounds <= n, (name, rounds, n)
        got, launches = D.relax_two_level(stream, sub_bits)
        assert np.array_equal(got, want) and 1 <= launches <= -(-n // D.GROUP) + 1, (name, launches, n)
        got, launches = D.relax_two_level(stream, sub_bits, group=4)  # (many workgroups: the hand-over itself)
        assert np.array_equal(got, want) and 1 <= launches <= -(-n // 4) + 1, (name, launches, n)
        if name == "constant" and sub_bits == 32:
            assert rounds > n // 2  # the bad case: a stream that parses consistently at a wrong MCU phase


def test_f_is_total_on_nonsense(golden):
    """Bits that begin no code advance by one bit; a state past the end comes back unchanged; a cut scan gives a status."""
    data = _streams(golden)["mixed"]
    parsed = D.parse(data)
    stream = D.Stream(parsed)
    assert stream.f(0, (5000, 1, 3), 128) == ((5000, 1, 3), 0, 0)
    junk = dict(parsed, scan=b"\xff" * 8)
    s = D.Stream(junk)
    assert s.walk((0, 0, 0), 64) == ((64, 0, 0), 0, 0)  # sixteen 1-bits are no code of the Annex K tables
    assert D.coefficients(junk)[1] & D.STATUS_COUNT
    cut = dict(parsed, scan=parsed["scan"][:len(parsed["scan"]) // 2])
    assert D.coefficients(cut)[1] & D.STATUS_COUNT and D.coefficients(cut, 128)[1] == D.coefficients(cut)[1]


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
    assert _lib.header_version() == 7 and lib.w2e_version() == 7 and "w2e_jpeg_pixels" in open(os.path.join(ROOT, "include", "w2e.h")).read()
    for name in NAMES:
        assert name in W._IMAGE_IO and getattr(W, name) is getattr(image_io, name)
    assert os.path.exists(os.path.join(ROOT, "where2edit_amd", "csrc", "jpeg_decode.hip"))
    assert (image_io._JPEG_TABLE_WORDS, image_io._JPEG_MAX_SCAN_BITS) == tuple(
        int(re.search(r"#define\s+" + n + r"\s+(\w+)", header).group(1), 0) for n in ("W2E_JPEG_TABLE_WORDS", "W2E_JPEG_MAX_SCAN_BITS"))
    assert [int(re.search(r"#define\s+W2E_JPEG_" + n.upper() + r"\s+(\d+)", header).group(1)) for n in image_io.JPEG_SAMPLINGS] == [0, 1, 2]
    assert int(re.search(r"#define\s+W2E_JPEG_DECODE_GROUP\s+(\d+)", header).group(1)) == D.GROUP


def _plan(lib, batch, h, w, sampling, scan_bits, sub_bits):
    plan = (ctypes.c_int64 * 8)()
    return lib.w2e_jpeg_decode_plan(batch, h, w, sampling, scan_bits, sub_bits, plan), list(plan)


def test_plan_numbers_by_hand_and_against_the_restatement(lib):
    # 1 x 1, 4:2:0: one MCU of six blocks; 100 bits in subsequences of 32: four, one workgroup, two launches at the most
    assert _plan(lib, 1, 1, 1, 0, 100, 32) == (0, [6, 1, 1, 4, 16 * (4 + 1), 6 * 64, 2, 384])
    assert _plan(lib, 1, 1, 1, 1, 100, 32)[1][:3] == [3, 1, 1] and _plan(lib, 1, 1, 1, 2, 100, 32)[1][:3] == [1, 1, 1]
    # an empty scan is one subsequence
    assert _plan(lib, 2, 17, 23, 0, 0, 1024) == (0, [24, 2, 2, 1, 2 * 16 * 2, 2 * 24 * 64, 2, 24 * 64])
    # 264 x 520: 33 x 17 MCUs of 16, 65 x 33 of 8; 562 subsequences of 32 bits are three workgroups
    assert _plan(lib, 3, 264, 520, 0, 562 * 32, 32) == (0, [3366, 33, 17, 562, 3 * 16 * (562 + 3), 3 * 3366 * 64, 4, 3366 * 64])
    assert _plan(lib, 1, 264, 520, 1, 562 * 32 - 31, 32)[1][:4] == [3 * 65 * 33, 65, 33, 562]
    assert _plan(lib, 1, 264, 520, 2, 562 * 32 + 1, 32)[1][:4] == [65 * 33, 65, 33, 563]
    # the reference's size at quality 75: 726 kbit
    rc, p = _plan(lib, 8, 1024, 1024, 0, 726000, 1024)
    assert rc == 0 and p[0] == 24576 and p[3] == 709 and p[6] == 4 and p[5] == 8 * 1024 * 1024 * 3 // 2
    assert _plan(lib, 0, 8, 8, 0, 64, 64) == (0, [6, 1, 1, 1, 0, 0, 2, 384])
    for h, w in R.ALL_SIZES:
        for s, name in enumerate(("420", "444", "grey")):
            mx, my, blocks = D.geometry(h, w, name)
            assert _plan(lib, 1, h, w, s, 4096, 4096)[1][:3] == [blocks, mx, my]
    from where2edit_amd.image_io import jpeg_decode_plan
    stream = D.Stream(D.parse(R.encode(R.pattern("mixed", 70, 38, 4))))
    assert jpeg_decode_plan(2, 70, 38, "420", stream.bits, 128) == {
        "blocks": 90, "mcus": (5, 3), "subsequences": stream.subsequences(128), "workspace": 2 * 16 * (stream.subsequences(128) + 1),
        "pixel_workspace": 2 * 90 * 64, "launches": 2, "coefficients": 90 * 64}


def test_argument_validation_needs_no_gpu(lib):
    p = ctypes.c_void_p(64)
    err = lib.w2e_last_error
    plan = (ctypes.c_int64 * 8)()

    def planned(batch=1, h=8, w=8, sampling=0, scan_bits=64, sub_bits=32, out=plan):
        return lib.w2e_jpeg_decode_plan(batch, h, w, sampling, scan_bits, sub_bits, out)

    assert planned(out=None) != 0 and b"null" in err()
    assert planned(batch=-1) != 0 and planned(batch=65536) != 0 and b"batch" in err()
    assert planned(h=0) != 0 and planned(w=16385) != 0 and b"1..16384" in err()
    assert planned(sampling=3) != 0 and planned(sampling=-1) != 0 and b"sampling" in err()
    for bad in (0, 16, 48, 33, 4128, -32):
        assert planned(sub_bits=bad) != 0 and b"sub_bits" in err(), bad
    assert planned(scan_bits=-1) != 0 and planned(scan_bits=1 << 31) != 0 and b"scan_bits" in err()
    assert planned(sub_bits=4096) == 0 and planned(scan_bits=0x7fff0000) == 0

    def stream_call(fn, tail, scan=p, meta=p, tables=p, scan_bytes=8, batch=1, h=8, w=8, sampling=0, scan_bits=64, sub_bits=32, work=p):
        return fn(scan, meta, tables, scan_bytes, batch, h, w, sampling, scan_bits, sub_bits, *tail(work))

    def sync(launch=0, changed=p, **kw):
        return stream_call(lib.w2e_jpeg_decode_sync, lambda work: (launch, work, changed, None), **kw)

    def coefficients(coef=p, status=p, **kw):
        return stream_call(lib.w2e_jpeg_decode_coefficients, lambda work: (work, coef, status, None), **kw)

    for fn in (sync, coefficients):
        for name in ("scan", "meta", "tables"):
            assert fn(**{name: None}) != 0 and b"null" in err()
        assert fn(work=None) != 0 and b"workspace" in err()
        assert fn(batch=-1) != 0 and b"batch" in err()
        assert fn(h=0) != 0 and fn(w=16385) != 0 and b"1..16384" in err()
        assert fn(sampling=3) != 0 and b"sampling" in err()
        assert fn(sub_bits=48) != 0 and fn(sub_bits=0) != 0 and b"sub_bits" in err()
        assert fn(scan_bits=-1) != 0 and b"scan_bits" in err()
        assert fn(scan_bytes=6) != 0 and fn(scan_bytes=-4) != 0 and b"scan_bytes" in err()
        assert fn(scan=ctypes.c_void_p(66)) != 0 and fn(meta=ctypes.c_void_p(68)) != 0 and fn(work=ctypes.c_void_p(68)) != 0 and b"aligned" in err()
        assert fn(batch=0) == 0  # an empty batch: nothing to launch
    assert sync(changed=None) != 0 and b"changed" in err()
    assert sync(launch=-1) != 0 and sync(launch=2) != 0 and b"launch" in err()  # 64 bits of 32: one workgroup, launches 0 and 1
    assert coefficients(coef=None) != 0 and coefficients(status=None) != 0 and b"null" in err()
    assert coefficients(coef=ctypes.c_void_p(72)) != 0 and b"16-byte" in err()

    def pixels(coef=p, q=p, batch=1, h=8, w=8, sampling=0, out=p, work=p):
        return lib.w2e_jpeg_pixels(coef, q, batch, h, w, sampling, out, work, None)

    for name in ("coef", "q", "out"):
        assert pixels(**{name: None}) != 0 and b"null" in err()
    assert pixels(work=None) != 0 and b"workspace" in err()
    assert pixels(batch=-1) != 0 and pixels(h=0) != 0 and pixels(w=16385) != 0 and pixels(sampling=5) != 0 and b"sampling" in err()
    assert pixels(coef=ctypes.c_void_p(72)) != 0 and pixels(work=ctypes.c_void_p(72)) != 0 and pixels(out=ctypes.c_void_p(66)) != 0 and b"aligned" in err()
    assert pixels(batch=0) == 0


def test_jpeg_parse_equals_the_restatements_parser(golden):
    from where2edit_amd.image_io import _jpeg_decode_table, jpeg_parse
    cases = _all_cases(golden)
    for key in list(cases)[::9] + [k for k in golden["pil_keys"] if "_40x56_" in k]:
        data = cases[key][2]()
        got, want = jpeg_parse(data), D.parse(data)
        assert (got["h"], got["w"], got["sampling"]) == (want["h"], want["w"], want["sampling"]), key
        assert got["tables"].dtype == torch.int32 and np.array_equal(got["tables"].numpy(), want["q"]), key
        assert got["huffman"] == want["dht"] and got["scan"] == want["scan"], key
        assert jpeg_parse(bytearray(data))["scan"] == want["scan"]
    # the kernels' view of a code table against the full 16-bit look-up of the restatement: Annex K, and a file's own
    own = D.parse(golden["files"]["pil_444opt95_40x56_random"])["dht"]
    for counts, symbols in [(tuple(b), bytes(v)) for _, b, v in R.HUFFMAN] + [t for c in own for t in c]:
        t, full = _jpeg_decode_table(counts, symbols), D._lookup(counts, symbols)
        assert t.dtype == np.uint32 and t.shape == (384,)
        lut, maxcode, valoff, vals = t[:256].view(np.uint16), t[256:274].view(np.int32), t[274:291].view(np.int32), t[320:].view(np.uint8)
        for v in list(range(0, 1 << 16, 13)) + [0xFFFF]:
            e = int(lut[v >> 7])
            if e == 0:
                e = next(((n << 8) | int(vals[((v >> (16 - n)) + valoff[n]) & 255]) for n in range(10, 17) if (v >> (16 - n)) <= maxcode[n]), 0)
            assert e == full[v], (counts, v)


def test_jpeg_parse_refuses_what_is_out_of_scope(golden):
    from where2edit_amd.image_io import from_jpeg, jpeg_parse, load_image
    refused = golden["refused"]
    for key, word in (("progressive", "progressive"), ("422", r"4:2:2"), ("cmyk", "CMYK"), ("png", "PNG")):
        with pytest.raises(ValueError, match=word + ".*decode it with Pillow"):
            jpeg_parse(refused[key])
        with pytest.raises(ValueError, match="decode it with Pillow"):  # on the host, before any launch: no GPU is asked for
            from_jpeg(refused[key])
        with pytest.raises(ValueError, match="decode it with Pillow"):
            load_image(io.BytesIO(refused[key]))
    good = golden["files"]["pil_444_40x56_mixed"]
    for cut in (3, 20, 100, good.index(b"\xff\xda") + 5):
        with pytest.raises(ValueError, match="cut inside its header.*decode it with Pillow"):
            jpeg_parse(good[:cut])
    with pytest.raises(ValueError, match="no JPEG"):
        jpeg_parse(b"")
    with pytest.raises(ValueError, match="bytes of a JPEG"):
        jpeg_parse("a.jpg")
    head = good[:good.index(b"\xff\xc0")]
    sof = good[good.index(b"\xff\xc0"):]
    with pytest.raises(ValueError, match="restart interval"):
        jpeg_parse(head + b"\xff\xdd\x00\x04\x00\x08" + sof)
    assert jpeg_parse(head + b"\xff\xdd\x00\x04\x00\x00" + sof)["scan"] == jpeg_parse(good)["scan"]  # DRI 0 switches restarts off
    with pytest.raises(ValueError, match="12-bit"):
        jpeg_parse(head + sof[:4] + b"\x0c" + sof[5:])
    with pytest.raises(ValueError, match="arithmetic"):
        jpeg_parse(head + b"\xff\xc9" + sof[2:])
    with pytest.raises(ValueError, match="several scans"):
        jpeg_parse(good[:-2] + good[good.index(b"\xff\xda"):])
    no_jfif = good[:2] + good[good.index(b"\xff\xdb"):]  # without JFIF or Adobe the component ids decide: 1 2 3 is YCbCr, R G B is not
    assert jpeg_parse(no_jfif)["sampling"] == "444"
    at = no_jfif.index(b"\xff\xc0") + 10
    rgb = bytearray(no_jfif)
    rgb[at], rgb[at + 3], rgb[at + 6] = b"RGB"
    sos = rgb.index(b"\xff\xda") + 5
    rgb[sos], rgb[sos + 2], rgb[sos + 4] = b"RGB"
    with pytest.raises(ValueError, match="RGB-coded"):
        jpeg_parse(bytes(rgb))
    # a file that ends inside its scan is left to the kernels' status
    assert len(jpeg_parse(good[:-40])["scan"]) < len(jpeg_parse(good)["scan"])


def test_python_side_refuses_what_it_does_not_take(golden, tmp_path):
    from where2edit_amd import image_io as I
    good = golden["files"]["pil_444_40x56_mixed"]
    for bad in (0, 16, 48, 8192, 1024.0, None, True):
        for fn in (I.from_jpeg, I.jpeg_decode_states, I.jpeg_decode_coefficients):
            with pytest.raises(ValueError, match="sub_bits"):
                fn(good, sub_bits=bad)
    for fn in (I.jpeg_decode_states, I.jpeg_decode_coefficients):
        with pytest.raises(ValueError, match="agree in height, width and sampling"):
            fn([good, golden["files"]["pil_grey_40x56_mixed"]])
    with pytest.raises(ValueError, match="stack=True"):
        I.from_jpeg([good, golden["files"]["pil_444_17x23_mixed"]], stack=True)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        I.jpeg_pixels(torch.zeros(105, 64, dtype=torch.int16), torch.ones(3, 64, dtype=torch.int32), 40, 56, "444")
    with pytest.raises(RuntimeError, match="must be torch.int16"):
        I.jpeg_pixels(torch.zeros(105, 64), torch.ones(3, 64, dtype=torch.int32), 40, 56, "444")
    with pytest.raises(ValueError, match="read"):
        I.load_image(3)
    with pytest.raises(RuntimeError, match="device must be a GPU.*no CPU path"):
        I.from_jpeg(good, device="cpu")
    # save_image still writes JPEG only
    with pytest.raises(ValueError, match="PNG"):
        I.save_image(torch.zeros(1, 3, 8, 8), str(tmp_path / "a.png"))
