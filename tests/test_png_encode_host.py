"""The PNG encoder without a GPU: the filter rule of tests/png_encode_ref.py against Pillow (itself where it imports, its recorded
rows everywhere); the deflate core (csrc/png_deflate_core.h, the very text the kernel compiles) as a stand-alone host program with
one lane under AddressSanitizer and UndefinedBehaviorSanitizer -- every stream inflates with zlib to its input, stays under the stored
bound and equals the recording of tests/golden/png_encode.npz; the size of the files against Pillow's; the plan, the argument checks
and the file assembly of the public surface."""
import ctypes
import hashlib
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

import png_encode_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("w2e_png_encode_plan", "w2e_png_deflate_plan", "w2e_png_filter", "w2e_png_deflate")
NAMES = ("png_encode_plan", "png_filter", "png_deflate", "to_png", "save_png")
SIZE_SLACK = 0.02  # a file may be this much of Pillow's size above its recorded ratio: the coder is deterministic, this stops a silent loss


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "png_encode.npz"))


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
def host(tmp_path_factory):
    """The core with one lane, built with the sanitizers and run once on everything the recording covers: name -> (input, stream)."""
    inputs = E.recorded_inputs()
    streams, said = E.host_streams(list(inputs.values()), tmp_path_factory.mktemp("png_deflate_host"))
    print(said)
    assert f"png_deflate_host: {len(inputs)} streams" in said
    return {name: (data, z) for (name, data), z in zip(inputs.items(), streams)}


# ---- stage 1: the filter rule ----
def test_filter_rule_equals_pillow(golden):
    cases = E.filter_cases()
    assert list(golden["filter_names"]) == list(cases) and len(cases) == 240
    assert {a.shape[2] for a in cases.values()} == {1, 2, 3, 4} and any(a.shape[0] == 1 for a in cases.values()) and any(a.shape[1] == 1 for a in cases.values())
    chosen = set()
    for (name, a), sha in zip(cases.items(), golden["filter_sha256"]):
        rows = E.filter_rows(a)
        assert hashlib.sha256(rows).hexdigest() == str(sha), name  # Pillow's rows, as recorded
        chosen |= set(np.frombuffer(rows, np.uint8).reshape(a.shape[0], -1)[:, 0].tolist())
    assert chosen == {0, 1, 2, 4}  # every candidate wins somewhere; Average never
    pytest.importorskip("PIL.Image")
    for name, a in cases.items():
        assert E.filter_rows(a) == E.pillow_rows(a), name


def test_a_tie_between_sub_and_up_goes_to_up():
    # the second row differs from the first as much as from its own left neighbours: Sub, Up and Paeth score 40 alike, None 100
    a = np.array([[0, 10, 20, 30], [10, 20, 30, 40]], np.uint8)[:, :, None]
    rows = np.frombuffer(E.filter_rows(a), np.uint8).reshape(2, 5)
    assert rows[1].tolist() == [2, 10, 10, 10, 10]
    pytest.importorskip("PIL.Image")
    assert E.filter_rows(a) == E.pillow_rows(a)


# ---- stage 2: the core on the host ----
def test_the_corpus_is_what_it_says():
    c = E.corpus()
    for n in (0, 1, 32767, 32768, 32769, 2 * 32768 + 1):
        assert any(len(v) == n for v in c.values()), n
    assert len(set(c["permutation_200"])) == 200 and sorted(np.bincount(np.frombuffer(c["fibonacci_28656"], np.uint8))[::11].tolist())[-1] == 10946
    assert c["period_300"][:300] == c["period_300"][300:600] and c["far_repeat"][:8] == c["far_repeat"][-8:] and len(c["far_repeat"]) == 32768


def test_core_under_asan_and_ubsan_round_trips_and_keeps_the_stored_bound(host):
    for name, (data, z) in host.items():
        assert zlib.decompress(z) == data, name  # (zlib checks the Adler-32 and refuses a bad code-length set)
        assert len(z) <= E.stored_bound(len(data)), name
        assert z[:2] == b"\x78\x9c", name
    n = lambda name: len(host[name][1])
    assert n("noise_32768") == 32768 + 5 + 6 and n("noise_40000") == 40000 + 5 + 10 + 6  # stored blocks, a marker between two chunks
    assert n("zeros_32768") < 64 and n("zeros_65537") < 128 and n("far_repeat") < 96 and n("period_300") < 480
    assert n("empty") == 8 and n("one_byte") == 9


def test_the_streams_use_what_the_corpus_is_there_for(host):
    """The census of tests/png_ref.py's inflate: which block types, lengths and distances the streams hold."""
    import png_ref as P

    def census(name):
        data, z = host[name]
        out, c = P.inflate(z)
        assert out == data, name
        return c

    c = census("zeros_32768")  # one literal, then 258-byte matches at distance 1 and nothing else: one distance code
    assert c["largest_distance"] == 1 and c["longest_match"] == 258 and c["run258"] >= 126 and c["blocks"][0] == 0
    c = census("zeros_65537")  # three chunks: two markers
    assert c["empty_stored"] == 2 and sum(c["blocks"].values()) == 5
    c = census("permutation_200")  # no match: no distance code at all (or the stored form)
    assert c["huffman_only"] and c["longest_match"] == 0
    c = census("noise_32768")
    assert c["blocks"] == {0: 1, 1: 0, 2: 0}
    c = census("noise_40000")
    assert c["blocks"] == {0: 3, 1: 0, 2: 0} and c["empty_stored"] == 1
    c = census("fibonacci_28656")  # a deep code (the limit of 15 itself: the program's checks of the length builder)
    assert c["blocks"][2] == 1 and 12 <= c["longest_code"] <= 15
    c = census("period_300")  # a repeat of 10700 bytes at distance 300, in pieces of at most 258
    assert c["largest_distance"] == 300 and c["longest_match"] == 258 and c["blocks"][2] == 1
    c = census("far_repeat")
    assert c["largest_distance"] == 32760 and c["longest_match"] == 258
    assert census("empty")["blocks"] == {0: 0, 1: 1, 2: 0} and census("one_byte")["blocks"] == {0: 0, 1: 1, 2: 0}
    c = census("rows_label")  # one block per chunk, a marker between two
    assert census("rows_photo")["blocks"][2] == 4 and c["blocks"][1] + c["blocks"][2] == 9 and c["empty_stored"] == c["blocks"][0] == 8


def test_core_reproduces_the_recording(host, golden):
    names = [str(n) for n in golden["names"]]
    assert names == list(host)
    blob, offsets = golden["blob"].tobytes(), golden["offsets"]
    whole = 0
    for i, name in enumerate(names):
        z = host[name][1]
        assert (len(z), hashlib.sha256(z).hexdigest()) == (int(golden["lengths"][i]), str(golden["sha256"][i])), name
        kept = blob[offsets[i]:offsets[i + 1]]
        assert kept == (z if len(z) <= E.WHOLE else b""), name
        whole += bool(kept)
    assert whole >= 15


def test_file_sizes_against_pillow(host, golden):
    fixtures = E.size_fixtures()
    assert [str(n) for n in golden["size_names"]] == list(fixtures) == ["photo", "smooth", "label", "graphic", "constant", "noise"]
    lines = open(os.path.join(ROOT, "profiles", "png_encode_sizes.txt")).read()
    for i, (name, a) in enumerate(fixtures.items()):
        ours, pillow = len(E.png_file(a, host["rows_" + name][1])), int(golden["size_pillow"][i])
        recorded = int(golden["size_ours"][i]) / pillow
        print(f"{name}: {ours} bytes, Pillow {pillow}, ratio {ours / pillow:.4f} (recorded {recorded:.4f})")
        assert f"{name:10s} ours {int(golden['size_ours'][i]):8d}  Pillow {pillow:8d}  ratio {recorded:.4f}" in lines, name
        if name == "noise":
            assert len(host["rows_noise"][1]) <= E.stored_bound(len(host["rows_noise"][0]))
        else:
            assert ours / pillow <= recorded + SIZE_SLACK, name
    try:
        import PIL
    except ImportError:
        return
    if PIL.__version__ == str(golden["pillow"]):
        assert [len(E.pillow_file(a)) for a in fixtures.values()] == golden["size_pillow"].tolist()


def test_the_file_around_a_stream_is_a_png_any_reader_takes(host):
    Image = pytest.importorskip("PIL.Image")
    for name, a in list(E.gpu_images().items())[:6]:
        f = E.png_file(a, host["rows_" + name][1])
        assert E.idat_payload(f)[1] == ["IHDR", "IDAT", "IEND"]
        image = Image.open(io.BytesIO(f))
        assert image.mode == E.MODE_OF_CHANNELS[a.shape[2]] and image.size == (a.shape[1], a.shape[0])
        assert np.array_equal(np.asarray(image).reshape(a.shape), a), name


# ---- the C ABI and the public surface ----
def test_entry_points_are_declared_prototyped_and_exported(lib):
    import where2edit_amd as W
    from where2edit_amd import _lib, image_io
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
        assert name.endswith("_plan") or params[-1] == "void* stream"
    assert _lib.header_version() == 7 and lib.w2e_version() == 7 and "w2e_png_deflate" in open(os.path.join(ROOT, "include", "w2e.h")).read()
    for name in NAMES:
        assert name in W._IMAGE_IO and getattr(W, name) is getattr(image_io, name)
    for name in ("png_encode.hip", "png_deflate_core.h"):
        assert os.path.exists(os.path.join(ROOT, "where2edit_amd", "csrc", name))
    define = lambda n: int(re.search(r"#define\s+W2E_PNG_" + n + r"\s+(\d+)", header).group(1))
    assert define("CHUNK") == E.CHUNK == 32768 and define("SLOT") == 32780 and define("DEFLATE_LDS") * 2 <= 160 * 1024


def _plan(lib, batch, h, w, channels):
    plan = (ctypes.c_int64 * 8)()
    return lib.w2e_png_encode_plan(batch, h, w, channels, plan), list(plan)


def test_plan_numbers_by_hand(lib):
    per_chunk = 32780 + 4 * 32768 + 16
    # 3 x 5 RGB: rows of 1 + 15 bytes, 48 in all, one chunk; the stored form is 48 + 10 + 6 bytes
    assert _plan(lib, 1, 3, 5, 3) == (0, [16, 48, 48, 1, 32780, per_chunk, 64, 64])
    # 3 x 5 grey: rows of 6 bytes, 18 in all, 20 with the pitch's padding; 34 bytes at most, 36 with the pitch's
    assert _plan(lib, 7, 3, 5, 1) == (0, [6, 18, 20, 1, 32780, 7 * per_chunk, 34, 36])
    assert _plan(lib, 1, 3, 5, 2)[1][:3] == [11, 33, 36] and _plan(lib, 1, 3, 5, 4)[1][:3] == [21, 63, 64]
    # the workloads: a 1024 x 1024 RGB canvas is 1024 * 3073 bytes in 97 chunks; a 512 x 512 label 512 * 513 in 9
    assert _plan(lib, 8, 1024, 1024, 3)[1] == [3073, 1024 * 3073, 1024 * 3073, 97, 32780, 8 * 97 * per_chunk, 1024 * 3073 + 970 + 6, 1024 * 3073 + 976]
    assert _plan(lib, 90, 512, 512, 1)[1][:4] == [513, 512 * 513, 512 * 513, 9]
    # the chunk edges of the GPU test: 32767 and 32768 bytes are one chunk, 32769 are two
    assert [_plan(lib, 1, h, w, c)[1][1:4:2] for h, w, c in ((217, 150, 1), (217, 50, 3), (256, 127, 1), (99, 330, 1))] == [
        [32767, 1], [32767, 1], [32768, 1], [32769, 2]]
    assert _plan(lib, 1, 16384, 16384, 4)[1][1] == 16384 * 65537
    plan = (ctypes.c_int64 * 4)()
    assert lib.w2e_png_deflate_plan(3, 0, plan) == 0 and list(plan) == [1, 32780, 3 * per_chunk, 16]
    assert lib.w2e_png_deflate_plan(1, 2 * 32768 + 1, plan) == 0 and list(plan) == [3, 32780, 3 * per_chunk, 65537 + 36]
    for n in (0, 1, 32768, 32769, 100000):
        assert lib.w2e_png_deflate_plan(1, n, plan) == 0 and plan[3] == E.stored_bound(n)
    from where2edit_amd.image_io import png_encode_plan
    assert png_encode_plan(2, 3, 5, 3) == {"row_bytes": 16, "size": 48, "pitch": 48, "chunks": 1, "slot": 32780, "workspace": 2 * per_chunk, "stream": 64,
                                          "out_pitch": 64}


def test_argument_validation_needs_no_gpu(lib, tmp_path):
    p = ctypes.c_void_p(64)
    err = lib.w2e_last_error
    plan = (ctypes.c_int64 * 8)()

    def planned(batch=1, h=8, w=8, channels=3, out=plan):
        return lib.w2e_png_encode_plan(batch, h, w, channels, out)

    assert planned() == 0 and planned(batch=0) == 0 and planned(batch=65535) == 0
    assert planned(out=None) != 0 and b"null" in err()
    assert planned(batch=-1) != 0 and planned(batch=65536) != 0 and b"batch" in err()
    assert planned(h=0) != 0 and planned(w=16385) != 0 and b"1..16384" in err()
    assert planned(channels=0) != 0 and planned(channels=5) != 0 and b"channels" in err()
    assert lib.w2e_png_deflate_plan(1, -1, plan) != 0 and lib.w2e_png_deflate_plan(1, 1 << 31, plan) != 0 and b"max_size" in err()
    assert lib.w2e_png_deflate_plan(1, 8, None) != 0 and b"null" in err()

    def filt(x=p, batch=1, h=8, w=8, channels=3, raw=p, pitch=8 * 25):
        return lib.w2e_png_filter(x, batch, h, w, channels, raw, pitch, None)

    assert filt(x=None) != 0 and filt(raw=None) != 0 and b"null" in err()
    assert filt(batch=-1) != 0 and filt(h=0) != 0 and filt(w=16385) != 0 and filt(channels=5) != 0 and b"channels" in err()
    assert filt(pitch=8 * 25 - 1) != 0 and b"raw_pitch" in err()
    assert filt(batch=0) == 0  # an empty batch: nothing to launch

    work = 2 * (32780 + 4 * 32768 + 16)

    def deflate(raw=p, pitch=40000, sizes=p, batch=1, max_size=40000, out=p, out_pitch=40028, lengths=p, workspace=p, work_bytes=work):
        return lib.w2e_png_deflate(raw, pitch, sizes, batch, max_size, out, out_pitch, lengths, workspace, work_bytes, None)

    for name in ("raw", "sizes", "out", "lengths", "workspace"):
        assert deflate(**{name: None}) != 0 and b"null" in err(), name
    assert deflate(batch=-1) != 0 and deflate(batch=65536) != 0 and b"batch" in err()
    assert deflate(max_size=-1) != 0 and b"max_size" in err()
    assert deflate(pitch=39996) != 0 and deflate(pitch=40002) != 0 and b"raw_pitch" in err()
    assert deflate(out_pitch=40024) != 0 and deflate(out_pitch=40030) != 0 and b"out_pitch" in err()  # 40000 + 2 * 10 + 6 = 40026
    assert deflate(work_bytes=work - 1) != 0 and b"workspace" in err()
    for name, bad in (("raw", 66), ("out", 65), ("sizes", 68), ("lengths", 68), ("workspace", 68)):
        assert deflate(**{name: ctypes.c_void_p(bad)}) != 0 and b"aligned" in err(), name
    assert deflate(batch=0, work_bytes=0) == 0

    import torch
    from where2edit_amd import image_io as I
    u8 = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    for fn in (I.to_png, I.png_filter):
        with pytest.raises(RuntimeError, match="must be on the GPU"):
            fn(u8)
        with pytest.raises(RuntimeError, match="must be torch.uint8"):
            fn(u8.float())
        with pytest.raises(RuntimeError, match="3 or 4 dimensions"):
            fn(u8[0, 0])
        with pytest.raises(RuntimeError, match="3 or 4 dimensions"):
            fn(u8[None])
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        I.save_png(torch.zeros(1, 3, 8, 8), str(tmp_path / "a.png"))
    with pytest.raises(ValueError, match=r"\.png"):
        I.save_png(torch.zeros(1, 3, 8, 8), str(tmp_path / "a.jpg"))
    with pytest.raises(ValueError, match="write"):
        I.save_png(torch.zeros(1, 3, 8, 8), 3)
    with pytest.raises(ValueError, match="PNG"):  # save_image is as it was
        I.save_image(torch.zeros(1, 3, 8, 8), str(tmp_path / "a.png"))
    with pytest.raises(ValueError, match="list of buffers"):
        I.png_deflate(b"abc")
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        I.png_deflate([torch.zeros(4, dtype=torch.uint8)])
    with pytest.raises(RuntimeError, match="uint8 tensor of one dimension"):
        I.png_deflate([torch.zeros((2, 2), dtype=torch.uint8)])
    assert "save_png" in I.save_image.__doc__ and "save_png" in open(os.path.join(ROOT, "README.md")).read()
