"""The JPEG decoder on the GPU (where2edit_amd/image_io.py, csrc/jpeg_decode.hip) against the numpy restatement of
tests/jpeg_decode_ref.py, which tests/test_jpeg_decode_host.py holds against Pillow, and against the recorded digests of Pillow's own
pixels (tests/golden/jpeg_decode.npz): exact equality everywhere -- entry states, coefficients, pixels.

Files: everything tests/jpeg_ref.py's encoder writes for jpeg_ref.cases() (4:2:0, the Annex K tables; the sizes of
tests/test_gpu_jpeg.py, which are also the ones at which partial MCUs, odd chroma planes and a long MCU row go wrong) and for the
256 x 256 photograph; and the recorded Pillow files: 4:4:4, grey, optimised Huffman tables, qualities 95 and 100, up to 40 x 56."""
import functools
import hashlib
import io
import os

import numpy as np
import pytest
import torch

import jpeg_decode_ref as D
import jpeg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = R.ALL_SIZES + (D.PHOTO_SIZE,)


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_decode.npz"))
    blob, offsets = g["pil_blob"].tobytes(), g["pil_offsets"]
    files = {str(k): blob[offsets[i]:offsets[i + 1]] for i, k in enumerate(g["pil_keys"])}
    sha = dict(zip((str(k) for k in g["enc_keys"]), (str(s) for s in g["enc_sha256"])))
    sha.update(zip((str(k) for k in g["pil_keys"]), (str(s) for s in g["pil_sha256"])))
    return files, sha


@functools.lru_cache(maxsize=None)
def _cases():
    """{key: (h, w, make)}: every file of the case list."""
    files, _ = _golden()
    out = {key: (h, w, make) for key, h, w, make in D.encode_cases()}
    out.update({c[0]: (c[1], c[2], functools.partial(files.__getitem__, c[0])) for c in D.pillow_cases()})
    assert set(files) <= set(out)
    return out


def _keys(size):
    return [k for k, (h, w, _) in _cases().items() if (h, w) == tuple(size)]


@functools.lru_cache(maxsize=None)
def _ref(key):
    """(the file, its parse, the restatement's coefficients, its pixels): computed once, shared by the tests below, read-only."""
    data = _cases()[key][2]()
    parsed = D.parse(data)
    coef, status = D.coefficients(parsed)
    assert status == 0
    pixels = D.pixels(coef, parsed["q"], parsed["h"], parsed["w"], parsed["sampling"])
    coef.setflags(write=False), pixels.setflags(write=False)
    return data, parsed, coef, pixels


def _cut_in_half(data):
    """The file with the second half of its scan gone (the end marker kept): what a download that broke off looks like."""
    start = data.index(b"\xff\xda")
    start += 2 + int.from_bytes(data[start + 2:start + 4], "big")
    scan = data[start:-2]
    half = scan[:len(scan) // 2]
    return data[:start] + (half[:-1] if half.endswith(b"\xff") else half) + b"\xff\xd9"


STATE_STREAMS = ("enc_70x38_mixed_q75", "enc_48x40_checker_q100", "enc_264x520_constant_q75", "enc_264x520_random_q75", "enc_1x1_mixed_q75",
                 "enc_2054x30_mixed_q75", "pil_444opt95_40x56_random", "pil_grey_17x23_mixed", "pil_420opt_33x16_colour_checker")


@pytest.mark.parametrize("sub_bits", D.SUB_BITS)
def test_entry_states_equal_the_sequential_decoder(sub_bits):
    """32 bits: blocks that span a dozen subsequences (the checkerboard at quality 100), and the constant 264 x 520 image, which parses
    consistently at a wrong MCU phase -- its rounds equal its subsequences, more than one workgroup holds them and more than one
    launch is needed.  1024 bits: streams shorter than one subsequence."""
    from where2edit_amd.image_io import jpeg_decode_plan, jpeg_decode_states
    for key in STATE_STREAMS:
        data, parsed, _, _ = _ref(key)
        stream = D.Stream(parsed)
        want = D.sequential_states(stream, sub_bits)
        got, launches = jpeg_decode_states(data, sub_bits)
        assert got.dtype == torch.int32 and tuple(got.shape) == want.shape == (stream.subsequences(sub_bits), 3)
        bad = np.argwhere((got.numpy() != want).any(axis=1))
        assert len(bad) == 0, f"{key}: {len(bad)} of {len(want)} entry states differ, the first at subsequence {int(bad[0])}"
        plan = jpeg_decode_plan(1, parsed["h"], parsed["w"], parsed["sampling"], stream.bits, sub_bits)
        assert plan["subsequences"] == len(want) and plan["launches"] == -(-len(want) // D.GROUP) + 1
        assert 1 <= launches <= plan["launches"], key
        assert launches == D.relax_two_level(stream, sub_bits)[1], key  # (the hand-over between workgroups is by launch: nothing to race)
        if key == "enc_264x520_constant_q75" and sub_bits == 32:
            assert len(want) > 2 * D.GROUP and launches > 1
        if key == "enc_48x40_checker_q100" and sub_bits == 32:
            assert stream.bits > 6 * sub_bits * stream.blocks  # the Y blocks span a dozen subsequences each, the chroma blocks none
        if sub_bits == 1024 and key in ("enc_1x1_mixed_q75", "pil_grey_17x23_mixed"):
            assert len(want) == 1 and launches == 1


def test_states_of_a_batch_of_different_lengths():
    from where2edit_amd.image_io import jpeg_decode_states
    keys = ("enc_40x56_random_q75", "enc_40x56_constant_q75", "enc_40x56_mixed_q75")
    files = [_ref(k)[0] for k in keys]
    assert len({len(f) for f in files}) == 3
    for sub_bits in (32, 128):
        got, launches = jpeg_decode_states(files, sub_bits)
        assert isinstance(got, list) and len(got) == 3
        for k, g in zip(keys, got):
            assert np.array_equal(g.numpy(), D.sequential_states(D.Stream(_ref(k)[1]), sub_bits)), (k, sub_bits)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decoded_coefficients_equal_the_restatement(size):
    from where2edit_amd.image_io import jpeg_decode_coefficients
    for key in _keys(size):
        data, parsed, want, _ = _ref(key)
        got = jpeg_decode_coefficients(data)
        assert got.dtype == torch.int16 and tuple(got.shape) == want.shape and got.is_contiguous() and got.is_cuda
        bad = np.argwhere(got.cpu().numpy() != want)
        assert len(bad) == 0, f"{key}: {len(bad)} coefficients differ, the first at (block, k) = {tuple(bad[0])}"


def test_decoded_coefficients_are_the_encoders():
    """For a file to_jpeg made, stage 1 of the decoder returns the tensor stage 1 of the encoder wrote."""
    from where2edit_amd.image_io import jpeg_coefficients, jpeg_decode_coefficients, to_jpeg
    for (h, w), name, quality in (((70, 38), "mixed", 75), ((130, 262), "random", 75), ((48, 40), "colour_checker", 100), ((33, 16), "ramp", 30)):
        x = torch.from_numpy(R.pattern(name, h, w, 7)).to(DEV)
        got = jpeg_decode_coefficients(to_jpeg(x, quality))
        assert torch.equal(got, jpeg_coefficients(x, quality)), (h, w, name, quality)
    x = torch.from_numpy(np.stack([R.pattern(n, 40, 56, 20 + i) for i, n in enumerate(("random", "constant", "mixed"))])).to(DEV)
    assert torch.equal(jpeg_decode_coefficients(to_jpeg(x)), jpeg_coefficients(x))


def test_the_result_is_identical_for_every_sub_bits():
    from where2edit_amd.image_io import jpeg_decode_coefficients
    for key in ("enc_70x38_mixed_q75", "enc_48x40_checker_q100", "enc_264x520_constant_q75", "enc_2054x30_random_q75", "pil_444opt95_40x56_random",
                "pil_grey100_40x56_mixed", "enc_1x1_random_q75"):
        data, _, want, _ = _ref(key)
        for sub_bits in (32, 64, 128, 512, 1024, 4096):
            assert np.array_equal(jpeg_decode_coefficients(data, sub_bits).cpu().numpy(), want), (key, sub_bits)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_jpeg_pixels_equal_the_restatement(size):
    """Stage 2 on the restatement's coefficients."""
    from where2edit_amd.image_io import jpeg_pixels
    for key in _keys(size):
        _, parsed, coef, want = _ref(key)
        got = jpeg_pixels(torch.from_numpy(np.array(coef)).to(DEV), torch.from_numpy(parsed["q"]), parsed["h"], parsed["w"], parsed["sampling"])
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous()
        bad = np.argwhere(got.cpu().numpy() != want)
        assert len(bad) == 0, f"{key}: {len(bad)} bytes differ, the first at (y, x, channel) = {tuple(bad[0])}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_from_jpeg_equals_pillows_pixels(size):
    from where2edit_amd.image_io import from_jpeg
    _, sha = _golden()
    for key in _keys(size):
        data, _, _, want = _ref(key)
        got = from_jpeg(data)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (size[0], size[1], 3) and got.is_cuda
        got = got.cpu().numpy()
        assert np.array_equal(got, want), key
        assert hashlib.sha256(got.tobytes()).hexdigest() == sha[key], key


def test_from_jpeg_of_a_batch_of_a_mixed_list_and_stacked():
    from where2edit_amd.image_io import from_jpeg
    keys = ("enc_40x56_random_q75", "enc_40x56_constant_q75", "enc_40x56_mixed_q75")
    files = [_ref(k)[0] for k in keys]
    got = from_jpeg(files)
    assert isinstance(got, list) and len(got) == 3
    for k, g in zip(keys, got):
        assert np.array_equal(g.cpu().numpy(), _ref(k)[3]), k
    stacked = from_jpeg(files, stack=True)
    assert tuple(stacked.shape) == (3, 40, 56, 3) and all(torch.equal(stacked[i], got[i]) for i in range(3))
    # two geometries and one grey file, interleaved; files of one geometry with different tables (quality 75 and 95, optimised)
    mixed = ("enc_40x56_mixed_q75", "pil_grey_40x56_mixed", "enc_17x23_random_q75", "pil_444opt95_40x56_random", "pil_420opt_40x56_random",
             "pil_444_40x56_constant", "enc_17x23_checker_q100")
    got = from_jpeg([_ref(k)[0] for k in mixed])
    for k, g in zip(mixed, got):
        assert np.array_equal(g.cpu().numpy(), _ref(k)[3]), k
    with pytest.raises(ValueError, match="stack=True"):
        from_jpeg([_ref(k)[0] for k in mixed], stack=True)
    assert from_jpeg([]) == []


def test_round_trip_to_tensor_and_load_image(tmp_path):
    from where2edit_amd.image_io import from_jpeg, load_image, save_image, to_jpeg, to_tensor
    x = torch.from_numpy(R.pattern("mixed", 70, 38, 3)).to(DEV)
    data = to_jpeg(x)
    got = from_jpeg(data)
    assert np.array_equal(got.cpu().numpy(), D.decode(data))
    # the input side of the reference: file -> normalised tensor at the mask's size, against the same kernel on the uploaded pixels
    key = "enc_70x38_mixed_q75"
    pixels = torch.from_numpy(np.array(_ref(key)[3])).to(DEV)
    assert torch.equal(to_tensor(from_jpeg([_ref(key)[0]], stack=True), 16), to_tensor(pixels[None], 16))
    path = tmp_path / "a.jpg"
    save_image(torch.rand(2, 3, 24, 40, device=DEV) * 2 - 1, str(path))
    want = D.decode(path.read_bytes())
    assert np.array_equal(load_image(str(path)).cpu().numpy(), want)
    assert np.array_equal(load_image(io.BytesIO(path.read_bytes())).cpu().numpy(), want)


def test_the_same_call_gives_the_same_tensors():
    from where2edit_amd import _lib
    from where2edit_amd.image_io import from_jpeg, jpeg_decode_coefficients
    data = _ref("enc_264x520_mixed_q75")[0]
    first, coef = from_jpeg(data), jpeg_decode_coefficients(data, 128)
    assert torch.equal(from_jpeg(data), first) and torch.equal(jpeg_decode_coefficients(data, 128), coef)
    before = _lib.get_option("deterministic")
    _lib.set_option("deterministic", 1)
    try:
        assert torch.equal(from_jpeg(data), first) and torch.equal(jpeg_decode_coefficients(data, 128), coef)
    finally:
        _lib.set_option("deterministic", before)


def test_a_scan_cut_in_half_is_an_error_not_a_fault():
    """An input every decoder meets.  The kernels clamp every read to the scan and bound every loop, so the file gives a nonzero status
    (the restatement's own) and a ValueError; the file next to it in the batch is still named as the good one."""
    from where2edit_amd import image_io as I
    good = _ref("enc_40x56_mixed_q75")[0]
    cut = _cut_in_half(good)
    _, want = D.coefficients(D.parse(cut))
    assert want & D.STATUS_COUNT
    with torch.cuda.device(0):
        batch = I._JpegBatch([I.jpeg_parse(good), I.jpeg_parse(cut)], torch.device("cuda", 0), 128)
        batch.relax()
        _, status = batch.coefficients()
    assert status.tolist() == [0, want]
    with pytest.raises(ValueError, match=r"image 1 has a corrupt scan.*number of blocks"):
        I.from_jpeg([good, cut])
    with pytest.raises(ValueError, match="corrupt scan"):
        I.jpeg_decode_coefficients(cut)
    assert np.array_equal(I.from_jpeg(good).cpu().numpy(), _ref("enc_40x56_mixed_q75")[3])  # and the next call is untouched
