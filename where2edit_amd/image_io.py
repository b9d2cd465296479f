"""Image I/O on the device, with the reference's own pixel values: bytes in, bytes out (include/w2e_image.h, csrc/image.hip).

In.  Every real-image path of the reference begins with a PIL image that goes through `transforms.Resize((s, s))`, `ToTensor` and
`Normalize` (show_demo/try_demo.py:96-99; utils.py:594-619 transform_img / transform_label; utils.py:654-726 over CelebAMaskHQ).
`Resize` on a PIL image is Pillow's 8-bit `Image.resize(BILINEAR)`: an antialiased triangle filter whose window grows with the
down-scaling factor, integer coefficients in 2^-22 units, a byte between the horizontal and the vertical pass.  `resample_tables`
restates the coefficients (Python floats, in Pillow's operation order), `resize_u8` / `to_tensor` / `label_ids` run the two passes as
one kernel; ToTensor + Normalize is a 256-entry table per channel that the device only looks values up in.

Out.  Every path of the reference that emits an image ends in `torchvision.utils.save_image(..., normalize=True, range=(-1, 1))`
(mapper/scripts/inference.py:70-77, utils.py:493-503, coach.py:264).  `to_bytes` is that call up to the bytes it hands to the PNG
encoder: torchvision 0.8.2's make_grid normalisation and layout, then mul(255).add_(0.5).clamp_(0, 255).to(uint8), as one kernel.

Every file the reference writes is a `.jpg`: torchvision ends `save_image` in `Image.fromarray(ndarr).save(fp)`, Pillow's default JPEG
(libjpeg: quality 75, 4:2:0, the Annex K Huffman tables, no optimisation).  `to_jpeg` is that encoder on the device, in integers from
end to end, so the file is Pillow's byte for byte (include/w2e_jpeg.h, csrc/jpeg.hip; DESIGN.md "K17b"): colour conversion,
down-sampling, DCT, quantisation and Huffman coding are kernels; the header, byte stuffing and the end marker are host work on the
coded segment, which is what crosses to the host (a few per cent of the pixels).  `save_image` is `to_bytes` + `to_jpeg` + the file.

Files in.  Every real-image path of the reference starts with `Image.open(path)` on a JPEG (show_demo/try_demo.py:96-99; the
CelebAMask-HQ images, utils.py:573-587).  `from_jpeg` / `load_image` decode a baseline file on the device to Pillow's own pixels
(csrc/jpeg_decode.hip; DESIGN.md "K17c"): the host walks the markers (`jpeg_parse`), only the coded file crosses to the device, the
Huffman stream is decoded in parallel by self-synchronisation, then inverse DCT, chroma up-sampling and colour conversion.

PNG files in.  The other files the reference reads are PNGs: the CelebAMask-HQ parsing labels (`Image.open(str(i) + '.png')`,
utils.py:573-587) and the demo's portraits (show_demo/try_demo.py:66-68, 96-97).  `from_png` / `load_png` decode a non-interlaced 8-bit
(palette: 1 to 8 bits) file on the device to Pillow's own pixels, `mode="RGB"` for `convert("RGB")` and `mode="raw"` for the ids of a
label (csrc/png.hip, csrc/png_core.h; DESIGN.md "K17d"): the host walks the chunks and verifies their CRCs (`png_parse`), only the
compressed stream and the palette cross to the device, one wave inflates each stream of a batch, then the row filters are undone.
`read_image` takes either kind of file.  `save_image` writes JPEG only, as the reference does.

PNG files out.  `to_png` / `save_png` are the lossless way out: torchvision's `save_image(x, "name.png")` ends in Pillow's PNG encoder,
and `to_png` is that encoder on the device up to the compressed bytes (csrc/png_encode.hip, csrc/png_deflate_core.h; DESIGN.md
"K17e").  The filtered rows are Pillow's byte for byte (`png_filter`: its choice among None, Sub, Up and Paeth for every row); the
deflate stream is the library's own (`png_deflate`: independent 32 KiB chunks, one workgroup each, joined as zlib's sync flush joins
them), so any reader gets the pixels back exactly and only the compressed data crosses to the host.

GPU only: there is no CPU fallback (tests/imageio_ref.py, tests/jpeg_ref.py, tests/jpeg_decode_ref.py,
tests/png_ref.py and tests/png_encode_ref.py are the numpy restatements the kernels are tested against)."""
import ctypes
import functools
import math
import os
import re
import zlib

import numpy as np
import torch

from ._lib import CONSTS, call, stream_ptr

PRECISION_BITS = CONSTS["W2E_IMAGE_PRECISION_BITS"]
FILTERS = ("bilinear", "nearest")


def _axis_tables(in_size, out_size, filter):
    """Pillow Resample.c precompute_coeffs + normalize_coeffs_8bpc for one axis, as lists: (K [out][ksize], bounds [out][2])."""
    one = 1 << PRECISION_BITS
    scale = in_size / out_size
    if filter == "nearest":
        return [[one] for _ in range(out_size)], [[min(int((xx + 0.5) * scale), in_size - 1), 1] for xx in range(out_size)]
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    coeffs, bounds = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = []
        ww = 0.0
        for x in range(n):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        row = [0] * ksize
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            row[x] = int(-0.5 + k * one) if k < 0 else int(0.5 + k * one)
        coeffs.append(row)
        bounds.append([xmin, n])
    return coeffs, bounds


@functools.lru_cache(maxsize=None)
def _host_tables(in_size, out_size, filter):
    k, b = _axis_tables(in_size, out_size, filter)
    return torch.tensor(k, dtype=torch.int32), torch.tensor(b, dtype=torch.int32)


def _check_size(what, v):
    if not (isinstance(v, int) and 1 <= v <= 16384):
        raise ValueError(f"{what}: sizes are integers in 1..16384 (got {v!r})")


def resample_tables(in_size, out_size, filter="bilinear"):
    """The integer coefficients of one axis of Pillow's `Image.resize`, `in_size` -> `out_size` samples: int32 CPU tensors
    (K [out, ksize], bounds [out, 2]) with bounds[o] = (first input index of output o's window, its length n) and K[o, :n] the
    window's coefficients in 2^-22 units (zero beyond n).  Per axis, in float64 and in this order: scale = in / out,
    fs = max(scale, 1), support = fs, ksize = 2 ceil(support) + 1; for output o, center = (o + 0.5) scale,
    first = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), in) - first, w[x] = tri((x + first - center + 0.5)
    / fs), K = int(0.5 + w / sum(w) * 2^22).  filter="nearest": one tap of 2^22 at min(int((o + 0.5) scale), in - 1).
    The result is cached: treat it as read-only."""
    _check_size("resample_tables", in_size), _check_size("resample_tables", out_size)
    if filter not in FILTERS:
        raise ValueError(f"resample_tables: filter must be one of {FILTERS} (got {filter!r}); bicubic and Lanczos are not implemented")
    return _host_tables(in_size, out_size, filter)


_DEVICE_TABLES = {}  # (in, out, filter, device) -> (K, bounds) on that device
_NORM_TABLES = {}    # (mean, std, channels, device) -> [channels, 256] fp32 on that device


def _device_tables(in_size, out_size, filter, device):
    key = (in_size, out_size, filter, device)
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        k, b = resample_tables(in_size, out_size, filter)
        hit = _DEVICE_TABLES[key] = (k.to(device), b.to(device))
    return hit


def _per_channel(what, v, channels):
    v = tuple(float(x) for x in v) if isinstance(v, (tuple, list)) else (float(v),) * channels
    if len(v) != channels:
        raise ValueError(f"to_tensor: {what} has {len(v)} entries for {channels} channels")
    return v


def normalize_table(mean, std, channels):
    """ToTensor + Normalize(mean, std) as a table: fp32 CPU [channels, 256], lut[c, v] = float32((float32(v) / 255 - mean[c]) / std[c])
    -- the same torch operations, in the same order and precision, that the two transforms apply to a pixel."""
    mean, std = _per_channel("mean", mean, channels), _per_channel("std", std, channels)
    if any(s == 0 for s in std):
        raise ValueError("to_tensor: std has a zero entry")
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)  # ToTensor
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return v[None, :].repeat(channels, 1).sub_(m[:, None]).div_(s[:, None])  # Normalize


def _norm_table(mean, std, channels, device):
    key = (_per_channel("mean", mean, channels), _per_channel("std", std, channels), channels, device)
    hit = _NORM_TABLES.get(key)
    if hit is None:
        hit = _NORM_TABLES[key] = normalize_table(mean, std, channels).to(device)
    return hit


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr() if t.numel() else 16)


def _on_gpu(who, what, x, dtype, ranks):
    if not torch.is_tensor(x):
        raise RuntimeError(f"{who}: {what} must be a tensor (got {type(x).__name__})")
    if x.dtype != dtype:
        raise RuntimeError(f"{who}: {what} must be {dtype} (got {x.dtype})")
    if x.ndim not in ranks:
        raise RuntimeError(f"{who}: {what} must have {' or '.join(str(r) for r in ranks)} dimensions (got shape {tuple(x.shape)})")
    if not x.is_cuda:
        raise RuntimeError(f"{who}: {what} must be on the GPU (got {x.device}): move it with .to('cuda') first -- there is no CPU path")


def _size2(who, size):
    if isinstance(size, int):
        size = (size, size)
    size = tuple(size)
    if len(size) != 2:
        raise ValueError(f"{who}: size is an integer or (height, width) (got {size!r})")
    _check_size(who, size[0]), _check_size(who, size[1])
    return size


def resize_plan(batch, channels, in_h, in_w, out_h, out_w):
    """w2e_image_resize_plan as a dict: form (0 fused / 1 two launches), workspace bytes, the bilinear ksize per axis, the fused
    tile and its LDS.  Pure host."""
    plan = (ctypes.c_int64 * 8)()
    call("w2e_image_resize_plan", batch, channels, in_h, in_w, out_h, out_w, plan)
    return {"form": plan[0], "workspace": plan[1], "ksize_x": plan[2], "ksize_y": plan[3], "tile": (plan[4], plan[5]), "lds": plan[6]}


def _resize(who, x, size, filter, lut):
    """x uint8 [B,H,W,C] contiguous on the GPU -> uint8 [B,oh,ow,C] (lut None) or fp32 [B,C,oh,ow] through lut [C,256]."""
    if filter not in FILTERS:
        raise ValueError(f"{who}: filter must be one of {FILTERS} (got {filter!r})")
    b, h, w, c = x.shape
    if c not in (1, 3):
        raise RuntimeError(f"{who}: images are [B,H,W,C] with C = 1 or 3, channels last (got shape {tuple(x.shape)})")
    oh, ow = size
    _check_size(who, h), _check_size(who, w)
    if not x.is_contiguous():
        x = x.contiguous()
    with torch.cuda.device(x.device):
        dev = x.device
        kx, bx = _device_tables(w, ow, filter, dev) if w != ow else (None, None)
        ky, by = _device_tables(h, oh, filter, dev) if h != oh else (None, None)
        out = torch.empty((b, oh, ow, c), dtype=torch.uint8, device=dev) if lut is None else torch.empty((b, c, oh, ow), dtype=torch.float32, device=dev)
        plan = resize_plan(b, c, h, w, oh, ow)
        work = torch.empty(plan["workspace"], dtype=torch.uint8, device=dev) if plan["workspace"] else None
        call("w2e_image_resize", _p(x), b, c, h, w, oh, ow, _p(kx), _p(bx), kx.shape[1] if kx is not None else 1, _p(ky), _p(by),
             ky.shape[1] if ky is not None else 1, _p(lut), _p(out), _p(work), stream_ptr())
    return out


def resize_u8(x, size, filter="bilinear"):
    """`PIL.Image.resize((ow, oh), BILINEAR | NEAREST)` of every image of a batch: uint8 [B,H,W,C] (C = 1 or 3) or [B,H,W] on the GPU
    -> the same layout at size = (oh, ow) (an integer: square), byte for byte what Pillow returns for modes L and RGB.  One launch
    (two, through a temporary, when the down-scaling is so strong that a tile's input span does not fit in LDS: resize_plan)."""
    _on_gpu("resize_u8", "x", x, torch.uint8, (3, 4))
    size = _size2("resize_u8", size)
    if x.ndim == 3:
        return _resize("resize_u8", x.unsqueeze(-1), size, filter, None).squeeze(-1)
    return _resize("resize_u8", x, size, filter, None)


def to_tensor(x, size=None, mean=0.5, std=0.5):
    """transforms.Compose([Resize(size), ToTensor(), Normalize(mean, std)]) of PIL images: uint8 [B,H,W,C] on the GPU -> fp32
    [B,C,oh,ow].  size None: no resize.  mean / std: a number or one per channel.  to_tensor(x, 256) is the reference's
    transform_img(256, False, True, True, True) (utils.py:594-606), bit for bit."""
    _on_gpu("to_tensor", "x", x, torch.uint8, (4,))
    size = tuple(x.shape[1:3]) if size is None else _size2("to_tensor", size)
    c = x.shape[3]
    if c not in (1, 3):
        raise RuntimeError(f"to_tensor: images are [B,H,W,C] with C = 1 or 3, channels last (got shape {tuple(x.shape)})")
    with torch.cuda.device(x.device):
        lut = _norm_table(mean, std, c, x.device)
    return _resize("to_tensor", x, size, "bilinear", lut)


def label_ids(x, size, filter="bilinear"):
    """Parsing labels at the mask's resolution: uint8 ids [B,H,W] on the GPU -> uint8 [B,oh,ow].  With filter="bilinear" this is the
    reference's transform_label(s, False, True, True, False) followed by (label * 255).type(torch.int) (utils.py:608-619, :702): it
    resizes the mode-L label PNG with Pillow's antialiased bilinear filter, so ids BLEND at region borders and a border pixel carries
    an id that neither neighbour has; `label == k` then keeps only the exact hits.  filter="nearest" keeps ids intact."""
    _on_gpu("label_ids", "x", x, torch.uint8, (3,))
    return resize_u8(x, size, filter)


def grid_shape(batch, h, w, nrow=8, padding=2):
    """(rows, columns) of torchvision 0.8.2 make_grid's canvas for a [batch, *, h, w] tensor."""
    if batch == 1:
        return h, w
    xmaps = min(nrow, batch)
    ymaps = -(-batch // xmaps)
    return ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def to_bytes(x, value_range=(-1, 1), nrow=8, padding=2, pad_value=0.0, grid=True, eps=1e-5):
    """`torchvision.utils.save_image(x, ..., normalize=True, range=value_range, nrow=, padding=, pad_value=)` (0.8.2) up to the bytes
    it hands to PIL: fp32 [B,C,H,W] (C = 1 or 3) on the GPU -> uint8 HWC.  grid=True: make_grid's canvas, [H,W,3] for a batch of one
    (unpadded) and [ymaps (H + padding) + padding, xmaps (W + padding) + padding, 3] otherwise, a 1-channel input replicated to 3
    channels, empty cells and borders at pad_value.  grid=False: [B,H,W,C], each image on its own.
    Per value, every step a separately rounded fp32 operation: t = (clamp(x, lo, hi) - lo) / float32(hi - lo + eps),
    byte = trunc(clamp(t * 255 + 0.5, 0, 255)); NaN -> 0.  One launch, 4 B read and 1 B written per value."""
    _on_gpu("to_bytes", "x", x, torch.float32, (4,))
    lo, hi = float(value_range[0]), float(value_range[1])
    if not lo < hi:
        raise ValueError(f"to_bytes: value_range must be (lo, hi) with lo < hi (got {value_range!r})")
    b, c, h, w = x.shape
    if c not in (1, 3):
        raise RuntimeError(f"to_bytes: images are [B,C,H,W] with C = 1 or 3 (got shape {tuple(x.shape)})")
    _check_size("to_bytes", h), _check_size("to_bytes", w)
    if not (isinstance(nrow, int) and nrow >= 1 and isinstance(padding, int) and 0 <= padding <= 1024):
        raise ValueError(f"to_bytes: nrow >= 1 and 0 <= padding <= 1024 (got {nrow!r}, {padding!r})")
    if not x.is_contiguous():
        x = x.contiguous()
    divisor = ctypes.c_float(hi - lo + eps).value  # the sum in double, rounded once
    with torch.cuda.device(x.device):
        if grid:
            rows, cols = grid_shape(b, h, w, nrow, padding) if b else (0, 0)
            out = torch.empty((rows, cols, 3), dtype=torch.uint8, device=x.device)
        else:
            out = torch.empty((b, h, w, c), dtype=torch.uint8, device=x.device)
        call("w2e_image_quantize", _p(x), b, c, h, w, lo, hi, divisor, nrow, padding, float(pad_value), 1 if grid else 0, _p(out), stream_ptr())
    return out


# ---- JPEG (include/w2e_jpeg.h) ----
# Annex K of the JPEG standard: the quantisation base tables in natural order, and the four Huffman tables as (class << 4 | id,
# codes per length 1..16, symbols in code order), in the order the header writes them and the device table holds them.
_JPEG_LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_JPEG_CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_JPEG_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_JPEG_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6"
    "c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
_JPEG_HUFFMAN = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D), _JPEG_AC_LUMA),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), _JPEG_AC_CHROMA),
)
# _JPEG_ZIGZAG[k]: the natural (row-major) index of the k-th coefficient of the zigzag scan
_JPEG_ZIGZAG = tuple(sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8)))
_JPEG_ZIGZAG_POS = tuple(_JPEG_ZIGZAG.index(i) for i in range(64))  # the inverse: the zigzag position of natural index i
_JPEG_GUESS_DIVISOR = 2  # to_jpeg's first copy takes h * w / 2 bytes per image: 4 bits per pixel, several times a photograph's rate
_HUFF_TABLES = {}        # device -> uint32 [4, 256]


def _check_quality(who, quality):
    if not (isinstance(quality, int) and not isinstance(quality, bool) and 1 <= quality <= 100):
        raise ValueError(f"{who}: quality is an integer in 1..100 (got {quality!r})")


@functools.lru_cache(maxsize=None)
def _jpeg_tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(torch.tensor([min(max((v * scale + 50) // 100, 1), 255) for v in base], dtype=torch.int32) for base in (_JPEG_LUMA_Q, _JPEG_CHROMA_Q))


def jpeg_tables(quality=75):
    """The two quantisation tables of a quality in 1..100: int32 CPU tensors (luminance [64], chrominance [64]) in natural (row-major)
    order.  The Annex K base tables scaled as libjpeg's jpeg_set_quality does with baseline forced: scale = 5000 // q below 50,
    200 - 2 q from there; entry = clamp((base * scale + 50) // 100, 1, 255).  The result is cached: treat it as read-only."""
    _check_quality("jpeg_tables", quality)
    return _jpeg_tables(quality)


def _jpeg_segment(marker, payload):
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def jpeg_header(h, w, quality=75):
    """The bytes of the file from SOI through SOS, as Pillow writes them for an h x w RGB image: APP0 (JFIF 1.1, density 1 x 1, no
    unit), one DQT per table (8-bit, zigzag order), SOF0 (Y 2x2 on table 0, Cb and Cr 1x1 on table 1), four DHT (DC0, AC0, DC1, AC1: the
    Annex K tables), SOS."""
    _check_size("jpeg_header", h), _check_size("jpeg_header", w)
    luma, chroma = (t.tolist() for t in jpeg_tables(quality))
    out = b"\xff\xd8" + _jpeg_segment(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
    out += _jpeg_segment(0xDB, bytes([0] + [luma[i] for i in _JPEG_ZIGZAG])) + _jpeg_segment(0xDB, bytes([1] + [chroma[i] for i in _JPEG_ZIGZAG]))
    out += _jpeg_segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes((3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for ident, counts, symbols in _JPEG_HUFFMAN:
        out += _jpeg_segment(0xC4, bytes([ident]) + bytes(counts) + symbols)
    return out + _jpeg_segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def jpeg_code_table():
    """The device's view of the four Huffman tables: uint32 CPU [4, 256] in the order DC0, AC0, DC1, AC1, entry [symbol] =
    (code << 5) | length, 0 for a symbol the table does not have.  Codes are assigned as Annex C says: in order of length, counting
    up, shifted left at each new length."""
    table = torch.zeros((4, 256), dtype=torch.int64)
    for t, (_, counts, symbols) in enumerate(_JPEG_HUFFMAN):
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                table[t, symbols[k]] = (code << 5) | length
                code, k = code + 1, k + 1
            code <<= 1
    return table.to(torch.int32)  # (every entry is below 2^21)


def _huff_table(device):
    hit = _HUFF_TABLES.get(device)
    if hit is None:
        hit = _HUFF_TABLES[device] = jpeg_code_table().to(device)
    return hit


def jpeg_plan(batch, h, w):
    """w2e_jpeg_plan as a dict: blocks per image, the MCU grid, the entropy stage's workspace bytes, the largest possible segment of
    an image in bytes, the coefficient elements per image, stage 1's workgroups and the prefix sum's tile.  Pure host."""
    plan = (ctypes.c_int64 * 8)()
    call("w2e_jpeg_plan", batch, h, w, plan)
    return {"blocks": plan[0], "mcus": (plan[2], plan[1]), "workspace": plan[3], "segment": plan[4], "coefficients": plan[5],
            "strips": plan[6], "scan_tile": plan[7]}


def _jpeg_input(who, x, quality):
    _on_gpu(who, "x", x, torch.uint8, (3, 4))
    if x.shape[-1] != 3:
        raise RuntimeError(f"{who}: images are [H,W,3] or [B,H,W,3], RGB, channels last (got shape {tuple(x.shape)})")
    _check_quality(who, quality)
    x4 = x.unsqueeze(0) if x.ndim == 3 else x
    _check_size(who, x4.shape[1]), _check_size(who, x4.shape[2])
    return x4 if x4.is_contiguous() else x4.contiguous()


def _jpeg_coefficients(x4, quality, plan):
    b, h, w, _ = x4.shape
    coef = torch.empty((b, plan["blocks"], 64), dtype=torch.int16, device=x4.device)
    call("w2e_jpeg_coefficients", _p(x4), b, h, w, quality, _p(coef), stream_ptr())
    return coef


def jpeg_coefficients(x, quality=75):
    """Stage 1 of the encoder on its own (for tests and for finding a fault): uint8 [H,W,3] or [B,H,W,3] on the GPU -> int16
    [blocks, 64] or [B, blocks, 64], the quantised DCT coefficients of every block in zigzag order.  Blocks are in scan order: MCUs
    of 16 x 16 pixels in raster order, Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr inside each; a Y block outside the image (a dummy) has zero
    AC coefficients and the DC of the block before it."""
    x4 = _jpeg_input("jpeg_coefficients", x, quality)
    with torch.cuda.device(x4.device):
        coef = _jpeg_coefficients(x4, quality, jpeg_plan(*x4.shape[:3]))
    return coef[0] if x.ndim == 3 else coef


def to_jpeg(x, quality=75):
    """`Image.fromarray(x).save(fp, format="JPEG", quality=quality)` of images on the GPU, byte for byte: uint8 [H,W,3] -> bytes,
    uint8 [B,H,W,3] -> a list of B bytes.  Four launches for the whole batch; what crosses to the host is the coded data, not the
    pixels, in ONE copy (lengths included) as long as no image codes to more than 4 bits per pixel -- several times the rate of a
    photograph at quality 75; past that (noise at a high quality) a second copy fetches the rest."""
    x4 = _jpeg_input("to_jpeg", x, quality)
    b, h, w, _ = x4.shape
    if b == 0:
        return []
    with torch.cuda.device(x4.device):
        dev = x4.device
        plan = jpeg_plan(b, h, w)
        coef = _jpeg_coefficients(x4, quality, plan)
        cap = plan["segment"]
        out = torch.empty((b, cap), dtype=torch.uint8, device=dev)
        lengths = torch.empty((b,), dtype=torch.int64, device=dev)
        work = torch.empty((plan["workspace"],), dtype=torch.uint8, device=dev)
        call("w2e_jpeg_entropy", _p(coef), b, h, w, _p(_huff_table(dev)), _p(out), cap, _p(lengths), _p(work), stream_ptr())
        guess = min(cap, h * w // _JPEG_GUESS_DIVISOR + 1024)
        packed = torch.cat((lengths.view(torch.uint8).view(b, 8), out[:, :guess]), dim=1).cpu().numpy()
        sizes = packed[:, :8].copy().view("<i8").ravel().tolist()
        data = packed[:, 8:]
        if max(sizes) > guess:
            data = out[:, :max(sizes)].cpu().numpy()
    head = jpeg_header(h, w, quality)
    files = [head + data[i, :n].tobytes().replace(b"\xff", b"\xff\x00") + b"\xff\xd9" for i, n in enumerate(sizes)]
    return files[0] if x.ndim == 3 else files


def save_image(x, fp, nrow=8, padding=2, value_range=(-1, 1), pad_value=0.0, quality=75):
    """`torchvision.utils.save_image(x, fp, nrow=, padding=, normalize=True, range=value_range, pad_value=)` (0.8.2) for a `.jpg`:
    fp32 [B,C,H,W] (C = 1 or 3) on the GPU -> to_bytes' canvas -> to_jpeg -> the file.  fp: a path ending in .jpg / .jpeg, or an
    object with write() (the reference only ever writes JPEG).  This function writes no PNG and refuses a `.png` path: a lossless
    file of the same canvas goes through `save_png`."""
    if isinstance(fp, (str, os.PathLike)):
        if os.path.splitext(os.fspath(fp))[1].lower() not in (".jpg", ".jpeg"):
            raise ValueError(f"save_image: {os.fspath(fp)!r} does not end in .jpg or .jpeg; PNG (and every other format) is not implemented")
    elif not hasattr(fp, "write"):
        raise ValueError(f"save_image: fp is a path ending in .jpg / .jpeg or an object with write() (got {type(fp).__name__})")
    _check_quality("save_image", quality)
    data = to_jpeg(to_bytes(x, value_range=value_range, nrow=nrow, padding=padding, pad_value=pad_value, grid=True), quality)
    if hasattr(fp, "write"):
        fp.write(data)
    else:
        with open(fp, "wb") as f:
            f.write(data)


# ---- JPEG decoding (include/w2e_jpeg.h, csrc/jpeg_decode.hip; DESIGN.md "K17c") ----
JPEG_SAMPLINGS = ("420", "444", "grey")   # W2E_JPEG_420, W2E_JPEG_444, W2E_JPEG_GREY
JPEG_SUB_BITS = 512                       # the default subsequence length of the entropy decoder, in bits: the fastest of 256 / 512 / 1024 at batch 8
_JPEG_TABLE_WORDS = CONSTS["W2E_JPEG_TABLE_WORDS"]
_JPEG_MAX_SCAN_BITS = CONSTS["W2E_JPEG_MAX_SCAN_BITS"]
_JPEG_SOF_NAMES = {0xC1: "an extended-sequential JPEG", 0xC2: "a progressive JPEG", 0xC3: "a lossless JPEG", 0xC5: "a hierarchical JPEG",
                   0xC6: "a hierarchical JPEG", 0xC7: "a hierarchical JPEG", 0xC9: "an arithmetic-coded JPEG", 0xCA: "an arithmetic-coded JPEG",
                   0xCB: "an arithmetic-coded JPEG", 0xCD: "an arithmetic-coded JPEG", 0xCE: "an arithmetic-coded JPEG", 0xCF: "an arithmetic-coded JPEG"}
_JPEG_STATUS = ((1, "the scan does not hold the image's number of blocks"), (2, "a coefficient category above 11 (DC) or 10 (AC)"),
                (4, "the scan ends inside a block"))
_JPEG_NEXT_MARKER = re.compile(rb"\xff[^\x00]")


def _refuse(what):
    raise ValueError(f"jpeg_parse: the file is {what}, which the GPU decoder does not take; decode it with Pillow")


def jpeg_parse(data):
    """The host side of the decoder: walk the markers of a JPEG file and hand back what the kernels need, as a dict -- `h`, `w`,
    `sampling` ("420" | "444" | "grey"), `tables` (int32 CPU [components, 64]: each component's quantisation table in natural,
    row-major order), `huffman` (per component ((counts per length 1..16, symbols) of its DC table, the same of its AC table): the
    file's own DHT lists) and `scan` (the entropy-coded segment up to EOI, byte stuffing 0xFF 0x00 -> 0xFF removed).
    In scope: baseline sequential (SOF0), 8 bits, Huffman coded, one scan, no restart interval; one component (grey), or three that
    are YCbCr by libjpeg's rule (a JFIF marker; otherwise an Adobe marker with transform 1; otherwise anything but the ids R, G, B)
    sampled 4:4:4 or 4:2:0; sizes 1..16384.  Everything else -- progressive, 12 bits, arithmetic coding, DRI != 0, 4:2:2 and other
    samplings, CMYK and RGB-coded files, several scans, data that is no JPEG -- raises a ValueError that names what the file is.  EXIF
    orientation is ignored, as Image.open ignores it.  A file that ends inside its scan is NOT refused here: its scan goes to the
    kernels as it is and their status refuses it."""
    if isinstance(data, (bytearray, memoryview)):
        data = bytes(data)
    if not isinstance(data, bytes):
        raise ValueError(f"jpeg_parse: data is the bytes of a JPEG file (got {type(data).__name__})")
    if data[:8] == b"\x89PNG\r\n\x1a\n":
        _refuse("a PNG")
    if data[:2] != b"\xff\xd8":
        _refuse("no JPEG (it does not begin with the SOI marker)")
    at, quant, huff, frame, jfif, adobe = 2, {}, {}, None, False, None
    cut = "a JPEG cut inside its header"
    while True:
        if at + 2 > len(data):
            _refuse(cut)
        if data[at] != 0xFF:
            _refuse(f"a corrupt JPEG (no marker at byte {at})")
        marker = data[at + 1]
        if marker == 0xFF:  # a fill byte
            at += 1
            continue
        if marker == 0xD9:
            _refuse("a JPEG without a scan")
        if at + 4 > len(data):
            _refuse(cut)
        size = int.from_bytes(data[at + 2:at + 4], "big")
        if size < 2 or at + 2 + size > len(data):
            _refuse(cut)
        body = data[at + 4:at + 2 + size]
        at += 2 + size
        if marker == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif marker == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif marker == 0xDB:
            while body:
                if body[0] >> 4:
                    _refuse("a JPEG with 16-bit quantisation tables")
                if len(body) < 65 or (body[0] & 15) > 3:
                    _refuse("a corrupt JPEG (a bad DQT segment)")
                quant[body[0] & 15] = [body[1 + _JPEG_ZIGZAG_POS[i]] for i in range(64)]
                body = body[65:]
        elif marker == 0xC4:
            while body:
                counts = tuple(body[1:17])
                if len(body) < 17 or (body[0] >> 4) > 1 or (body[0] & 15) > 3 or sum(counts) > 256 or len(body) < 17 + sum(counts):
                    _refuse("a corrupt JPEG (a bad DHT segment)")
                room = 1  # codes still free at the current length
                for n in counts:
                    room = 2 * room - n
                    if room < 0:
                        _refuse("a corrupt JPEG (a DHT segment whose codes do not fit their lengths)")
                huff[body[0]] = (counts, bytes(body[17:17 + sum(counts)]))
                body = body[17 + sum(counts):]
        elif marker == 0xC0:
            if frame is not None:
                _refuse("a JPEG with several frames")
            if len(body) < 6 or len(body) < 6 + 3 * body[5]:
                _refuse(cut)
            if body[0] != 8:
                _refuse(f"a {body[0]}-bit JPEG")
            h, w = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            frame = [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(body[5])]
        elif marker in _JPEG_SOF_NAMES:
            _refuse(_JPEG_SOF_NAMES[marker] + (f" ({body[0]} bits)" if body and body[0] != 8 else ""))
        elif marker == 0xCC:
            _refuse("an arithmetic-coded JPEG")
        elif marker == 0xDD:
            if len(body) >= 2 and int.from_bytes(body[:2], "big"):
                _refuse("a JPEG with a restart interval (DRI)")
        elif marker == 0xDA:
            break
    if frame is None:
        _refuse("a JPEG whose scan comes before its frame header")
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        _refuse(f"a JPEG of {h} x {w} pixels (sizes are 1..16384)")
    ids, factors = tuple(f[0] for f in frame), tuple(f[1] for f in frame)
    if len(frame) == 1:
        sampling = "grey"
    elif len(frame) == 3:
        if (not jfif and adobe is not None and adobe != 1) or (not jfif and adobe is None and ids == (82, 71, 66)):
            _refuse("an RGB-coded JPEG (no YCbCr transform)")
        sampling = {(0x22, 0x11, 0x11): "420", (0x11, 0x11, 0x11): "444"}.get(factors)
        if sampling is None:
            name = " (4:2:2)" if factors == (0x21, 0x11, 0x11) else ""
            _refuse("a JPEG sampled " + ", ".join(f"{f >> 4}x{f & 15}" for f in factors) + name + ", neither 4:4:4 nor 4:2:0")
    else:
        _refuse(f"a JPEG of {len(frame)} components" + (" (CMYK or YCCK)" if len(frame) == 4 else ""))
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        _refuse("a corrupt JPEG (a bad SOS segment)")
    if body[0] != len(frame) or tuple(body[1 + 2 * i] for i in range(body[0])) != ids:
        _refuse("a JPEG of several scans")
    if tuple(body[-3:]) != (0, 63, 0):
        _refuse("a JPEG whose scan is no whole sequential scan (a progressive one)")
    select = [body[2 + 2 * i] for i in range(len(frame))]
    if any(f[2] not in quant for f in frame) or any((s >> 4) not in huff or (0x10 | (s & 15)) not in huff for s in select):
        _refuse("a corrupt JPEG (its scan uses a table that it does not define)")
    m = _JPEG_NEXT_MARKER.search(data, at)
    if m is None:  # the file ends inside its scan
        end, marker = len(data) - (1 if data[-1:] == b"\xff" else 0), None
    else:
        end, j = m.start(), m.start() + 1
        while j < len(data) and data[j] == 0xFF:  # fill bytes in front of the marker
            j += 1
        marker = data[j] if j < len(data) else None
        if marker == 0:
            _refuse("a corrupt JPEG (fill bytes inside its scan)")
    if marker is not None and 0xD0 <= marker <= 0xD7:
        _refuse("a JPEG with restart markers in its scan")
    if marker is not None and marker != 0xD9:
        _refuse("a JPEG of several scans")
    return {"h": h, "w": w, "sampling": sampling, "tables": torch.tensor([quant[f[2]] for f in frame], dtype=torch.int32),
            "huffman": tuple((huff[s >> 4], huff[0x10 | (s & 15)]) for s in select), "scan": data[at:end].replace(b"\xff\x00", b"\xff")}


@functools.lru_cache(maxsize=64)
def _jpeg_decode_table(counts, symbols):
    """One code table as the kernels read it (include/w2e_jpeg.h): uint32 [W2E_JPEG_TABLE_WORDS]."""
    lut, maxcode, valoff = np.zeros(512, np.uint16), np.full(18, -1, np.int32), np.zeros(17, np.int32)
    code = k = 0
    for length in range(1, 17):
        n = counts[length - 1]
        if n:
            valoff[length] = k - code
            if length <= 9:
                for j in range(n):
                    lut[(code + j) << (9 - length):(code + j + 1) << (9 - length)] = (length << 8) | symbols[k + j]
            code, k = code + n, k + n
            maxcode[length] = code - 1
        code <<= 1
    vals = np.zeros(256, np.uint8)
    vals[:len(symbols)] = np.frombuffer(symbols, np.uint8)
    t = np.zeros(_JPEG_TABLE_WORDS, np.uint32)
    t[:256], t[256:274], t[274:291], t[320:384] = lut.view(np.uint32), maxcode.view(np.uint32), valoff.view(np.uint32), vals.view(np.uint32)
    t.setflags(write=False)
    return t


def jpeg_decode_plan(batch, h, w, sampling, scan_bits, sub_bits=JPEG_SUB_BITS):
    """w2e_jpeg_decode_plan as a dict: blocks per image, the MCU grid, subsequences per image, the workspace bytes of the two stages,
    the most launches the relaxation can take, the coefficient elements per image.  Pure host."""
    plan = (ctypes.c_int64 * 8)()
    call("w2e_jpeg_decode_plan", batch, h, w, _sampling_id("jpeg_decode_plan", sampling), scan_bits, sub_bits, plan)
    return {"blocks": plan[0], "mcus": (plan[2], plan[1]), "subsequences": plan[3], "workspace": plan[4], "pixel_workspace": plan[5],
            "launches": plan[6], "coefficients": plan[7]}


def _sampling_id(who, sampling):
    if sampling not in JPEG_SAMPLINGS:
        raise ValueError(f"{who}: sampling must be one of {JPEG_SAMPLINGS} (got {sampling!r})")
    return JPEG_SAMPLINGS.index(sampling)


def _check_sub_bits(who, sub_bits):
    if not (isinstance(sub_bits, int) and not isinstance(sub_bits, bool) and 32 <= sub_bits <= 4096 and sub_bits % 32 == 0):
        raise ValueError(f"{who}: sub_bits is a multiple of 32 in 32..4096 (got {sub_bits!r})")


def _decode_device(who, device):
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: device must be a GPU (got {device}) -- there is no CPU path")
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who}: the decoder runs on the GPU and none is available -- there is no CPU path (decode with Pillow instead)")
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)


def _parsed_list(who, files):
    single = isinstance(files, (bytes, bytearray, memoryview))
    files = [files] if single else list(files)
    return single, [jpeg_parse(f) for f in files]


def _same_geometry(who, parsed):
    keys = {(p["h"], p["w"], p["sampling"]) for p in parsed}
    if len(keys) != 1:
        raise ValueError(f"{who}: the files of one call must agree in height, width and sampling (got {sorted(keys)}); from_jpeg takes a mixed list")


class _JpegBatch:
    """The files of one geometry on the device: ONE upload (offsets and lengths, the code tables, the scans one after the other, each
    padded with 0xFF to a multiple of 4 bytes), the plan, the workspace of stage 1."""

    def __init__(self, parsed, device, sub_bits):
        p0 = parsed[0]
        self.b, self.h, self.w, self.sampling = len(parsed), p0["h"], p0["w"], _sampling_id("from_jpeg", p0["sampling"])
        self.sub_bits, self.device = sub_bits, device
        self.bits = [8 * len(p["scan"]) for p in parsed]
        self.scan_bits = max(self.bits)
        if self.scan_bits > _JPEG_MAX_SCAN_BITS:
            raise ValueError(f"from_jpeg: a scan of {self.scan_bits // 8} bytes is longer than the decoder's 32-bit bit positions reach; decode it with Pillow")
        meta, tables = np.zeros((self.b, 2), np.int64), np.zeros((self.b, 6, _JPEG_TABLE_WORDS), np.uint32)
        scans, at = [], 0
        for i, p in enumerate(parsed):
            meta[i] = at, self.bits[i]
            for c, (dc, ac) in enumerate(p["huffman"]):
                tables[i, 2 * c], tables[i, 2 * c + 1] = _jpeg_decode_table(*dc), _jpeg_decode_table(*ac)
            scans.append(p["scan"] + b"\xff" * (-len(p["scan"]) % 4))
            at += len(scans[-1])
        self.scan_bytes = at
        head = meta.tobytes() + tables.tobytes()
        blob = bytearray(head + b"".join(scans) + b"\xff" * 4)  # (never empty past the head: a pointer the library can check)
        self.blob = torch.frombuffer(blob, dtype=torch.uint8).to(device)
        self.meta, self.tables, self.scan = self.blob[:16 * self.b], self.blob[16 * self.b:len(head)], self.blob[len(head):]
        self.plan = jpeg_decode_plan(self.b, self.h, self.w, p0["sampling"], self.scan_bits, sub_bits)
        self.work = torch.empty(max(self.plan["workspace"], 16), dtype=torch.uint8, device=device)
        self.quant = torch.zeros((self.b, 3, 64), dtype=torch.int32)
        for i, p in enumerate(parsed):
            self.quant[i, :p["tables"].shape[0]] = p["tables"]

    def _args(self):
        return (_p(self.scan), _p(self.meta), _p(self.tables), self.scan_bytes, self.b, self.h, self.w, self.sampling, self.scan_bits, self.sub_bits)

    def relax(self):
        """Launch w2e_jpeg_decode_sync until nothing changes; one 4-byte copy per launch.  Returns the number of launches."""
        bound = self.plan["launches"]
        changed = torch.zeros(bound, dtype=torch.int32, device=self.device)
        for launch in range(bound):
            call("w2e_jpeg_decode_sync", *self._args(), launch, _p(self.work), _p(changed[launch:]), stream_ptr())
            if changed[launch].item() == 0:
                return launch + 1
        raise RuntimeError(f"jpeg decoder: the relaxation did not settle in its {bound} launches (a bug, not the file's fault)")

    def states(self):
        n = self.plan["subsequences"]
        e = self.work[:8 * self.b * n].view(torch.int32).view(self.b, n, 2).cpu()
        out = []
        for i in range(self.b):
            ni = max(1, -(-self.bits[i] // self.sub_bits))
            out.append(torch.stack((e[i, :ni, 0], e[i, :ni, 1] >> 8, e[i, :ni, 1] & 255), dim=1))
        return out

    def coefficients(self):
        coef = torch.empty((self.b, self.plan["blocks"], 64), dtype=torch.int16, device=self.device)
        status = torch.empty((self.b,), dtype=torch.int32, device=self.device)
        call("w2e_jpeg_decode_coefficients", *self._args(), _p(self.work), _p(coef), _p(status), stream_ptr())
        return coef, status


def _jpeg_raise(who, status, names=None):
    for i, s in enumerate(status.tolist()):
        if s:
            why = "; ".join(text for bit, text in _JPEG_STATUS if s & bit)
            raise ValueError(f"{who}: image {i if names is None else names[i]} has a corrupt scan (status {s}): {why}")


def jpeg_decode_states(files, sub_bits=JPEG_SUB_BITS, device=None):
    """The entropy decoder's relaxation on its own (for tests and for finding a fault): the bytes of one file, or a list of files of
    one geometry -> (the converged entry state of every subsequence, int32 CPU [n, 3] = (bit position of the next symbol, block
    position in the MCU, next zigzag index) per image; the number of launches it took)."""
    _check_sub_bits("jpeg_decode_states", sub_bits)
    single, parsed = _parsed_list("jpeg_decode_states", files)
    _same_geometry("jpeg_decode_states", parsed)
    device = _decode_device("jpeg_decode_states", device)
    with torch.cuda.device(device):
        batch = _JpegBatch(parsed, device, sub_bits)
        launches = batch.relax()
        states = batch.states()
    return (states[0] if single else states), launches


def jpeg_decode_coefficients(files, sub_bits=JPEG_SUB_BITS, device=None):
    """Stage 1 of the decoder on its own: the bytes of one file -> int16 [blocks, 64] on the GPU; a list of files of one geometry ->
    [B, blocks, 64].  Zigzag order, MCU scan order, the blocks outside the image included: for a file `to_jpeg` made, what
    `jpeg_coefficients` returned.  The result is the same for every sub_bits.  A corrupt scan raises ValueError."""
    _check_sub_bits("jpeg_decode_coefficients", sub_bits)
    single, parsed = _parsed_list("jpeg_decode_coefficients", files)
    _same_geometry("jpeg_decode_coefficients", parsed)
    device = _decode_device("jpeg_decode_coefficients", device)
    with torch.cuda.device(device):
        batch = _JpegBatch(parsed, device, sub_bits)
        batch.relax()
        coef, status = batch.coefficients()
        _jpeg_raise("jpeg_decode_coefficients", status.cpu())
    return coef[0] if single else coef


def _jpeg_pixels(coef, quant, h, w, sampling_id, plan):
    b = coef.shape[0]
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=coef.device)
    work = torch.empty(max(plan["pixel_workspace"], 16), dtype=torch.uint8, device=coef.device)
    call("w2e_jpeg_pixels", _p(coef), _p(quant), b, h, w, sampling_id, _p(out), _p(work), stream_ptr())
    return out


def jpeg_pixels(coef, tables, h, w, sampling):
    """Stage 2 of the decoder on its own: int16 [blocks, 64] or [B, blocks, 64] on the GPU (zigzag order, scan order) and the
    quantisation tables (an integer tensor [components, 64], or [B, components, 64] for one set per image, natural order; CPU or GPU)
    -> uint8 [h, w, 3] or [B, h, w, 3]: dequantisation, libjpeg's accurate integer inverse DCT, for "420" its fancy chroma
    up-sampling, YCbCr -> RGB (grey: R = G = B = Y)."""
    _on_gpu("jpeg_pixels", "coef", coef, torch.int16, (2, 3))
    sid = _sampling_id("jpeg_pixels", sampling)
    _check_size("jpeg_pixels", h), _check_size("jpeg_pixels", w)
    c3 = coef.unsqueeze(0) if coef.ndim == 2 else coef
    c3 = c3 if c3.is_contiguous() else c3.contiguous()
    b = c3.shape[0]
    with torch.cuda.device(coef.device):
        plan = jpeg_decode_plan(b, h, w, sampling, 0)
        if tuple(c3.shape[1:]) != (plan["blocks"], 64):
            raise RuntimeError(f"jpeg_pixels: a {h} x {w} image sampled {sampling} has {plan['blocks']} blocks of 64 (got shape {tuple(coef.shape)})")
        if not torch.is_tensor(tables) or tables.is_floating_point() or tables.ndim not in (2, 3) or tables.shape[-1] != 64:
            raise RuntimeError("jpeg_pixels: tables is an integer tensor [components, 64] or [B, components, 64]")
        t3 = tables.unsqueeze(0).expand(b, -1, -1) if tables.ndim == 2 else tables
        if t3.shape[0] != b or t3.shape[1] != (1 if sampling == "grey" else 3):
            raise RuntimeError(f"jpeg_pixels: tables of shape {tuple(tables.shape)} for {b} images of {1 if sampling == 'grey' else 3} components")
        quant = torch.zeros((b, 3, 64), dtype=torch.int32, device=coef.device)
        quant[:, :t3.shape[1]] = t3.to(device=coef.device, dtype=torch.int32)
        out = _jpeg_pixels(c3, quant, h, w, sid, plan)
    return out[0] if coef.ndim == 2 else out


def from_jpeg(data, device=None, sub_bits=JPEG_SUB_BITS, stack=False):
    """`np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))` on the GPU, byte for byte: the bytes of a baseline JPEG file ->
    uint8 [H, W, 3]; a list of files -> a list of tensors (stack=True: one [B, H, W, 3] tensor; the sizes must then agree).  Only the
    coded file crosses to the device.  Files of equal geometry (height, width, sampling) are decoded together as one batch: one
    upload, the launches of the relaxation (`jpeg_decode_states`; one 4-byte copy each), then six launches.  What is in scope:
    `jpeg_parse`, which refuses everything else on the host, before any launch.  A corrupt scan -- a file cut short, a damaged
    byte -- raises ValueError; libjpeg's behaviour of warning and going on with grey blocks is NOT reproduced.
    `to_tensor(from_jpeg(files, stack=True), 256)` is the reference's input side, file to normalised tensor, on the GPU."""
    _check_sub_bits("from_jpeg", sub_bits)
    single, parsed = _parsed_list("from_jpeg", data)
    if stack and len({(p["h"], p["w"]) for p in parsed}) > 1:
        raise ValueError(f"from_jpeg: stack=True needs images of one size (got {sorted({(p['h'], p['w']) for p in parsed})})")
    if not parsed:
        return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=_decode_device("from_jpeg", device)) if stack else []
    device = _decode_device("from_jpeg", device)
    groups = {}
    for i, p in enumerate(parsed):
        groups.setdefault((p["h"], p["w"], p["sampling"]), []).append(i)
    out, pending = [None] * len(parsed), []
    with torch.cuda.device(device):
        for members in groups.values():
            batch = _JpegBatch([parsed[i] for i in members], device, sub_bits)
            batch.relax()
            coef, status = batch.coefficients()
            pixels = _jpeg_pixels(coef, batch.quant.to(device), batch.h, batch.w, batch.sampling, batch.plan)
            pending.append((members, status))
            for j, i in enumerate(members):
                out[i] = pixels[j]
        for members, status in pending:
            _jpeg_raise("from_jpeg", status.cpu(), members)
    if single:
        return out[0]
    return torch.stack(out) if stack else out


def load_image(fp, device=None):
    """The counterpart of `save_image`: a path, or an object with read(), of a baseline JPEG file -> `from_jpeg` of its bytes, uint8
    [H, W, 3] on the GPU."""
    if hasattr(fp, "read"):
        data = fp.read()
    elif isinstance(fp, (str, os.PathLike)):
        with open(fp, "rb") as f:
            data = f.read()
    else:
        raise ValueError(f"load_image: fp is a path or an object with read() (got {type(fp).__name__})")
    return from_jpeg(data, device=device)


# ---- PNG decoding (include/w2e_png.h, csrc/png.hip, csrc/png_core.h; DESIGN.md "K17d") ----
PNG_MODES = ("RGB", "raw")   # W2E_PNG_MODE_RGB, W2E_PNG_MODE_RAW
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PNG_COLOURS = {0: "grey", 2: "RGB", 3: "palette", 4: "grey + alpha", 6: "RGBA"}
_PNG_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
_PNG_STATUS = tuple((CONSTS["W2E_PNG_STATUS_" + name], text) for name, text in (
    ("TYPE", "a block of type 3"), ("STORED", "a stored block whose LEN and NLEN disagree"), ("LENGTHS", "a bad code-length set"),
    ("CODE", "a code that matches no symbol (or length symbol 286 / 287, distance symbol 30 / 31)"),
    ("DISTANCE", "a distance that reaches before the start of the output"), ("INPUT", "the input ends inside the stream"),
    ("SHORT", "the stream ends before the image's size"), ("LONG", "the stream goes on past the image's size"),
    ("ADLER", "the Adler-32 of the inflated bytes is not the stream's"), ("FILTER", "a filter byte above 4")))


def _png_refuse(what):
    raise ValueError(f"png_parse: the file is {what}, which the GPU decoder does not take; decode it with Pillow")


def _check_zlib_header(who, z):
    """The two header bytes of a zlib stream (RFC 1950): method 8, a window of at most 32 KiB, the check bits, no preset dictionary."""
    if len(z) < 2 or (z[0] & 15) != 8 or (z[0] >> 4) > 7 or ((z[0] << 8) | z[1]) % 31:
        raise ValueError(f"{who}: the compressed data does not begin with a zlib header")
    if z[1] & 32:
        raise ValueError(f"{who}: the zlib stream asks for a preset dictionary, which the GPU decoder does not take; decode it with Pillow")


def png_parse(data):
    """The host side of the PNG decoder: walk the chunks of a file and hand back what the kernels need, as a dict -- `h`, `w`, `colour`
    (the PNG colour type: 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA), `depth`, `palette` (uint32 CPU [256], entry = R | G << 8 |
    B << 16, 0 past the end of PLTE; None without a palette) and `stream` (the IDAT payloads joined: one zlib stream).
    Every chunk's CRC is verified (a bad one is a ValueError, as with Pillow).  In scope: non-interlaced, 8 bits for colour types 0, 2,
    4, 6, and 1 / 2 / 4 / 8 bits for the palette; sizes 1..16384.  Adam7 interlacing, 16 bits, grey below 8 bits, APNG, a preset
    dictionary and larger sizes raise a ValueError that names what the file is and ends "decode it with Pillow".  tRNS and every
    other ancillary chunk are ignored, as `convert("RGB")` ignores transparency.  A damaged zlib stream is NOT refused here: it goes to
    the kernels as it is and their status refuses it."""
    if isinstance(data, (bytearray, memoryview)):
        data = bytes(data)
    if not isinstance(data, bytes):
        raise ValueError(f"png_parse: data is the bytes of a PNG file (got {type(data).__name__})")
    if data[:8] != _PNG_SIGNATURE:
        _png_refuse("no PNG (it does not begin with the PNG signature)")
    at, head, palette, parts, ended = 8, None, None, [], False
    while not ended:
        if at + 8 > len(data):
            raise ValueError("png_parse: the file is cut inside a chunk")
        size, kind = int.from_bytes(data[at:at + 4], "big"), data[at + 4:at + 8]
        if at + 12 + size > len(data):
            raise ValueError(f"png_parse: the file is cut inside its {kind.decode('latin-1')} chunk")
        body = data[at + 8:at + 8 + size]
        if zlib.crc32(data[at + 4:at + 8 + size]) != int.from_bytes(data[at + 8 + size:at + 12 + size], "big"):
            raise ValueError(f"png_parse: the CRC of the {kind.decode('latin-1')} chunk at byte {at} is wrong")
        at += 12 + size
        if head is None and kind != b"IHDR":
            raise ValueError("png_parse: the first chunk is not IHDR")
        if kind == b"IHDR":
            if size != 13 or head is not None:
                raise ValueError("png_parse: a bad IHDR chunk")
            head = (int.from_bytes(body[0:4], "big"), int.from_bytes(body[4:8], "big")) + tuple(body[8:13])
        elif kind == b"PLTE":
            if size % 3 or not 3 <= size <= 768:
                raise ValueError("png_parse: a bad PLTE chunk")
            rgb = np.frombuffer(body, np.uint8).reshape(-1, 3).astype(np.uint32)
            palette = torch.zeros(256, dtype=torch.int32)
            palette[:len(rgb)] = torch.from_numpy((rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)).astype(np.int32))
        elif kind == b"acTL":
            _png_refuse("an animated PNG (APNG)")
        elif kind == b"IDAT":
            parts.append(body)
        elif kind == b"IEND":
            ended = True
    w, h, depth, colour, compression, filtering, interlace = head
    if colour not in _PNG_COLOURS or compression or filtering or depth not in (1, 2, 4, 8, 16) or interlace > 1:
        raise ValueError(f"png_parse: a bad IHDR chunk (colour type {colour}, depth {depth}, compression {compression}, filter {filtering}, interlace {interlace})")
    if interlace:
        _png_refuse("an interlaced PNG (Adam7)")
    if depth == 16:
        _png_refuse("a 16-bit PNG")
    if depth < 8 and colour == 0:
        _png_refuse(f"a {depth}-bit grey PNG")
    if depth < 8 and colour != 3:
        raise ValueError(f"png_parse: a bad IHDR chunk ({_PNG_COLOURS[colour]} at {depth} bits)")
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        _png_refuse(f"a PNG of {h} x {w} pixels (sizes are 1..16384)")
    if colour == 3 and palette is None:
        raise ValueError("png_parse: a palette PNG without a PLTE chunk")
    if not parts:
        raise ValueError("png_parse: a PNG without an IDAT chunk")
    stream = b"".join(parts)
    _check_zlib_header("png_parse", stream)
    return {"h": h, "w": w, "colour": colour, "depth": depth, "palette": palette if colour == 3 else None, "stream": stream}


def _png_mode_id(who, mode):
    if mode not in PNG_MODES:
        raise ValueError(f"{who}: mode must be one of {PNG_MODES} (got {mode!r})")
    return PNG_MODES.index(mode)


def png_plan(batch, h, w, colour, depth=8, mode="RGB"):
    """w2e_png_plan as a dict: the bytes of a filtered row (filter byte included), the inflated size of an image, the pitch of the
    filtered-row buffer, the channels and bytes of the output, the filters' pixel distance, stage 1's LDS bound and stage 2's band.
    Pure host."""
    plan = (ctypes.c_int64 * 8)()
    call("w2e_png_plan", batch, h, w, colour, depth, _png_mode_id("png_plan", mode), plan)
    return {"row_bytes": plan[0], "size": plan[1], "pitch": plan[2], "channels": plan[3], "out_bytes": plan[4], "bpp": plan[5], "lds": plan[6],
            "band": plan[7]}


def _png_upload(streams, sizes, device):
    """ONE upload: offsets and lengths, the inflated sizes, then the streams one after the other, each padded to a multiple of 4."""
    b = len(streams)
    meta, at, parts = np.zeros((b, 3), np.int64), 0, []
    for i, z in enumerate(streams):
        meta[i] = at, len(z), sizes[i]
        parts.append(bytes(z) + b"\0" * (-len(z) % 4))
        at += len(parts[-1])
    head = np.ascontiguousarray(meta[:, :2]).tobytes() + np.ascontiguousarray(meta[:, 2]).tobytes()
    blob = torch.frombuffer(bytearray(head + b"".join(parts) + b"\0" * 4), dtype=torch.uint8).to(device)
    return blob[:16 * b], blob[16 * b:24 * b], blob[24 * b:], at


def _png_inflate(streams, sizes, pitch, device):
    b = len(streams)
    meta, dsizes, data, total = _png_upload(streams, sizes, device)
    raw = torch.empty((b, pitch), dtype=torch.uint8, device=device)
    status = torch.empty((b,), dtype=torch.int32, device=device)
    call("w2e_png_inflate", _p(data), _p(meta), _p(dsizes), total, b, _p(raw), pitch, _p(status), stream_ptr())
    return raw, status


def _png_raise(who, status, names=None):
    for i, s in enumerate(status.tolist()):
        if s:
            why = "; ".join(text for bit, text in _PNG_STATUS if s & bit)
            raise ValueError(f"{who}: image {i if names is None else names[i]} has a corrupt stream (status {s}): {why}")


def png_inflate(streams, sizes, device=None):
    """Stage 1 of the decoder on its own (for tests and for finding a fault): a zlib stream (bytes) and the exact number of bytes it
    inflates to -> uint8 [size] on the GPU; a list of streams and a list of sizes -> a list of tensors, inflated as ONE batch in one
    launch.  A corrupt stream, or one that inflates to another size, raises ValueError."""
    single = isinstance(streams, (bytes, bytearray, memoryview))
    streams, sizes = ([bytes(streams)], [sizes]) if single else ([bytes(z) for z in streams], list(sizes))
    if len(streams) != len(sizes) or any(not (isinstance(n, int) and 0 <= n <= 0x7fffffff) for n in sizes):
        raise ValueError(f"png_inflate: one size (an integer in 0..2^31-1) per stream (got {len(streams)} streams and sizes {sizes!r})")
    for z in streams:
        _check_zlib_header("png_inflate", z)
    device = _decode_device("png_inflate", device)
    if not streams:
        return []
    with torch.cuda.device(device):
        raw, status = _png_inflate(streams, sizes, -(-max(max(sizes), 1) // 4) * 4, device)
        _png_raise("png_inflate", status.cpu())
    out = [raw[i, :n] for i, n in enumerate(sizes)]
    return out[0] if single else out


def _png_pixels(raw, palette, h, w, colour, depth, mode_id, plan, status):
    b = raw.shape[0]
    shape = (b, h, w) if plan["channels"] == 1 else (b, h, w, plan["channels"])
    out = torch.empty(shape, dtype=torch.uint8, device=raw.device)
    call("w2e_png_pixels", _p(raw), raw.shape[1], _p(palette), b, h, w, colour, depth, mode_id, _p(out), _p(status), stream_ptr())
    return out


def png_pixels(raw, h, w, colour, depth=8, palette=None, mode="RGB"):
    """Stage 2 of the decoder on its own: the filtered rows of an image, uint8 [h * row bytes] (each row its filter byte and its
    bytes, as a zlib stream inflates to them) or [B, h * row bytes] on the GPU -> the pixels of `mode`: "RGB" uint8 [h, w, 3]; "raw"
    [h, w] for grey and palette (the index), [h, w, 2 | 3 | 4] for grey + alpha, RGB and RGBA.  palette: an integer tensor [n, 3] (n <=
    256) or [B, n, 3] of R, G, B for colour 3.  The input is left as it was.  A filter byte above 4 raises ValueError."""
    _on_gpu("png_pixels", "raw", raw, torch.uint8, (1, 2))
    mode_id = _png_mode_id("png_pixels", mode)
    _check_size("png_pixels", h), _check_size("png_pixels", w)
    r2 = raw.unsqueeze(0) if raw.ndim == 1 else raw
    b = r2.shape[0]
    with torch.cuda.device(raw.device):
        plan = png_plan(b, h, w, colour, depth, mode)
        if r2.shape[1] != plan["size"]:
            raise RuntimeError(f"png_pixels: a {h} x {w} image of colour type {colour} at {depth} bits has {plan['size']} filtered bytes (got shape {tuple(raw.shape)})")
        table = None
        if colour == 3:
            if not torch.is_tensor(palette) or palette.is_floating_point() or palette.ndim not in (2, 3) or palette.shape[-1] != 3 or palette.shape[-2] > 256:
                raise RuntimeError("png_pixels: palette is an integer tensor [n, 3] or [B, n, 3] with n <= 256 for colour type 3")
            p3 = (palette.unsqueeze(0).expand(b, -1, -1) if palette.ndim == 2 else palette).to(device=raw.device, dtype=torch.int32)
            if p3.shape[0] != b:
                raise RuntimeError(f"png_pixels: palette of shape {tuple(palette.shape)} for {b} images")
            table = torch.zeros((b, 256), dtype=torch.int32, device=raw.device)
            table[:, :p3.shape[1]] = (p3[..., 0] & 255) | ((p3[..., 1] & 255) << 8) | ((p3[..., 2] & 255) << 16)
        work = torch.zeros((b, plan["pitch"]), dtype=torch.uint8, device=raw.device)  # (the kernel keeps rows in its input)
        work[:, :plan["size"]] = r2
        status = torch.zeros((b,), dtype=torch.int32, device=raw.device)
        out = _png_pixels(work, table, h, w, colour, depth, mode_id, plan, status)
        _png_raise("png_pixels", status.cpu())
    return out[0] if raw.ndim == 1 else out


def from_png(data, mode="RGB", device=None, stack=False):
    """`np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))` (mode="RGB": uint8 [H, W, 3], grey replicated, alpha dropped, the
    palette looked up) or `np.asarray(Image.open(io.BytesIO(data)))` (mode="raw": [H, W] for grey and palette files -- the ids a
    parsing label holds -- and [H, W, 2 | 3 | 4] for grey + alpha, RGB and RGBA) on the GPU, byte for byte: the bytes of a PNG file
    -> a tensor; a list of files -> a list of tensors (stack=True: one tensor; the shapes must then agree).  Only the compressed
    stream and the palette cross to the device.  Files of equal geometry (height, width, colour type, depth) are decoded together:
    one upload and two launches per group, all streams of a group inflating at once, one wave each.  What is in scope: `png_parse`,
    which refuses everything else on the host, before any launch.  A corrupt stream raises ValueError; the status is read once per
    call, after every group is launched.
    `label_ids(from_png(files, mode="raw", stack=True), 64)` is the reference's label side, file to ids, on the GPU."""
    mode_id = _png_mode_id("from_png", mode)
    single = isinstance(data, (bytes, bytearray, memoryview))
    parsed = [png_parse(f) for f in ([data] if single else list(data))]
    device = _decode_device("from_png", device)
    groups = {}
    for i, p in enumerate(parsed):
        groups.setdefault((p["h"], p["w"], p["colour"], p["depth"]), []).append(i)
    if stack and len({(h, w, png_plan(1, h, w, c, d, mode)["channels"]) for h, w, c, d in groups}) > 1:
        raise ValueError(f"from_png: stack=True needs images of one shape (got the (h, w, colour type, depth) {sorted(groups)})")
    if not parsed:
        return torch.empty((0, 0, 0, 3) if mode == "RGB" else (0, 0, 0), dtype=torch.uint8, device=device) if stack else []
    out, pending = [None] * len(parsed), []
    with torch.cuda.device(device):
        for (h, w, colour, depth), members in groups.items():
            plan = png_plan(len(members), h, w, colour, depth, mode)
            raw, status = _png_inflate([parsed[i]["stream"] for i in members], [plan["size"]] * len(members), plan["pitch"], device)
            palette = torch.stack([parsed[i]["palette"] for i in members]).to(device) if colour == 3 else None
            pixels = _png_pixels(raw, palette, h, w, colour, depth, mode_id, plan, status)
            pending.append((members, status))
            for j, i in enumerate(members):
                out[i] = pixels[j]
        for members, status in pending:
            _png_raise("from_png", status.cpu(), members)
    if single:
        return out[0]
    return torch.stack(out) if stack else out


def _read_file(who, fp):
    if hasattr(fp, "read"):
        return fp.read()
    if isinstance(fp, (str, os.PathLike)):
        with open(fp, "rb") as f:
            return f.read()
    raise ValueError(f"{who}: fp is a path or an object with read() (got {type(fp).__name__})")


def load_png(fp, mode="RGB", device=None):
    """A path, or an object with read(), of a PNG file -> `from_png` of its bytes."""
    return from_png(_read_file("load_png", fp), mode=mode, device=device)


def read_image(fp, device=None):
    """`Image.open(fp).convert("RGB")` (show_demo/try_demo.py:96-97) for a PNG or a baseline JPEG file, by its first eight bytes: a
    path, or an object with read() -> uint8 [H, W, 3] on the GPU, through `from_png(mode="RGB")` or `from_jpeg`."""
    data = _read_file("read_image", fp)
    return from_png(data, mode="RGB", device=device) if data[:8] == _PNG_SIGNATURE else from_jpeg(data, device=device)


# ---- PNG encoding (include/w2e_png.h "encoding", csrc/png_encode.hip, csrc/png_deflate_core.h; DESIGN.md "K17e") ----
_PNG_COLOUR_OF_CHANNELS = {1: 0, 2: 4, 3: 2, 4: 6}   # L, LA, RGB, RGBA
_PNG_GUESS = (5, 8)  # to_png's first copy takes 5/8 of the filtered size per image: above a photograph's rate (about 0.55 at 1024 x 1024)


def png_encode_plan(batch, h, w, channels):
    """w2e_png_encode_plan as a dict: the bytes of a filtered row (filter byte included), the filtered size of an image, the pitch of
    the filtered-row buffer, the chunks per image, the slot bytes per chunk, the workspace bytes, the largest possible stream (from the
    stored form: size + 10 per chunk + 6) and the pitch of the stream buffer.  Pure host."""
    plan = (ctypes.c_int64 * 8)()
    call("w2e_png_encode_plan", batch, h, w, channels, plan)
    return {"row_bytes": plan[0], "size": plan[1], "pitch": plan[2], "chunks": plan[3], "slot": plan[4], "workspace": plan[5], "stream": plan[6],
            "out_pitch": plan[7]}


def _png_encode_input(who, x):
    _on_gpu(who, "x", x, torch.uint8, (3, 4))
    if not 1 <= x.shape[-1] <= 4:
        raise RuntimeError(f"{who}: images are [H,W,C] or [B,H,W,C] with C = 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA), channels last (got shape {tuple(x.shape)})")
    x4 = x.unsqueeze(0) if x.ndim == 3 else x
    _check_size(who, x4.shape[1]), _check_size(who, x4.shape[2])
    return x4 if x4.is_contiguous() else x4.contiguous()


def _png_filter(x4, plan):
    b, h, w, c = x4.shape
    raw = torch.empty((b, plan["pitch"]), dtype=torch.uint8, device=x4.device)
    call("w2e_png_filter", _p(x4), b, h, w, c, _p(raw), plan["pitch"], stream_ptr())
    return raw


def png_filter(x):
    """Stage 1 of the encoder on its own (for tests and for finding a fault): uint8 [H,W,C] or [B,H,W,C] on the GPU -> uint8
    [H * (1 + W * C)] or [B, H * (1 + W * C)], the rows a PNG's zlib stream holds: per row the filter byte, then the filtered bytes.
    The filter of every row is the one Pillow chooses (None, Sub, Up or Paeth by the smallest sum of min(v, 256 - v))."""
    x4 = _png_encode_input("png_filter", x)
    with torch.cuda.device(x4.device):
        plan = png_encode_plan(*x4.shape)
        raw = _png_filter(x4, plan)[:, :plan["size"]]
    return raw[0] if x.ndim == 3 else raw


def _png_deflate(raw, sizes, max_size):
    """raw: uint8 [b, pitch] on the GPU; sizes: int64 [b] on the GPU -> (streams uint8 [b, out_pitch], lengths int64 [b])."""
    b = raw.shape[0]
    plan = (ctypes.c_int64 * 4)()
    call("w2e_png_deflate_plan", b, max_size, plan)
    pitch = -(-plan[3] // 4) * 4
    out = torch.empty((b, pitch), dtype=torch.uint8, device=raw.device)
    lengths = torch.empty((b,), dtype=torch.int64, device=raw.device)
    work = torch.empty((plan[2],), dtype=torch.uint8, device=raw.device)
    call("w2e_png_deflate", _p(raw), raw.shape[1], _p(sizes), b, max_size, _p(out), pitch, _p(lengths), _p(work), plan[2], stream_ptr())
    return out, lengths


def _png_fetch(out, lengths, guess):
    """Streams and lengths to the host in ONE copy while no stream is longer than `guess`; a second copy fetches the rest."""
    b = out.shape[0]
    guess = min(out.shape[1], guess)
    packed = torch.cat((lengths.view(torch.uint8).view(b, 8), out[:, :guess]), dim=1).cpu().numpy()
    sizes = packed[:, :8].copy().view("<i8").ravel().tolist()
    data = packed[:, 8:]
    if max(sizes) > guess:
        data = out[:, :max(sizes)].cpu().numpy()
    return [data[i, :n].tobytes() for i, n in enumerate(sizes)]


def png_deflate(raw_list, device=None):
    """Stage 2 of the encoder on its own: a list of buffers (uint8 tensors of one dimension, bytes or numpy arrays; any lengths, empty
    included) -> a list of zlib streams (bytes), coded as ONE batch in two launches.  Every stream inflates to its buffer with any
    inflate; the bytes are this library's own, the same on every run: chunks of 32 KiB coded independently, one deflate block each
    (stored, fixed or dynamic, whichever is shortest), joined by empty stored blocks as zlib's sync flush joins them."""
    if isinstance(raw_list, (bytes, bytearray, memoryview)) or torch.is_tensor(raw_list):
        raise ValueError("png_deflate: raw_list is a list of buffers (got one buffer)")
    buffers = []
    for i, r in enumerate(raw_list):
        if torch.is_tensor(r):
            if r.dtype != torch.uint8 or r.ndim != 1:
                raise RuntimeError(f"png_deflate: buffer {i} must be a uint8 tensor of one dimension (got {r.dtype}, shape {tuple(r.shape)})")
            if not r.is_cuda:
                raise RuntimeError(f"png_deflate: buffer {i} must be on the GPU (got {r.device}): move it with .to('cuda') first -- there is no CPU path")
        else:
            r = np.frombuffer(bytes(r), np.uint8) if not isinstance(r, np.ndarray) else np.ascontiguousarray(r, np.uint8).ravel()
        buffers.append(r)
    if any(len(r) > 0x7fffffff for r in buffers):
        raise ValueError("png_deflate: a buffer has at most 2^31-1 bytes")
    tensors = [r for r in buffers if torch.is_tensor(r)]
    device = _decode_device("png_deflate", tensors[0].device if tensors and device is None else device)
    if not buffers:
        return []
    with torch.cuda.device(device):
        sizes = [len(r) for r in buffers]
        pitch = -(-max(max(sizes), 1) // 4) * 4
        if tensors:
            raw = torch.zeros((len(buffers), pitch), dtype=torch.uint8, device=device)
            for i, r in enumerate(buffers):
                raw[i, :sizes[i]] = r if torch.is_tensor(r) else torch.from_numpy(r.copy()).to(device)
        else:  # ONE upload
            host = np.zeros((len(buffers), pitch), np.uint8)
            for i, r in enumerate(buffers):
                host[i, :sizes[i]] = r
            raw = torch.from_numpy(host).to(device)
        out, lengths = _png_deflate(raw, torch.tensor(sizes, dtype=torch.int64).to(device), max(sizes))
        return _png_fetch(out, lengths, out.shape[1])


def _png_chunk(name, body):
    return len(body).to_bytes(4, "big") + name + body + zlib.crc32(name + body).to_bytes(4, "big")


def to_png(x):
    """`Image.fromarray(x).save(fp, format="PNG")` of images on the GPU, up to the compressed bytes: uint8 [H,W,C] -> bytes, uint8
    [B,H,W,C] -> a list of B bytes (`[]` for B = 0).  C = 1, 2, 3, 4 give PNG colour types 0, 4, 2, 6 at 8 bits: Pillow's modes L, LA,
    RGB, RGBA.  The file is non-interlaced, with one IDAT and no ancillary chunk.  Its IDAT inflates to Pillow's filtered rows byte for
    byte -- the same filter for every row -- so any reader gets the pixels back exactly; the compressed bytes are this library's own
    (`png_deflate`), within a few per cent of Pillow's size on photographs and labels (DESIGN.md "K17e").  Three launches for the whole
    batch; what crosses to the host is the compressed data and the lengths, in ONE copy as long as no image compresses to more than
    5/8 of its filtered size; past that (noise) a second copy fetches the rest.  The host adds the signature, IHDR, the IDAT framing
    with its CRC and IEND.
    Out of scope: palette and sub-8-bit output, 16 bits, interlacing, ancillary chunks, matches across the 32 KiB chunks, Pillow's
    `optimize` and `compress_level`."""
    x4 = _png_encode_input("to_png", x)
    b, h, w, c = x4.shape
    if b == 0:
        return []
    with torch.cuda.device(x4.device):
        plan = png_encode_plan(b, h, w, c)
        raw = _png_filter(x4, plan)
        sizes = torch.full((b,), plan["size"], dtype=torch.int64, device=x4.device)
        out, lengths = _png_deflate(raw, sizes, plan["size"])
        streams = _png_fetch(out, lengths, plan["size"] * _PNG_GUESS[0] // _PNG_GUESS[1] + 1024)
    head = _PNG_SIGNATURE + _png_chunk(b"IHDR", w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes((8, _PNG_COLOUR_OF_CHANNELS[c], 0, 0, 0)))
    tail = _png_chunk(b"IEND", b"")
    files = [head + _png_chunk(b"IDAT", z) + tail for z in streams]
    return files[0] if x.ndim == 3 else files


def save_png(x, fp, nrow=8, padding=2, value_range=(-1, 1), pad_value=0.0):
    """`torchvision.utils.save_image(x, "name.png", nrow=, padding=, normalize=True, range=value_range, pad_value=)` (0.8.2): fp32
    [B,C,H,W] (C = 1 or 3) on the GPU -> to_bytes' canvas -> to_png -> the file.  fp: a path ending in .png, or an object with write().
    The decoded file is the canvas exactly; see `to_png` for what is in and out of scope."""
    if isinstance(fp, (str, os.PathLike)):
        if os.path.splitext(os.fspath(fp))[1].lower() != ".png":
            raise ValueError(f"save_png: {os.fspath(fp)!r} does not end in .png (JPEG goes through save_image)")
    elif not hasattr(fp, "write"):
        raise ValueError(f"save_png: fp is a path ending in .png or an object with write() (got {type(fp).__name__})")
    data = to_png(to_bytes(x, value_range=value_range, nrow=nrow, padding=padding, pad_value=pad_value, grid=True))
    if hasattr(fp, "write"):
        fp.write(data)
    else:
        with open(fp, "wb") as f:
            f.write(data)


def clear_caches():
    """Drop the device copies of the coefficient, normalisation and Huffman tables (they are small; this is for tests and device
    resets)."""
    _DEVICE_TABLES.clear(), _NORM_TABLES.clear(), _HUFF_TABLES.clear()
