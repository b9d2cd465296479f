"""Numpy restatement of the image I/O arithmetic (include/w2e_image.h), written from the published sources -- Pillow's
src/libImaging/Resample.c (8 bits per channel) and torchvision 0.8.2's utils.make_grid / save_image -- not from the kernels or from
where2edit_amd/image_io.py.  tests/test_image_io_host.py holds it against Pillow itself (where it imports), against the committed
Pillow outputs of tests/golden/image_io.npz and against the torch CPU op sequence; the GPU tests hold the kernels against it."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
ONE = 1 << PRECISION_BITS

# (B, C, in_h, in_w, out_h, out_w): what each case exercises is listed in tests/test_gpu_image_io.py
SHAPES = (
    (1, 3, 5, 5, 1, 1),
    (2, 1, 2, 3, 5, 4),
    (1, 3, 9, 7, 16, 16),
    (2, 3, 37, 53, 16, 16),
    (1, 3, 16, 16, 16, 8),
    (1, 1, 16, 24, 4, 24),
    (1, 3, 64, 64, 64, 64),
    (1, 1, 100, 75, 32, 33),
    (1, 3, 200, 520, 50, 130),
    (1, 3, 300, 200, 7, 11),
    (2, 1, 512, 512, 64, 64),
    (2, 3, 1024, 1024, 256, 256),
)
SMALL_SHAPES = tuple(s for s in SHAPES if s[2] <= 100 and s[3] <= 100)  # the cases the committed fixture holds
PATTERNS = ("random", "ones", "zeros", "checker")


def pattern(name, shape, seed=0):
    """uint8 [B,H,W,C] test input: seeded random bytes / all 255 (the accumulator's peak: sum(K) may exceed 2^22) / all 0 / a
    one-pixel 0-255 checkerboard (the largest swing between neighbouring taps)."""
    b, c, h, w = shape[:4]
    if name == "random":
        return np.random.RandomState(1000 + seed).randint(0, 256, size=(b, h, w, c)).astype(np.uint8)
    if name == "ones":
        return np.full((b, h, w, c), 255, np.uint8)
    if name == "zeros":
        return np.zeros((b, h, w, c), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8)[None, :, :, None], (b, h, w, c)).copy()


def block_label(grid_ids, block):
    """A parsing label made of block x block squares: ids [G,G] -> uint8 [G * block, G * block]."""
    return np.kron(np.asarray(grid_ids, np.uint8), np.ones((block, block), np.uint8))


def label_grid(seed=7, g=16):
    """The 16 x 16 id grid (ids 0..18) of the 512^2 label case."""
    return np.random.RandomState(seed).randint(0, 19, size=(g, g)).astype(np.uint8)


def _triangle(t):
    t = -t if t < 0.0 else t
    return 1.0 - t if t < 1.0 else 0.0


def axis_tables(in_size, out_size, filter="bilinear"):
    """precompute_coeffs + normalize_coeffs_8bpc for one axis: (K int32 [out, ksize], bounds int32 [out, 2] = (xmin, n))."""
    scale = float(in_size) / float(out_size)
    if filter == "nearest":
        idx = [min(int((xx + 0.5) * scale), in_size - 1) for xx in range(out_size)]
        return np.full((out_size, 1), ONE, np.int32), np.array([[i, 1] for i in idx], np.int32)
    assert filter == "bilinear"
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    kk = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [_triangle((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * ONE) if k < 0 else int(0.5 + k * ONE)
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass(img, axis, kk, bounds):
    """One pass over `axis` (1 = rows / vertical, 2 = columns / horizontal) of uint8 [B,H,W,C]."""
    out_size = kk.shape[0]
    shape = list(img.shape)
    shape[axis] = out_size
    out = np.empty(shape, np.uint8)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    dst = np.moveaxis(out, axis, 0)
    for o in range(out_size):
        first, n = int(bounds[o, 0]), int(bounds[o, 1])
        acc = np.full(src.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for t in range(n):
            acc += src[first + t] * int(kk[o, t])
        assert acc.max() < 2 ** 31 and acc.min() >= -2 ** 31  # the kernels accumulate in int32
        dst[o] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img, out_h, out_w, filter="bilinear"):
    """Image.resize((out_w, out_h), filter) of every image of uint8 [B,H,W,C]: horizontal pass first, into bytes, then the vertical
    pass; an axis whose size does not change is not passed."""
    img = np.ascontiguousarray(img, np.uint8)
    _, h, w, _ = img.shape
    if w != out_w:
        img = _pass(img, 2, *axis_tables(w, out_w, filter))
    if h != out_h:
        img = _pass(img, 1, *axis_tables(h, out_h, filter))
    return img


def normalize_table(mean, std, channels):
    """[channels, 256] float32: ToTensor (v / 255 in fp32) then Normalize ((t - mean) / std in fp32)."""
    mean = np.broadcast_to(np.asarray(mean, np.float32), (channels,))
    std = np.broadcast_to(np.asarray(std, np.float32), (channels,))
    t = np.arange(256, dtype=np.float32) / np.float32(255)
    return ((t[None, :] - mean[:, None]) / std[:, None]).astype(np.float32)


def to_tensor(img_u8, mean, std):
    """uint8 [B,H,W,C] -> float32 [B,C,H,W] through the table."""
    c = img_u8.shape[3]
    lut = normalize_table(mean, std, c)
    return np.stack([lut[ch][img_u8[..., ch]] for ch in range(c)], 1)


def quantise_unit(t):
    """save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8) of float32 `t`, each step rounded to fp32; NaN -> 0."""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (t * np.float32(255)).astype(np.float32) + np.float32(0.5)
        q = np.minimum(np.maximum(q.astype(np.float32), np.float32(0)), np.float32(255))
        return np.where(np.isnan(q), 0, np.trunc(np.nan_to_num(q))).astype(np.uint8)


def quantise(x, lo=-1.0, hi=1.0, eps=1e-5):
    """make_grid's norm_ip + save_image's quantisation of float32 `x` (any shape)."""
    x = np.asarray(x, np.float32)
    d = np.float32(float(hi) - float(lo) + eps)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.minimum(np.maximum(x, np.float32(lo)), np.float32(hi))  # (np.minimum / maximum propagate NaN, as clamp_ does)
        t = ((v + np.float32(-lo)).astype(np.float32) / d).astype(np.float32)
    return quantise_unit(t)


def to_bytes(x, lo=-1.0, hi=1.0, nrow=8, padding=2, pad_value=0.0, grid=True, eps=1e-5):
    """float32 [B,C,H,W] -> uint8 HWC canvas (grid) or [B,H,W,C]."""
    x = np.asarray(x, np.float32)
    b, c, h, w = x.shape
    q = quantise(x, lo, hi, eps)
    if not grid:
        return np.ascontiguousarray(q.transpose(0, 2, 3, 1))
    if c == 1:
        q = np.concatenate([q, q, q], 1)
    if b == 1:
        return np.ascontiguousarray(q[0].transpose(1, 2, 0))
    xmaps = min(nrow, b)
    ymaps = int(math.ceil(float(b) / xmaps))
    ch, cw = h + padding, w + padding
    canvas = np.full((ymaps * ch + padding, xmaps * cw + padding, 3), quantise_unit(np.float32(pad_value)), np.uint8)
    k = 0
    for y in range(ymaps):
        for xg in range(xmaps):
            if k >= b:
                break
            canvas[y * ch + padding:y * ch + padding + h, xg * cw + padding:xg * cw + padding + w] = q[k].transpose(1, 2, 0)
            k += 1
    return canvas


def boundary_set(lo, hi, eps=1e-5, seed=5, n_random=100000):
    """float32 inputs around every rounding boundary of the quantiser: lo + d (k + 0.5) / 255 rounded to fp32 with its three fp32
    neighbours on either side (k = 0..255), lo, hi, +-5, +-inf, NaN, and `n_random` seeded uniform values a little wider than the
    range."""
    d = float(hi) - float(lo) + eps
    pts = [np.float32(lo + d * (k + 0.5) / 255) for k in range(256)]
    vals = []
    for p in pts:
        down = up = p
        vals.append(p)
        for _ in range(3):
            down, up = np.nextafter(down, np.float32(-np.inf)), np.nextafter(up, np.float32(np.inf))
            vals += [down, up]
    vals += [np.float32(v) for v in (lo, hi, 5, -5, np.inf, -np.inf, np.nan)]
    width = float(hi) - float(lo)
    rnd = np.random.RandomState(seed).uniform(lo - 0.05 * width, hi + 0.05 * width, size=n_random).astype(np.float32)
    return np.concatenate([np.array(vals, np.float32), rnd])
