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

Decoding and encoding (JPEG, PNG) stay with the caller.  GPU only: there is no CPU fallback (tests/imageio_ref.py is the numpy
restatement the kernels are tested against)."""
import ctypes
import functools
import math

import torch

from ._lib import call, stream_ptr

PRECISION_BITS = 22  # W2E_IMAGE_PRECISION_BITS
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


def clear_caches():
    """Drop the device copies of the coefficient and normalisation tables (they are small; this is for tests and device resets)."""
    _DEVICE_TABLES.clear(), _NORM_TABLES.clear()
