"""torch.autograd.Functions over the C ABI of libw2e.so (include/w2e.h).

PyTorch is plumbing here: it owns the device memory (outputs are torch.empty on the input's device),
the stream (kernels are enqueued on torch's current HIP stream) and the autograd tape.  All arithmetic
on image-sized tensors happens in the HIP kernels; torch ops are used only on [B,C]-sized style math.
"""
import ctypes
import functools
import math
import os

import torch
from torch.autograd.function import once_differentiable

from . import _lib, profiling
from ._lib import CONSTS, call, ptr, stream_ptr

SQRT2 = math.sqrt(2.0)

# ---- "the first n samples of the batch carry no gradient".  Coach runs x = G(w) (no grad) and x_hat = G(w_hat) as ONE
# generator pass over the batch [w; w_hat] (twice the rows per launch: the same kernels run ~9 % faster per image at twice
# the batch); the backward of every generator node then works on the rows [n:] only -- the saved activations and the incoming
# gradient are batch-major, so the slices are contiguous views -- and leaves rows [:n] of the gradients it returns
# unwritten: nothing reads them (each node's only producers / consumers are nodes that slice the same way).
_NOGRAD_PREFIX = 0
# Debug aid (W2E_DEBUG_POISON=1 / set_debug_poison): the prefix rows that the nodes above leave unwritten are filled with NaN,
# so that a consumer which DOES read them (a stock op slipped between `both` and a generator node, a node that forgot to slice)
# turns the loss / gradients into NaN instead of silently using uninitialised memory.  One fill per buffer: off by default.
_POISON = os.environ.get("W2E_DEBUG_POISON", "0") == "1"


def set_debug_poison(on=True):
    global _POISON
    _POISON = bool(on)


def _grad_rows(shape, n_skip, device, like=None):
    """An uninitialised full-batch gradient buffer whose rows [n_skip:] a kernel is about to write (rows [:n_skip] belong to the
    no-grad half of a merged pass: unwritten by design, NaN under the debug option)."""
    buf = torch.empty(shape, device=device, dtype=torch.float32) if like is None else torch.empty_like(like)
    if _POISON and n_skip:
        buf[:n_skip].fill_(float("nan"))
    return buf


class nograd_prefix:
    def __init__(self, n):
        self.n = int(n)

    def __enter__(self):
        global _NOGRAD_PREFIX
        self.prev, _NOGRAD_PREFIX = _NOGRAD_PREFIX, self.n
        return self

    def __exit__(self, *exc):
        global _NOGRAD_PREFIX
        _NOGRAD_PREFIX = self.prev


class _TailRows(torch.autograd.Function):
    """x[n:] of a batch whose first n rows carry no gradient (the merged generator pass): the backward hands the producer a
    full-batch buffer whose tail holds the gradient and whose first n rows are unwritten -- every generator node slices them off
    (`nograd_prefix`) -- instead of autograd's zero-fill of the whole batch + copy (SliceBackward)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.full = n, x.shape[0]
        return x[n:]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        out = _grad_rows((ctx.full,) + tuple(g.shape[1:]), ctx.n, g.device)
        out[ctx.n:].copy_(g)
        return out, None


def tail_rows(x, n):
    return _TailRows.apply(x, n)


class GradPool:
    """Zeroed scratch for the [B,C]-sized gradient accumulators of ONE generator pass: its backward nodes (17 StyledConv style
    gradients, 9 ToRGB ones, the W+ gradient) carve their buffers out of one zero-filled tensor -- one fill launch instead of 27.
    Created per pass by `grad_pool` (the buffer itself on first use, in the backward), handed out once per region, never reused:
    nothing is shared between steps or between graph captures."""

    __slots__ = ("buf", "off", "hint")

    def __init__(self, hint):
        self.buf, self.off, self.hint = None, 0, int(hint)

    def zeros(self, shape, device):
        n = 1
        for v in shape:
            n *= int(v)
        n_al = (n + 63) & ~63  # 256-byte granules: float4 / b128 accesses of the consumers stay aligned
        if self.buf is None or self.off + n_al > self.buf.numel() or self.buf.device != torch.device(device):
            self.buf, self.off = torch.zeros(max(n_al, self.hint), device=device, dtype=torch.float32), 0
        out = self.buf[self.off:self.off + n].view(shape)
        self.off += n_al
        return out


_GRAD_POOL = None


class grad_pool:
    """`with grad_pool(hint_floats):` -- the autograd nodes created inside share one GradPool for their small zeroed gradients."""

    def __init__(self, hint):
        self.pool = GradPool(hint)

    def __enter__(self):
        global _GRAD_POOL
        self.prev, _GRAD_POOL = _GRAD_POOL, self.pool
        return self.pool

    def __exit__(self, *exc):
        global _GRAD_POOL
        _GRAD_POOL = self.prev
        return False


def _zeros_with_tail(full, n, tail_shape, device, pool=None):
    """-> (buf, tail): a zeroed [full, *tail_shape] fp32 buffer and its rows [n:] (a contiguous view) for a kernel to write:
    the [B,C]-sized gradients of a node inside `nograd_prefix` in one fill, no concatenation.  `pool`: the pass's GradPool."""
    shape = (full,) + tuple(tail_shape)
    buf = pool.zeros(shape, device) if pool is not None else torch.zeros(shape, device=device, dtype=torch.float32)
    return buf, (buf[n:] if n else buf)


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------ K2
def _upfirdn2d_raw(x, kernel, out_h, out_w, up, down, pad_x0, pad_y0, flip, act=None, planar_hw=None, out=None):
    """One launch of w2e_upfirdn2d.  `act` = (out_scale[planes]|None, noise[HW]|None, noise_w|None, bias[C]|None).
    planar_hw=(in_h, in_w): x is the phase-planar [N,C,2,2,(in_h+1)/2,(in_w+1)/2] image the UP conv writes.
    `out`: a contiguous [n,c,out_h,out_w] tensor to write (e.g. the tail rows of a larger batch) instead of allocating."""
    n, c = x.shape[0], x.shape[1]
    h, w = planar_hw if planar_hw is not None else (x.shape[2], x.shape[3])
    if planar_hw is not None and tuple(x.shape[2:]) != (2, 2, (h + 1) // 2, planar_pitch((w - 1) // 2)):
        raise RuntimeError(f"upfirdn2d: a phase-planar input of a {h}x{w} image must be [N,C,2,2,{(h + 1) // 2},{planar_pitch((w - 1) // 2)}] "
                           f"(W2E_PLANAR_PITCH, include/w2e.h), got {tuple(x.shape)}")
    kh, kw = kernel.shape
    y = out if out is not None else torch.empty((n, c, out_h, out_w), device=x.device, dtype=torch.float32)
    if act is None:
        a = (0, None, None, None, None, 1, 0.2, SQRT2)
    else:
        out_scale, noise, noise_w, bias = act
        a = (1, ptr(out_scale), ptr(noise), ptr(noise_w), ptr(bias), c, 0.2, SQRT2)
    sp = profiling.span("upfirdn2d", 4.0 * n * c * (h * w + out_h * out_w))  # algorithmic bytes: read x + write y
    call("w2e_upfirdn2d", ptr(x), ptr(kernel), ptr(y), n * c, h, w, out_h, out_w, kh, kw, up, down, pad_x0, pad_y0,
         int(flip), int(planar_hw is not None), x.shape[-1] if planar_hw is not None else 0, *a, stream_ptr())
    if sp is not None:
        sp.end()
    return y


_FirPlanFields = ctypes.c_int64 * CONSTS["W2E_FIR_PLAN_FIELDS"]


def upfirdn_plan(planes, in_hw, out_hw, kernel_shape, up=1, down=1, pad_x0=0, planar=False, act=False, x_misalign=0, y_misalign=0):
    """w2e_upfirdn2d_plan (include/w2e.h): [kernel, act, planar, grid, block, lds, arg0, arg1, arg2] of the launch w2e_upfirdn2d would
    make -- kernel: 0 generic, 1 down4, 2 tile, 3 tile4, 4 blur4, 5 stream4 (W2E_FIR_*).  A launch it refuses raises its message."""
    out = _FirPlanFields()
    call("w2e_upfirdn2d_plan", planes, *in_hw, *out_hw, *kernel_shape, up, down, pad_x0, int(planar),
         planar_pitch((in_hw[1] - 1) // 2) if planar else 0, int(act), x_misalign, y_misalign, out)
    return out[:]


def fir_planar_ok(kernel_shape, out_w):
    """Whether w2e_upfirdn2d reads the UP conv's phase-planar image directly for an up = down = 1 FIR of these taps onto `out_w` columns
    (w2e_upfirdn2d_planar_ok); where it does not, the caller re-interleaves the image first (unplanar)."""
    return bool(_lib.load().w2e_upfirdn2d_planar_ok(kernel_shape[0], kernel_shape[1], 1, 1, out_w))


class _UpFirDn2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kernel, up, down, pad0, pad1):
        x = _c(x)
        kernel = _c(kernel.to(torch.float32))
        n, c, h, w = x.shape
        kh, kw = kernel.shape
        out_h = (h * up + pad0 + pad1 - kh) // down + 1
        out_w = (w * up + pad0 + pad1 - kw) // down + 1
        if out_h <= 0 or out_w <= 0:
            raise RuntimeError(f"upfirdn2d: empty output {out_h}x{out_w}")
        ctx.save_for_backward(kernel)
        ctx.geom = (h, w, up, down, pad0)
        return _upfirdn2d_raw(x, kernel, out_h, out_w, up, down, pad0, pad0, True)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (kernel,) = ctx.saved_tensors
        h, w, up, down, pad0 = ctx.geom
        kh, kw = kernel.shape
        # adjoint: swap up/down, un-flipped taps, leading pad k-1-pad0, output cropped to the input size
        gx = _upfirdn2d_raw(_c(gy), kernel, h, w, down, up, kw - 1 - pad0, kh - 1 - pad0, False)
        return gx, None, None, None, None, None


def upfirdn2d(input, kernel, up=1, down=1, pad=(0, 0)):
    """models/stylegan2/op/upfirdn2d.py:11 -- same signature and semantics, HIP kernel underneath."""
    return _UpFirDn2d.apply(input, kernel, up, down, pad[0], pad[1])


# ------------------------------------------------------------------------------------------ K3
class _BiasAct(torch.autograd.Function):
    """y = lrelu(x + bias (+ w*noise), slope) * gain with x viewed as [outer, C, inner]."""

    @staticmethod
    def forward(ctx, x, bias, slope, gain, channel_last):
        x = _c(x)
        bias = _c(bias)
        if channel_last:
            outer, ch, inner = x.numel() // x.shape[-1], x.shape[-1], 1
        else:
            outer, ch, inner = x.shape[0], x.shape[1], x.numel() // (x.shape[0] * x.shape[1])
        if bias.numel() != ch:
            raise RuntimeError(f"fused_leaky_relu: bias has {bias.numel()} entries, expected {ch}")
        y = torch.empty_like(x)
        call("w2e_bias_act_fwd", ptr(x), ptr(bias), None, None, ptr(y), outer, ch, inner, slope, gain, stream_ptr())
        ctx.save_for_backward(y)
        ctx.cfg = (slope, gain, channel_last, ch)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        slope, gain, channel_last, ch = ctx.cfg
        gy = _c(gy)
        gx = torch.empty_like(y)
        call("w2e_bias_act_bwd", ptr(gy), ptr(y), ptr(gx), y.numel(), slope, gain, stream_ptr())
        gb = None
        if ctx.needs_input_grad[1]:
            gb = gx.reshape(-1, ch).sum(0) if channel_last else gx.reshape(gx.shape[0], ch, -1).sum((0, 2))
        return gx, gb, None, None, None


def fused_leaky_relu(input, bias, negative_slope=0.2, scale=2 ** 0.5):
    """models/stylegan2/op/fused_act.py:23 -- bias on dim 1, except 3-D inputs (bias on the last dim).
    No device move inside the op (the reference's `input.cuda()` is a bug on CPU boxes, Q1)."""
    if input.ndim < 2:
        raise RuntimeError("fused_leaky_relu expects at least 2 dims")
    channel_last = input.ndim == 3 or input.ndim == 2
    return _BiasAct.apply(input, bias, float(negative_slope), float(scale), channel_last)


# ------------------------------------------------------------------------------------------ K1
def conv_pack(weight, scale, transpose, flip):
    """weight [Cout,Cin,3,3] -> [ceil(K/8)][9][2][N][4] (w2e_conv_pack): K the reduced, N the produced channels."""
    cout, cin = weight.shape[0], weight.shape[1]
    kd, nd = (cout, cin) if transpose else (cin, cout)
    wp = torch.empty(((kd + 7) // 8, 9, 2, nd, 4), device=weight.device, dtype=torch.float32)
    call("w2e_conv_pack", ptr(_c(weight.detach())), ptr(wp), cout, cin, float(scale), int(transpose), int(flip),
         stream_ptr())
    return wp


MODE_SAME, MODE_UP, MODE_DOWN = (CONSTS[f"W2E_CONV_{m}"] for m in ("SAME", "UP", "DOWN"))

# ---- Winograd F(4x4,3x3) forms of the same-resolution layers (include/w2e.h, K1w / K1g).  Two own kernels, no vendor GEMM:
#   form 4      the GEMM form for the WIDE layers: w2e_wino_pack_input (V in MFMA operand order) -> w2e_wino_gemm (the 36 contractions on fp32
#               MFMA, operands L2 -> registers, the output transform and the direct kernel's epilogues in its epilogue: M never reaches HBM)
#   form FUSED  w2e_wino_fused for the narrow high-resolution layers (nothing transform-domain in HBM at all)
# WINOGRAD (W2E_WINOGRAD, read once here):
#   "auto"  per layer, what measured fastest: the library's choice (w2e_wino_plan in csrc/winogemm.hip holds the thresholds and the
#           shape rules of both forms; up-sampling layers always run the direct kernels).  Rounding ~1e-5 relative (direct: 3e-7)
#   False   direct kernels only ("0");  4 / 8: that form wherever the shapes allow (tests, tools)
def _parse_winograd(v):
    table = {"": "auto", "auto": "auto", "0": False, "4": 4, "8": 8}
    if v not in table:  # (a typo used to mean "auto": a user asking for the exact direct kernels got the 1e-5 forms silently)
        raise ValueError(f"W2E_WINOGRAD={v!r}: expected 'auto', '0' (direct kernels), '4' (GEMM form) or '8' (fused form)")
    return table[v]


WINOGRAD = _parse_winograd(os.environ.get("W2E_WINOGRAD", ""))
WINO_LOG = None  # a list: every Winograd-form conv appends one line in the format of the library's tune_print (tests, tools/cfg_selections.py)


FUSED = 8  # form code of the fused F(4x4,3x3) kernel (w2e_wino_fused)


def set_winograd(mode):
    """mode: "auto" | False | 4 | 8 (4: the GEMM form, 8: the fused F(4x4,3x3) kernel, each wherever its shapes allow)"""
    global WINOGRAD
    if mode not in ("auto", False, 4, 8):
        raise ValueError("set_winograd: 'auto', False, 4 or 8")
    WINOGRAD = mode


FUSED_WGS = 0    # > 0: cap of the fused kernel's persistent grid (tests)
GEMM_SPLITS = 0  # > 0: force w2e_wino_gemm's K split (tests); 0: the library's plan

GENERATOR, ENCODER = CONSTS["W2E_WINO_GENERATOR"], CONSTS["W2E_WINO_ENCODER"]  # whose selection policy
EPI_PLAIN, EPI_ACT, EPI_PRELU, EPI_DOT = (CONSTS[f"W2E_WINO_EPI_{e}"] for e in ("PLAIN", "ACT", "PRELU", "DOT"))  # the first three are the launchers' `act`


_WinoPlanFields = ctypes.c_int64 * CONSTS["W2E_WINO_PLAN_FIELDS"]


def wino_plan(family, b, k, n, h, w, epilogue=EPI_PLAIN, request=None, fused_allowed=True):
    """w2e_wino_plan (include/w2e.h): [form, fits_gemm, fits_fused, tiles_padded, splits, workspace_floats] for one W2E_CONV_SAME call --
    0 (direct kernel), 4 (the GEMM form: w2e_wino_pack_input + w2e_wino_gemm) or FUSED (w2e_wino_fused), whether each form fits the shape
    at all, and the GEMM form's arguments.  The shape rules and both families' policies live in the library; `request`: None = WINOGRAD."""
    out = _WinoPlanFields()
    request = WINOGRAD if request is None else request
    call("w2e_wino_plan", family, -1 if request == "auto" else int(request), fused_allowed, epilogue, b, k, n, h, w, GEMM_SPLITS, out)
    return out[:]


def _wino_form(x, k, n, h, w, dot_with):
    """0, 4 or FUSED for one W2E_CONV_SAME call of the generator."""
    return wino_plan(GENERATOR, x.shape[0], k, n, h, w, EPI_PLAIN if dot_with is None else EPI_DOT)[0]


def _wino_weights_fused(wp, k, n):
    uf = getattr(wp, "_w2e_wino_uf", None)
    if uf is None:
        uf = torch.empty((36, k // 8, 2, n, 4), device=wp.device, dtype=torch.float32)
        call("w2e_wino_weights_fused", ptr(wp), ptr(uf), k, n, stream_ptr())
        wp._w2e_wino_uf = uf
    return uf


def wino_conv(m, x, wp, in_scale, out_scale, y, k, n, h, w, act_code=0, noise=None, noise_w=None, bias=None, slope=None,
              dot_with=None, dot=None, tag="modconv mode 0", plan=None):
    """One same-resolution 3x3 conv in Winograd form m: FUSED (K1w, w2e_wino_fused) or 4 (K1g, w2e_wino_pack_input -> w2e_wino_gemm with
    the tiles / K split / workspace of `plan`, a wino_plan() result; None: asked for here).  `dot` [b,n] receives the fused dot when
    dot_with is given (summed in a fixed order, no atomics).  A shape the form does not take is refused by its launcher."""
    b = x.shape[0]
    dot_txt = ", dot" if dot_with is not None else ""
    if m == FUSED:
        nblk = (h // 16) * (w // 32)
        if WINO_LOG is not None:  # (the encoders' line never carried the block count; recorded selections are compared byte for byte)
            WINO_LOG.append(f"{tag} (winograd F(4x4,3x3) fused{dot_txt}) K {k} N {n} {h}x{w} B {b}"
                            + (f" -> {b * nblk} blocks of 32 tiles" if tag == "modconv mode 0" else ""))
        # the fused dot leaves one partial per (spatial block, channel): summed below, in a fixed order
        part = torch.empty((b, n, nblk), device=x.device, dtype=torch.float32) if dot_with is not None else None
        call("w2e_wino_fused", ptr(x), ptr(in_scale), ptr(_wino_weights_fused(wp, k, n)), ptr(out_scale), ptr(y), b, k, n, h, w,
             act_code, ptr(noise), ptr(noise_w), ptr(bias), ptr(slope), ptr(dot_with), ptr(part), FUSED_WGS, stream_ptr())
        if part is not None:
            # (a kernel, not aten::sum: that one memsets under capture.)  `dot` arrives zeroed and nothing else adds to it before this
            # call returns -- the partial sums ARE its value: written in place (round 3 summed into a temporary and added that: 2 more launches)
            call("w2e_channel_sums", ptr(part), None, ptr(dot), b, n, nblk, stream_ptr())
        return
    _, _, _, tp, splits, ws_floats = plan or wino_plan(ENCODER, b, k, n, h, w, EPI_DOT if dot_with is not None else act_code, 4)
    if WINO_LOG is not None:
        WINO_LOG.append(f"{tag} (winograd F(4x4,3x3) gemm{dot_txt}) K {k} N {n} {h}x{w} B {b} -> "
                        f"36 x [{n}x{k}] x [{k}x{tp}], {splits} K split(s)")
    vf = torch.empty(36 * k * tp, device=x.device, dtype=torch.float32)
    work = torch.empty(ws_floats, device=x.device, dtype=torch.float32) if (splits > 1 or dot_with is not None) else None
    st = stream_ptr()
    call("w2e_wino_pack_input", ptr(x), ptr(in_scale), ptr(vf), b, k, h, w, tp, st)
    call("w2e_wino_gemm", ptr(_wino_weights_fused(wp, k, n)), ptr(vf), ptr(out_scale), ptr(y), b, k, n, h, w, tp, splits, ptr(work),
         act_code, ptr(noise), ptr(noise_w), ptr(bias), ptr(slope), ptr(dot_with), ptr(dot), st)


wino_gemm_conv = functools.partial(wino_conv, 4)  # (x, wp, in_scale, out_scale, y, k, n, h, w, ...): the GEMM form alone (tests)


def _modconv_raw(mode, x, wp, in_scale, out_scale, h, w, act=None, dot_with=None, out=None, dot_out=None):
    """One call of w2e_modconv3x3.  h,w: input size for SAME/UP, output size for DOWN.  `out`: write into this
    (contiguous, [b,n,h,w]) tensor -- e.g. the tail rows of a larger batch -- instead of allocating; `dot_out`: likewise a
    ZEROED [b,n] tensor for the fused per-channel dot (accumulated with atomics)."""
    b, k = x.shape[0], x.shape[1]
    n = wp.shape[3]
    if wp.shape[0] != (k + 7) // 8:
        raise RuntimeError(f"modconv: packed weight holds {wp.shape[0]} 8-channel groups, input has {k} channels")
    if mode == MODE_UP:  # phase-planar T: T[Y][X] = y[Y&1][X&1][Y>>1][X>>1]  (unit-stride stores per output phase)
        y = torch.empty((b, n, 2, 2, h + 1, planar_pitch(w)), device=x.device, dtype=torch.float32)  # sector-aligned rows
    elif out is not None:
        y = out
    else:
        y = torch.empty((b, n, h, w), device=x.device, dtype=torch.float32)
    dot = None
    if dot_with is not None:
        dot = dot_out if dot_out is not None else torch.zeros((b, n), device=x.device, dtype=torch.float32)
    noise = noise_w = bias = None
    if act is not None:
        noise, noise_w, bias = act
    # algorithmic FLOPs: 2*K*N*9 per domain pixel (MACs actually needed; SURVEY 2.3 convention)
    plan = wino_plan(GENERATOR, b, k, n, h, w, EPI_DOT if dot_with is not None else int(act is not None)) if mode == MODE_SAME else (0,)
    sp = profiling.span("modconv3x3_wino4" if plan[0] else "modconv3x3", 2.0 * b * k * n * 9 * h * w)
    if plan[0]:
        wino_conv(plan[0], x, wp, in_scale, out_scale, y, k, n, h, w, int(act is not None), noise, noise_w, bias, None, dot_with, dot, plan=plan)
    else:
        call("w2e_modconv3x3", mode, ptr(x), ptr(wp), ptr(in_scale), ptr(out_scale), ptr(y), b, k, n, h, w,
             y.shape[-1] if mode == MODE_UP else 0, int(act is not None), ptr(noise), ptr(noise_w), ptr(bias), ptr(dot_with), ptr(dot), stream_ptr())
    if sp is not None:
        sp.end()
    return y, dot


def _upblur_planned(b, k, n, h, w):
    """Whether the library takes an up-sampling StyledConv of this shape as ONE launch (w2e_modconv_upblur_plan: option tune_upblur,
    fp32 only, the layers it measured faster on)."""
    fused = ctypes.c_int(0)
    call("w2e_modconv_upblur_plan", b, k, n, h, w, ctypes.byref(fused))
    return bool(fused.value)


def _blur_actbwd_planned(planes, h, w, kernel_shape):
    """Whether the library takes the activation backward + adjoint blur of a [planes,h,w] gradient as ONE pass
    (w2e_blur_adjoint_actbwd_plan: the launcher's shape rules, not in deterministic mode, option tune_fuse)."""
    fused = ctypes.c_int(0)
    call("w2e_blur_adjoint_actbwd_plan", planes, h, w, kernel_shape[0], kernel_shape[1], ctypes.byref(fused))
    return bool(fused.value)


def _modconv_upblur_raw(x, wp, in_scale, out_scale, kernel, h, w, act):
    """One call of w2e_modconv_upblur: lrelu(blur(out_scale * conv_transpose(Wp, in_scale * x)) + nw*noise + bias) * sqrt2 as
    [b,n,2h,2w]; the (2h+1)x(2w+1) transposed-conv image is never written.  act = (noise, noise_w, bias)."""
    b, k = x.shape[0], x.shape[1]
    n = wp.shape[3]
    if wp.shape[0] != (k + 7) // 8:
        raise RuntimeError(f"modconv: packed weight holds {wp.shape[0]} 8-channel groups, input has {k} channels")
    noise, noise_w, bias = act
    y = torch.empty((b, n, 2 * h, 2 * w), device=x.device, dtype=torch.float32)
    sp = profiling.span("modconv3x3", 2.0 * b * k * n * 9 * h * w)  # algorithmic FLOPs: the recomputed halo is not useful work
    call("w2e_modconv_upblur", ptr(x), ptr(wp), ptr(in_scale), ptr(out_scale), ptr(kernel), ptr(y), b, k, n, h, w,
         ptr(noise), ptr(noise_w), ptr(bias), stream_ptr())
    if sp is not None:
        sp.end()
    return y


def _rgbfold_planned(b, k, n, h, w):
    """Whether the library takes the stride-2 input-gradient conv of this shape with the ToRGB backward folded into its epilogue
    (w2e_modconv_down_rgbfold_plan: option tune_rgbfold, the levels it measured faster on; never a split-K launch, deterministic mode,
    bf16x3 or a tile without that epilogue)."""
    fold = ctypes.c_int(0)
    call("w2e_modconv_down_rgbfold_plan", b, k, n, h, w, ctypes.byref(fold))
    return bool(fold.value)


def _modconv_down_rgbfold_raw(g, wp, in_scale, out_scale, h, w, x, gy, wrgb, style, noise, out=None, dot_out=None, sums3=None, gw=None):
    """One call of w2e_modconv_down_rgbfold (include/w2e.h K1f) -> (gpre, dot, sums3, gw).  g [b,k,2h+1,2w+1]; x [b,n,h,w]; gy [b,3,h,w];
    wrgb [3,n] with style [b,n], or [b,3,n] with style None; noise [h*w] or None.  `out`, `dot_out`, `sums3`, `gw`: write into these
    (the last three ZEROED: they are accumulated with atomics) instead of allocating."""
    b, k = g.shape[0], g.shape[1]
    n = wp.shape[3]
    if wp.shape[0] != (k + 7) // 8:
        raise RuntimeError(f"modconv: packed weight holds {wp.shape[0]} 8-channel groups, input has {k} channels")
    dev = g.device
    y = out if out is not None else torch.empty((b, n, h, w), device=dev, dtype=torch.float32)
    dot = dot_out if dot_out is not None else torch.zeros((b, n), device=dev, dtype=torch.float32)
    sums3 = sums3 if sums3 is not None else torch.zeros((b, n, 3), device=dev, dtype=torch.float32)
    gw = gw if gw is not None else torch.zeros((b, n) if style is not None else (b, 3, n), device=dev, dtype=torch.float32)
    sp = profiling.span("modconv3x3", 2.0 * b * k * n * 9 * h * w)
    call("w2e_modconv_down_rgbfold", ptr(g), ptr(wp), ptr(in_scale), ptr(out_scale), ptr(y), b, k, n, h, w, ptr(x), ptr(dot), ptr(gy),
         ptr(wrgb), ptr(style), ptr(noise), ptr(sums3), ptr(gw), 0.2, SQRT2, stream_ptr())
    if sp is not None:
        sp.end()
    return y, dot, sums3, gw


def _channel_dot(a, b, out=None):
    """[B,C] = sum_p a*b per plane (w2e_channel_sums: one wave per plane, fixed reduction order)."""
    n, c = a.shape[0], a.shape[1]
    if out is None:
        out = torch.empty((n, c), device=a.device, dtype=torch.float32)
    call("w2e_channel_sums", ptr(a), ptr(b), ptr(out), n, c, a.shape[2] * a.shape[3], stream_ptr())
    return out


def _scale_planes(a, s):
    """a[b,c,:,:] * s[b,c]  (w2e_se_apply_bwd with a zero offset)."""
    n, c = a.shape[0], a.shape[1]
    out = torch.empty_like(a)
    zero = torch.zeros((n, c), device=a.device, dtype=torch.float32)
    call("w2e_se_apply_bwd", ptr(a), ptr(_c(s)), ptr(zero), ptr(out), n, c, a.shape[2] * a.shape[3], stream_ptr())
    return out


def demod_coefficients(s, wsq, eps=1e-8):
    """d[b,o] = rsqrt(sum_i s[b,i]^2 wsq[o,i] + eps) (w2e_demod_fwd)."""
    b, cin = s.shape
    cout = wsq.shape[0]
    d = torch.empty((b, cout), device=s.device, dtype=torch.float32)
    call("w2e_demod_fwd", ptr(s), ptr(wsq), ptr(d), b, cin, cout, float(eps), stream_ptr())
    return d


def demod_coefficients_all(styles, wsqs, eps=1e-8):
    """[demod_coefficients(s, wsq) for s, wsq in zip(styles, wsqs)] in ONE launch (w2e_demod_all_fwd): the demodulation vectors of
    every layer of a generator pass, when the styles of all layers are known up front.  styles[j]: contiguous [B,cin_j]."""
    b = styles[0].shape[0]
    couts = [w.shape[0] for w in wsqs]
    buf = torch.empty(b * sum(couts), device=styles[0].device, dtype=torch.float32)
    descs = (_lib.DemodLayer * len(styles))()
    out, off = [], 0
    for j, (s, w) in enumerate(zip(styles, wsqs)):
        if s.shape != (b, w.shape[1]) or not s.is_contiguous() or not w.is_contiguous():
            raise RuntimeError(f"demod_coefficients_all: layer {j}: style {tuple(s.shape)} for wsq {tuple(w.shape)}")
        d = buf[off:off + b * couts[j]].view(b, couts[j])
        off += b * couts[j]
        descs[j].s, descs[j].wsq, descs[j].d, descs[j].cin, descs[j].cout = ptr(s).value, ptr(w).value, ptr(d).value, w.shape[1], couts[j]
        out.append(d)
    call("w2e_demod_all_fwd", descs, len(styles), b, float(eps), stream_ptr())
    return out


WGRAD_SAME, WGRAD_UP, WGRAD_CENTRE = 0, 1, 2


def modconv_wsq(weight, scale):
    """wsq [Cout,Cin] = sum_k (scale*W[o,i,k])^2 of a [1,Cout,Cin,k,k] weight (w2e_modconv_wsq): a kernel, so that a trained layer
    can rebuild it in every forward, inside a graph capture too."""
    cout, cin = weight.shape[1], weight.shape[2]
    wsq = torch.empty((cout, cin), device=weight.device, dtype=torch.float32)
    call("w2e_modconv_wsq", ptr(_c(weight.detach())), ptr(wsq), cout, cin, weight.shape[3] * weight.shape[4], float(scale), stream_ptr())
    return wsq


def modconv_wgrad(mode, g, x, d, s, weight, scale, sums=None, dz=None, noise_w=None, bias=None):
    """dL/dW [1,Cout,Cin,k,k] of a ModulatedConv2d (w2e_modconv_wgrad + w2e_modconv_wgrad_finish).  g: the pre-activation gradient
    ([B,Cout,h,w]; for WGRAD_UP the one on the (2h+1)x(2w+1) transposed-conv grid); x [B,Cin,h,w]; s [B,Cin]; d [B,Cout] or None
    (no demodulation); sums / dz: the demodulation-path coefficient exactly as w2e_demod_bwd takes it.  Always plain fp32."""
    b, cin, h, w = x.shape
    cout = weight.shape[1]
    taps = 1 if mode == WGRAD_CENTRE else 9
    splits = ctypes.c_int(0)
    call("w2e_modconv_wgrad_plan", mode, b, cin, cout, h, w, ctypes.byref(splits))
    slab = torch.empty(splits.value * taps * cout * cin, device=x.device, dtype=torch.float32)
    sp = profiling.span("modconv_wgrad", 2.0 * b * cin * cout * taps * h * w)
    st = stream_ptr()
    call("w2e_modconv_wgrad", mode, ptr(_c(g)), ptr(_c(x)), ptr(d), ptr(_c(s)), ptr(slab), b, cin, cout, h, w, splits.value, st)
    dw = torch.empty(weight.shape, device=x.device, dtype=torch.float32)
    if d is not None:
        call("w2e_modconv_wgrad_finish", ptr(slab), splits.value, ptr(_c(weight.detach())), ptr(sums), ptr(dz), ptr(noise_w), ptr(bias),
             ptr(d), ptr(_c(s)), ptr(dw), b, cin, cout, taps, float(scale), st)
    else:
        call("w2e_modconv_wgrad_finish", ptr(slab), splits.value, None, None, None, None, None, None, None, ptr(dw), b, cin, cout, taps,
             float(scale), st)
    if sp is not None:
        sp.end()
    return dw


def planar_pitch(w):
    """W2E_PLANAR_PITCH (include/w2e.h): row pitch of the phase planes of the transposed-conv output for an input w wide."""
    return (w + 1 + 15) & ~15


def unplanar(t, in_w):
    """[B,N,2,2,H+1,WP] phase-planar transposed-conv output (WP = W+1 padded to a multiple of 4) -> the plain
    [B,N,2H+1,2W+1] image."""
    b, n, _, _, hp, wpp = t.shape
    w = in_w
    return t.permute(0, 1, 4, 2, 5, 3).reshape(b, n, 2 * hp, 2 * wpp)[:, :, :2 * hp - 1, :2 * w + 1].contiguous()


class ActLink:
    """Pairs ONE fused StyledConv node with the ToRGB node that is the only consumer of its output (the pass-through form of the
    synthesis loop, or the last layer).  The ToRGB backward, which has the activation and the gradient it returns in registers,
    applies the StyledConv's activation backward itself (w2e_torgb_bwd_actbwd) and leaves the pre-activation gradient tensor and
    its three per-(sample, channel) sums here; the StyledConv backward takes them if -- and only if -- the gradient it receives
    is that very tensor (the engine hands it on untouched: nothing else contributes to it)."""

    __slots__ = ("noise", "gpre", "sums")

    def __init__(self, noise):
        self.noise, self.gpre, self.sums = noise, None, None

    def take(self, gout):
        gpre, sums = self.gpre, self.sums
        self.gpre = self.sums = None
        if gpre is None:
            return None  # the ToRGB node did not run its backward (its output was unused): the ordinary path
        if gpre is not gout:
            # The ToRGB backward has ALREADY applied this layer's activation backward to the gradient it returned, but what arrives
            # here is another tensor: a hook / retain_grad on the activation, a second consumer, or an engine-side copy or
            # accumulation changed it on the way.  Running the activation backward again would be silently wrong.
            raise RuntimeError("where2edit_amd: the gradient of a StyledConv output that was routed through its ToRGB node "
                               "(ActLink) reached the StyledConv backward as a different tensor -- a tensor hook, retain_grad() "
                               "or a second consumer on that activation is not supported on the fused training path "
                               "(use return_features=True / the unfused modules to tap activations)")
        return sums


class RgbFoldLink:
    """Joins the three backward nodes around one pass-through ToRGB node of the synthesis loop, level R: the ToRGB node of level 2R,
    whose backward produces that node's incoming RGB gradient (`gy`, recorded here); the up-sampling StyledConv of level 2R, whose
    stride-2 input-gradient conv writes the tensor the ToRGB(R) backward would read, add to and rewrite; and ToRGB(R) itself, which
    at forward time registers what its backward kernel would need (`saved`).  Autograd runs them in that order.  When the library
    takes the shape (w2e_modconv_down_rgbfold_plan) the StyledConv backward runs the folded launch (w2e_modconv_down_rgbfold): what
    it returns as its input gradient already IS the pre-activation gradient of the StyledConv below ToRGB(R), and it leaves that
    tensor, its three sums and the ToRGB style / weight gradient here.  ToRGB(R)'s backward then runs no kernel for them -- if, and
    only if, the two tensors it receives are those very tensors; the folded value cannot be un-folded, so anything else raises."""

    __slots__ = ("gy", "saved", "gpre", "sums", "gw")

    def __init__(self):
        self.gy = self.saved = self.gpre = self.sums = self.gw = None

    def usable(self, x, n_skip):
        """(StyledConv backward) both neighbours have reported, for this very activation and the same no-grad prefix."""
        if self.gy is None or self.saved is None:
            return False
        xs, _, _, _, ns = self.saved
        return ns == n_skip and xs.shape[0] == x.shape[0] + n_skip and xs.data_ptr() + 4 * n_skip * xs[0].numel() == x.data_ptr() \
            and tuple(xs.shape[1:]) == tuple(x.shape[1:]) and tuple(self.gy.shape) == (xs.shape[0], 3) + tuple(xs.shape[2:])

    def take(self, gy, gx_next):
        """(ToRGB backward) -> (gpre, sums, gw) of the folded launch, or None when it did not run."""
        gpre, sums, gw, rec = self.gpre, self.sums, self.gw, self.gy
        self.gpre = self.sums = self.gw = self.gy = None
        if gpre is None:
            return None
        if gx_next is not gpre or gy is not rec:
            raise RuntimeError("where2edit_amd: the ToRGB backward was folded into the stride-2 input-gradient conv of the level above "
                               "(RgbFoldLink), but the gradients reached the ToRGB node as different tensors -- a tensor hook, "
                               "retain_grad() or a second consumer on the passed-through activation or on the RGB skip image is not "
                               "supported on the fused training path (use return_features=True / the unfused modules to tap "
                               "activations, or the option tune_rgbfold = 0)")
        return gpre, sums, gw


class _StyledConv(torch.autograd.Function):
    """Fused StyledConv: out = lrelu(d * conv(Wp, s*x) [blur] + nw*noise + bias) * sqrt2 with
    d = rsqrt(s^2 @ wsq^T + eps) (model.py:234-276, 285-290, op/fused_act.py); with fuse_act=False just
    d * conv(Wp, s*x) [blur] (a bare ModulatedConv2d).  Differentiable in x, s (direct + demodulation paths in one
    gradient), noise_w, bias, the shared noise map [1,1,oh,ow] (w2e_noise_grad: noise_w times the plane sum of the pre-activation
    gradient, only when the map requires grad -- the projector's case; per-sample noise [B,1,H,W] with B > 1 never comes here, it keeps
    stylegan2.StyledConv's unfused composition, where autograd gives the gradient) and -- when the raw `weight` [1,Cout,Cin,k,k] is given (a layer opted in by
    stylegan2.train_conv_weights) -- in the conv weight (w2e_modconv_wgrad + _finish; `wscale` = 1/sqrt(Cin*k^2)).  Without it
    the weight is frozen, as on the mapper path (coach.py:174-180 optimises net.mapper only), and no weight-gradient kernel runs."""

    @staticmethod
    def forward(ctx, x, s, wsq, noise, noise_w, bias, packs, blur_kernel, upsample, fuse_act, link=None, d_pre=None, weight=None,
                wscale=1.0, fold=None):
        """`d_pre`: the layer's demodulation vector when the caller already has it (demod_coefficients_all).  `weight`: the
        trained raw conv weight (packs and wsq are then derived from it by the caller in this very forward).  `fold`: the RgbFoldLink
        of the pass-through ToRGB node that x came through (up-sampling layers of the synthesis loop)."""
        x, s = _c(x), _c(s)
        b, cin, h, w = x.shape
        wp_f, wp_b = packs
        d = None
        if wsq is not None:
            d = d_pre if d_pre is not None else demod_coefficients(s, wsq)
        act = (noise, noise_w, bias) if fuse_act else None
        if upsample and fuse_act and tuple(blur_kernel.shape) == (4, 4) and _upblur_planned(b, cin, wp_f.shape[3], h, w):
            out = _modconv_upblur_raw(x, wp_f, s, d, blur_kernel, h, w, act)
        elif upsample:
            t, _ = _modconv_raw(MODE_UP, x, wp_f, s, d, h, w)
            if fir_planar_ok(blur_kernel.shape, 2 * w):  # the tile kernel reads the phase-planar layout directly
                out = _upfirdn2d_raw(t, blur_kernel, 2 * h, 2 * w, 1, 1, 1, 1, True,
                                     act=((None,) + act) if fuse_act else None, planar_hw=(2 * h + 1, 2 * w + 1))
            else:         # tiny images: re-interleave (a [B,C,<=17,<=17] copy) and use the generic kernel
                out = _upfirdn2d_raw(unplanar(t, w), blur_kernel, 2 * h, 2 * w, 1, 1, 1, 1, True,
                                     act=((None,) + act) if fuse_act else None)
        else:
            out, _ = _modconv_raw(MODE_SAME, x, wp_f, s, d, h, w, act=act)
        ctx.save_for_backward(x, s, d, wsq, noise, noise_w, bias, out, wp_b, blur_kernel, weight)
        ctx.cfg = (upsample, fuse_act)
        ctx.wscale = float(wscale)
        ctx.link = link  # (an ActLink shared with the consuming ToRGB node, or None)
        ctx.fold = fold if (upsample and weight is None and d is not None) else None
        ctx.n_skip = _NOGRAD_PREFIX if _NOGRAD_PREFIX < b else 0
        ctx.pool = _GRAD_POOL
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, s, d, wsq, noise, noise_w, bias, out, wp_b, blur_kernel, weight = ctx.saved_tensors
        upsample, fuse_act = ctx.cfg
        n_skip, full = ctx.n_skip, x.shape[0]
        gout_full = gout
        gout = _c(gout)
        if n_skip:  # rows [:n_skip] carry no gradient: batch-major tensors, so the tails are contiguous views
            x, s, out, gout = x[n_skip:], s[n_skip:], out[n_skip:], gout[n_skip:]
            d = d[n_skip:] if d is not None else None
        b, cin, h, w = x.shape
        cout, oh, ow = out.shape[1], out.shape[2], out.shape[3]
        # inside `nograd_prefix`: full-batch gradient buffers whose tails the kernels write in place; the prefix rows of the
        # image-sized one stay unwritten (the producer node slices them off the same way), the [B,C]-sized one is zeroed
        gx_full = _grad_rows((full, cin, h, w), n_skip, x.device) if n_skip else None
        gx_out = gx_full[n_skip:] if n_skip else None
        gs_full, gs_out = _zeros_with_tail(full, n_skip, (cin,), x.device, ctx.pool)
        g_bias = g_nw = g_noise = sums = dz = None
        blurred = False
        # the shared [1,1,oh,ow] noise map is being optimised (the projector): its gradient is one more read of the pre-activation gradient
        want_noise = fuse_act and noise is not None and ctx.needs_input_grad[3]
        pre_sums = ctx.link.take(gout_full) if (fuse_act and ctx.link is not None) else None
        if pre_sums is not None:  # gout already IS the pre-activation gradient (the ToRGB backward applied the activation backward)
            gpre, sums = gout, pre_sums
        elif fuse_act:
            sums = torch.empty((b, cout, 3), device=x.device, dtype=torch.float32)
            if upsample and not want_noise and _blur_actbwd_planned(b * cout, oh, ow, blur_kernel.shape):
                # wide up-sampling layers: activation backward, its three reductions and the adjoint blur in ONE pass over
                # (gout, out) -- the pre-activation gradient is never written (3 tensor passes instead of 5); a noise map that needs a
                # gradient needs that tensor, and takes the branch below with the separate adjoint blur
                gpre = torch.empty((b, cout, oh + 1, ow + 1), device=x.device, dtype=torch.float32)
                sp = profiling.span("upfirdn2d", 4.0 * b * cout * (2 * oh * ow + (oh + 1) * (ow + 1)))  # algorithmic bytes: gout + out + gT
                call("w2e_blur_adjoint_actbwd", ptr(gout), ptr(out), ptr(noise), ptr(blur_kernel), ptr(gpre), ptr(sums), b * cout, oh, ow,
                     0.2, SQRT2, stream_ptr())
                if sp is not None:
                    sp.end()
                blurred = True
            else:
                gpre = torch.empty_like(out)
                call("w2e_bias_act_bwd_reduce", ptr(gout), ptr(out), ptr(noise), ptr(gpre), ptr(sums), b, cout, oh * ow,
                     0.2, SQRT2, stream_ptr())
        else:
            gpre = gout
            if d is not None:
                dz = (gout * out).sum((2, 3))
        if fuse_act:
            if bias is not None and ctx.needs_input_grad[5]:
                g_bias = sums[..., 2].sum(0)
            if noise is not None and ctx.needs_input_grad[4]:
                g_nw = sums[..., 1].sum().reshape(1)
        if want_noise:  # before the adjoint blur: gpre is still [b, cout, oh, ow], the rows that carry a gradient
            g_noise = torch.empty_like(noise)
            call("w2e_noise_grad", ptr(gpre), ptr(noise_w), ptr(g_noise), b * cout, oh * ow, 0, stream_ptr())
        if upsample and not blurred:
            # adjoint of Blur(pad=(1,1)) back onto the (2h+1)x(2w+1) transposed-conv grid, then the
            # stride-2 conv that is the adjoint of conv_transpose2d
            gpre = _upfirdn2d_raw(gpre, blur_kernel, 2 * h + 1, 2 * w + 1, 1, 1, 2, 2, False)
        g_w = None
        if weight is not None and ctx.needs_input_grad[12]:
            # the conv-weight gradient from the same gpre (UP: on the transposed-conv grid), x, s, d and demodulation coefficient
            wmode = WGRAD_UP if upsample else (WGRAD_CENTRE if weight.shape[-1] == 1 else WGRAD_SAME)
            g_w = modconv_wgrad(wmode, gpre, x, d, s, weight, ctx.wscale, sums=sums if d is not None and fuse_act else None,
                                dz=dz, noise_w=noise_w if (fuse_act and noise is not None) else None, bias=bias if fuse_act else None)
        mode = MODE_DOWN if upsample else MODE_SAME
        if _lib.get_option("deterministic") and not (mode == MODE_SAME and _wino_form(gpre, gpre.shape[1], cin, h, w, x)):
            # (both Winograd forms sum the partials of their fused dot in a fixed order: they stay)
            # the direct kernel's fused dot epilogue joins the workgroups of a (b, channel) with fp32 atomics; here instead: the unscaled
            # input gradient, its per-channel dot with x by a fixed-order wave reduction, then the out_scale
            raw, _ = _modconv_raw(mode, gpre, wp_b, d, None, h, w)
            gs = _channel_dot(raw, x, out=gs_out)
            gx = _scale_planes(raw, s)
            if n_skip:
                gx_out.copy_(gx)
        elif ctx.fold is not None and ctx.fold.usable(x, n_skip) and _rgbfold_planned(b, gpre.shape[1], cin, h, w):
            # x came through a ToRGB node whose backward would read x and this launch's output again: the launch does that node's work
            # in its epilogue (RgbFoldLink) and what it writes is the pre-activation gradient of the StyledConv below that node
            fold = ctx.fold
            xr, wrgb, st, nz, _ = fold.saved
            rgb_full = fold.gy.shape[0]
            gw_full, gw = _zeros_with_tail(rgb_full, n_skip, (cin,) if st is not None else (3, cin), x.device, ctx.pool)
            sums3 = ctx.pool.zeros((b, cin, 3), x.device) if ctx.pool is not None else None
            gx, gs, sums3, _ = _modconv_down_rgbfold_raw(
                gpre, wp_b, d, s, h, w, x, fold.gy[n_skip:] if n_skip else fold.gy, wrgb if (st is not None or not n_skip) else wrgb[n_skip:],
                None if st is None else (st[n_skip:] if n_skip else st), nz, out=gx_out, dot_out=gs_out, sums3=sums3, gw=gw)
            fold.gpre, fold.sums, fold.gw = (gx_full if n_skip else gx), sums3, gw_full
        else:
            gx, gs = _modconv_raw(mode, gpre, wp_b, d, s, h, w, dot_with=x, out=gx_out, dot_out=gs_out)
        if d is not None:  # + the demodulation path: gs -= s * (dz*d^2) @ wsq, with dz = sum_p gpre*(pre - nw*noise - bias)
            call("w2e_demod_bwd", ptr(sums), ptr(dz), ptr(noise_w) if (fuse_act and noise is not None) else None,
                 ptr(bias) if fuse_act else None, ptr(d), ptr(s), ptr(wsq), ptr(gs), None, b, cin, cout, stream_ptr())
        if n_skip:
            gx = gx_full
        return gx, gs_full, None, g_noise, g_nw, g_bias, None, None, None, None, None, None, g_w, None, None


def styled_conv(x, s, wsq, noise, noise_w, bias, packs, blur_kernel, upsample, link=None, demod=None, weight=None, wscale=1.0, fold=None):
    return _StyledConv.apply(x, s, wsq, noise, noise_w, bias, packs, blur_kernel, upsample, True, link, demod, weight, wscale, fold)


def modconv(x, s, wsq, packs, blur_kernel, upsample, weight=None, wscale=1.0):
    """Bare ModulatedConv2d (3x3): d * conv(Wp, s*x), with the FIR blur for the up-sampling variant."""
    return _StyledConv.apply(x, s, wsq, None, None, None, packs, blur_kernel, upsample, False, None, None, weight, wscale)


def modconv_down_plain(x, s, d, wp_f, h, w):
    """Forward-only stride-2 conv on a (2h+1)x(2w+1) input."""
    y, _ = _modconv_raw(MODE_DOWN, _c(x), wp_f, _c(s) if s is not None else None, _c(d) if d is not None else None, h, w)
    return y


# ------------------------------------------------------------------------------------------ style affines
class _StyleAffineAll(torch.autograd.Function):
    """Every `style = self.modulation(style)` of one generator pass (model.py:211, 26 EqualLinear calls) in one launch.
    pack = (w [R,D] = stacked weight*scale, bias [R] = stacked bias*lr_mul, meta int32 [R,4], widths): see w2e.h.
    Returns one [B, cin_l] tensor per layer; differentiable in the latent only (the decoder is frozen on this path)."""

    @staticmethod
    def forward(ctx, latent, pack):
        import ctypes
        latent = _c(latent)
        b, n_latent, dim = latent.shape
        w, bias, meta, widths = pack
        rows = w.shape[0]
        out = torch.empty(b * rows, device=latent.device, dtype=torch.float32)
        call("w2e_style_affine_fwd", ptr(latent), ptr(w), ptr(bias), ctypes.c_void_p(meta.data_ptr()), ptr(out), b, n_latent,
             dim, rows, stream_ptr())
        ctx.pack = pack
        ctx.geom = (b, n_latent, dim)
        ctx.n_skip = _NOGRAD_PREFIX if _NOGRAD_PREFIX < b else 0
        ctx.pool = _GRAD_POOL
        outs, off = [], 0
        for cw in widths:
            outs.append(out[off * b:(off + cw) * b].view(b, cw))
            off += cw
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        import ctypes
        b, n_latent, dim = ctx.geom
        n_skip = ctx.n_skip
        b -= n_skip
        w, bias, meta, widths = ctx.pack
        parts = [(g[n_skip:].reshape(-1) if g is not None else torch.zeros(b * cw, device=w.device, dtype=torch.float32))
                 for g, cw in zip(gs, widths)]
        flat = torch.cat(parts)
        glat_full, glat = _zeros_with_tail(b + n_skip, n_skip, (n_latent, dim), w.device, ctx.pool)
        call("w2e_style_affine_bwd", ptr(flat), ptr(w), ctypes.c_void_p(meta.data_ptr()), ptr(glat), b, n_latent, dim,
             w.shape[0], stream_ptr())
        return glat_full, None


def style_affine_all(latent, pack):
    return _StyleAffineAll.apply(latent, pack)


# ------------------------------------------------------------------------------------------ K1r
class _ToRGB(torch.autograd.Function):
    """`style` None: wmod is the per-sample [B,3,cin] weight; else wmod is the shared (frozen) [3,cin] scale*W and the kernels
    form wmod[c,i]*style[b,i] themselves, the backward returning the style gradient directly (w2e_torgb_styled_*).
    `passthrough`: also return x itself as a second output for the NEXT layer to consume.  x then has this node as its
    only consumer, and the gradient coming back through the next layer arrives here as `gx_next` and is folded into the
    ToRGB input gradient by the kernel (w2e_torgb_bwd_acc) -- instead of autograd adding two activation-sized tensors."""

    @staticmethod
    def forward(ctx, x, wmod, style, bias, skip, upk, passthrough=False, producer_act=None, fold_out=None, fold_skip=None):
        """`producer_act` = the ActLink of the fused StyledConv (slope 0.2, gain sqrt 2) whose output x is, when this node is its only
        consumer (the pass-through form, or the last layer): the backward then returns that layer's PRE-activation gradient.
        `fold_out` / `fold_skip`: the RgbFoldLink of this node (pass-through form with `producer_act`) / of the ToRGB node `skip` came
        from -- see there."""
        x_in = x
        x, wmod = _c(x), _c(wmod)
        b, cin, h, w = x.shape
        y = torch.empty((b, 3, h, w), device=x.device, dtype=torch.float32)
        skip_c = _c(skip) if skip is not None else None
        bias_c = _c(bias.reshape(-1)) if bias is not None else None
        if style is None:
            call("w2e_torgb_fwd", ptr(x), ptr(wmod), ptr(bias_c), ptr(skip_c), ptr(upk) if skip is not None else None,
                 ptr(y), b, cin, h, w, stream_ptr())
        else:
            style = _c(style.reshape(b, cin))
            if wmod.numel() != 3 * cin:
                raise RuntimeError(f"to_rgb: the shared weight must be [3,{cin}], got {tuple(wmod.shape)}")
            call("w2e_torgb_styled_fwd", ptr(x), ptr(wmod), ptr(style), ptr(bias_c), ptr(skip_c),
                 ptr(upk) if skip is not None else None, ptr(y), b, cin, h, w, stream_ptr())
        ctx.save_for_backward(x, wmod, style, upk if skip is not None else None, producer_act.noise if producer_act is not None else None)
        ctx.link = producer_act  # (the caller vouches that this node is x's only consumer)
        ctx.n_skip = _NOGRAD_PREFIX if _NOGRAD_PREFIX < b else 0
        ctx.fold_out = fold_out if (passthrough and producer_act is not None) else None
        ctx.fold_skip = fold_skip if skip is not None else None
        if ctx.fold_out is not None:  # what the backward kernel of this node would read, for the launch that does its work instead
            ctx.fold_out.saved = (x.detach(), wmod.detach(), style.detach() if style is not None else None, producer_act.noise, ctx.n_skip)
        ctx.has = (bias is not None, skip is not None, tuple(bias.shape) if bias is not None else None)
        ctx.pool = _GRAD_POOL
        if passthrough:
            return y, x_in.view_as(x_in)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gx_next=None):
        x, wmod, style, upk, act_noise = ctx.saved_tensors
        has_bias, has_skip, bias_shape = ctx.has
        n_skip = ctx.n_skip
        b, cin, h, w = x.shape
        if gy is None:  # only the pass-through output was used
            return gx_next, None, None, None, None, None, None, None, None, None
        folded = ctx.fold_out.take(gy, gx_next) if ctx.fold_out is not None else None
        gy = _c(gy)
        if folded is not None:
            # the stride-2 conv of the level above has done this node's kernel in its epilogue: gx_next IS the pre-activation gradient
            gx, sums3, gw_full = folded
            gys = gy[n_skip:] if n_skip else gy
            ctx.link.gpre, ctx.link.sums = gx, sums3
            return (gx,) + _rgb_small_grads(ctx, gys, gw_full, wmod, style, upk, n_skip, b, h, w, x.device)
        gx = _grad_rows(None, n_skip, x.device, like=x)
        acc = _c(gx_next) if gx_next is not None else None
        if n_skip:  # the tails of batch-major tensors: contiguous views, written / read in place
            xs, gys, gxs = x[n_skip:], gy[n_skip:], gx[n_skip:]
            accs = acc[n_skip:] if acc is not None else None
        else:
            xs, gys, gxs, accs = x, gy, gx, acc
        ws = wmod if style is not None else (wmod[n_skip:] if n_skip else wmod)
        sts = None if style is None else (style[n_skip:] if n_skip else style)
        gw_full, gw = _zeros_with_tail(b, n_skip, (cin,) if style is not None else (3, cin), x.device, ctx.pool)
        if ctx.link is not None:
            # x is the activated output of the StyledConv below: hand that layer its pre-activation gradient and sums directly
            sums3 = torch.empty((b - n_skip, cin, 3), device=x.device, dtype=torch.float32)
            call("w2e_torgb_bwd_actbwd", ptr(xs), ptr(ws), ptr(sts), ptr(gys), ptr(accs), ptr(act_noise), ptr(gxs), ptr(gw), ptr(sums3),
                 b - n_skip, cin, h, w, 0.2, SQRT2, stream_ptr())
            ctx.link.gpre, ctx.link.sums = gx, sums3
        elif style is None:
            call("w2e_torgb_bwd_acc", ptr(xs), ptr(ws), ptr(gys), ptr(accs), ptr(gxs), ptr(gw), b - n_skip, cin, h, w, stream_ptr())
        else:
            call("w2e_torgb_styled_bwd", ptr(xs), ptr(ws), ptr(sts), ptr(gys), ptr(accs), ptr(gxs), ptr(gw), b - n_skip, cin, h, w,
                 stream_ptr())
        return (gx,) + _rgb_small_grads(ctx, gys, gw_full, wmod, style, upk, n_skip, b, h, w, x.device)


def _rgb_small_grads(ctx, gys, gw_full, wmod, style, upk, n_skip, b, h, w, device):
    """The tail of _ToRGB.backward's return tuple: weight or style gradient, the 3-channel bias gradient, and the gradient of the skip
    image (recorded on the RgbFoldLink of the ToRGB node below, whose incoming gradient it is)."""
    has_bias, has_skip, bias_shape = ctx.has
    g_wmod, g_style = (gw_full.view_as(wmod), None) if style is None else (None, gw_full)
    gb = gys.sum((0, 2, 3)).reshape(bias_shape) if (has_bias and ctx.needs_input_grad[3]) else None
    gskip = None
    if has_skip:  # adjoint of Upsample(up=2, pad=(2,1)): down=2, un-flipped taps, leading pad 4-1-2
        gskip = _grad_rows((b, 3, h // 2, w // 2), n_skip, device)  # rows [:n_skip]: see _StyledConv
        _upfirdn2d_raw(gys, upk, h // 2, w // 2, 1, 2, 1, 1, False, out=gskip[n_skip:] if n_skip else gskip)
        if ctx.fold_skip is not None:
            ctx.fold_skip.gy = gskip
    return g_wmod, g_style, gb, gskip, None, None, None, None, None


def to_rgb(x, wmod, bias, skip, upk, passthrough=False, style=None, producer_act=None, fold_out=None, fold_skip=None):
    """y = sum_i wmod[b,c,i] x[b,i] + bias + Upsample(skip)   (model.py:353-362); with `passthrough` -> (y, x).
    With `style` [B,cin]: wmod is the shared [3,cin] scale*W (treated as frozen) and the weight of sample b is
    wmod[c,i]*style[b,i]."""
    return _ToRGB.apply(x, wmod, style, bias, skip, upk, passthrough, producer_act, fold_out, fold_skip)


# ------------------------------------------------------------------------------------------ K5
class _ClipPreproc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img):
        img = _c(img)
        n, c, h, w = img.shape
        if h != w:
            raise RuntimeError("clip_preprocess expects square images")
        out = torch.empty((n, c, 224, 224), device=img.device, dtype=torch.float32)
        call("w2e_clip_preproc_fwd", ptr(img), ptr(out), n * c, h, stream_ptr())
        ctx.shape = img.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        n, c, h, w = ctx.shape
        gimg = torch.empty(ctx.shape, device=gout.device, dtype=torch.float32)
        call("w2e_clip_preproc_bwd", ptr(_c(gout)), ptr(gimg), n * c, h, stream_ptr())
        return gimg


def clip_preprocess(img):
    """AvgPool2d(size//32)(Upsample(scale_factor=7)(img)) in one closed-form pass (clip_loss.py:11-12,15)."""
    return _ClipPreproc.apply(img)


class _IdPreproc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img):
        img = _c(img)
        n, c, h, w = img.shape
        out = torch.empty((n, c, 112, 112), device=img.device, dtype=torch.float32)
        call("w2e_id_preproc_fwd", ptr(img), ptr(out), n * c, h, stream_ptr())
        ctx.shape = img.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        n, c, h, w = ctx.shape
        gimg = torch.empty(ctx.shape, device=gout.device, dtype=torch.float32)
        call("w2e_id_preproc_bwd", ptr(_c(gout)), ptr(gimg), n * c, h, stream_ptr())
        return gimg


def id_preprocess(img):
    """face_pool(pool(img)[:, :, 35:223, 32:220]) of criteria/id_loss.py:19-23 in one pass (square, size % 256 == 0)."""
    return _IdPreproc.apply(img)


# ------------------------------------------------------------------------------------------ K6
class _MaskBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, mask):
        a, b, mask = _c(a), _c(b), _c(mask)
        n, c, h, w = a.shape
        if b.shape != a.shape or mask.shape[0] != n or mask.shape[1] != 1 or mask.shape[2] != mask.shape[3]:
            raise RuntimeError(f"mask_blend: shapes {tuple(a.shape)} {tuple(b.shape)} {tuple(mask.shape)}")
        out = torch.empty_like(a)
        call("w2e_mask_blend_fwd", ptr(a), ptr(b), ptr(mask), ptr(out), n, c, h, w, mask.shape[2], stream_ptr())
        ctx.save_for_backward(a, b, mask)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        a, b, mask = ctx.saved_tensors
        n, c, h, w = a.shape
        gout = _c(gout)
        ga = torch.empty_like(a)
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        gm = torch.empty_like(mask) if ctx.needs_input_grad[2] else None
        call("w2e_mask_blend_bwd", ptr(gout), ptr(a), ptr(b), ptr(mask), ptr(ga), ptr(gb), ptr(gm), n, c, h, w,
             mask.shape[2], stream_ptr())
        return ga, gb, gm


def mask_blend(new, old, mask):
    """m*new + (1-m)*old with m = nearest-resized mask (attention_model.py:548-549)."""
    return _MaskBlend.apply(new, old, mask)
