"""Every FIR (upfirdn2d) kernel the dispatcher of where2edit_amd/csrc/upfirdn2d.hip can pick, run one by one and compared with float64.

w2e_upfirdn2d picks between six kernels and thirteen instantiations per launch (generic, down4, tile, tile4<ACT>,
blur4<ACT, PLANAR>, stream4<ACT, PLANAR>: 1 + 1 + 1 + 2 + 4 + 4); w2e_blur_adjoint_actbwd is the fourteenth (stream4<ACTBWD>).  FIR_MATRIX and
ACTBWD_MATRIX below are the launches these tests run.  Every entry names the kernel and the template flags it was written for, and
the library's `tune_print` "upfirdn variant" line of the launch has to name the same: a case that silently runs another kernel
fails.  The census in tests/test_gpu_conv_variants.py collects the FIR variants real eager steps launch and fails when one of
them has no entry here.

The reference (ref_upfirdn / ref_term_scale) is a plain float64 restatement of the ABI -- zero-stuffing, padding or cropping,
torch.nn.functional.conv2d on CPU doubles, the optional epilogue -- that shares no code with oracle/ops.py or the library;
test_reference_reproduces_the_golden_outputs pins it to the reference project's own outputs (tests/golden/ops.npz) without a GPU.

Inputs are heavy-tailed (per-plane log-normal scales, sigma 1.5, with x30 outlier planes; out_scale 10x apart between samples;
noise and biases on the scale of the smallest plane they are added to, so that both LeakyReLU branches are taken in every
plane).  x and y live inside larger buffers: the floats around x are NaN (never read into a result), the floats around y a
sentinel (never written), y itself starts as NaN (every output written), and the phase-planar layout's padding is NaN.

Tolerances.  A 4x4 output is a 16-term fp32 sum; with the separable factor kv[i] = k[i][0] / k[0][0] and the epilogue the
worst-case bound is about 20 * 2^-24 = 1.2e-6 of the term scale, so FWD_TOL = 1e-5 (the figure tests/test_gpu_parity.py uses for
this operation) leaves about 8x and needs no measurement; 9- to 16-tap kernels: the larger of 1e-5 and 8 * (taps + 4) * 2^-24
(tap_tol).  Every forward result is held to it twice: globally (assert_close) and per plane against the plane's own term scale
(assert_close_planes).  The three sums of the ACTBWD form are fp32 partial sums joined by atomics over up to 10^6 terms; they
are held, relative to each plane's sum of |terms|, to SUMS_TOL = min(2e-5, 4 x the worst error of the unfused pair
(w2e_bias_act_bwd_reduce, the baseline, not the code under test) measured on the same inputs).

Measured on an MI355X over this file's cases (worst plane, relative to the plane's own term scale):
    generic 2.1e-7, down4 2.0e-7, tile 1.9e-7, tile4<act 0> 2.0e-7, tile4<act 1> 1.7e-7,
    blur4<act 0, dense> 1.2e-7, blur4<act 1, dense> 1.7e-7, blur4<act 0, planar> 1.3e-7, blur4<act 1, planar> 1.5e-7,
    stream4<act 0, dense> 1.3e-7, stream4<act 1, dense> 1.6e-7, stream4<act 0, planar> 1.2e-7, stream4<act 1, planar> 1.6e-7,
    stream4<ACTBWD> gt 1.4e-7; its three sums, worst plane against the plane's sum of |terms|: fused 1.8e-8, the unfused pair
    2.0e-8 (UNFUSED_SUMS_WORST), so SUMS_TOL = 8e-8.
What the matrix found: stream4<ACT, dense> wrote the single last column (out_w = in_w + 1) without the epilogue, and gave that
column three taps for any odd out_w, also one narrower than the source where it has four; both are fixed in the library.
"""
import math
import re

import pytest
import torch
import torch.nn.functional as F

import seeded
from helpers import assert_close, assert_close_planes, golden, plane_errors
from make_golden import UPFIRDN_CASES, _kernel

DEV = "cuda"
SLOPE, GAIN = 0.2, 2 ** 0.5
FWD_TOL = 1e-5
UNFUSED_SUMS_WORST = 2.0e-8  # w2e_bias_act_bwd_reduce on ACTBWD_MATRIX's inputs, measured (test_actbwd_stream_against_float64 prints it)
SUMS_TOL = min(2e-5, 4.0 * UNFUSED_SUMS_WORST)


def tap_tol(kh, kw):
    """FWD_TOL up to 16 taps; beyond, 8 x the worst-case fp32 bound of a (kh * kw + 4)-operation sum."""
    return max(FWD_TOL, 8.0 * (kh * kw + 4) * 2.0 ** -24) if kh * kw > 16 else FWD_TOL


# ---- the float64 reference --------------------------------------------------------------------------------------------------------
def _fir64(x, k, up, down, pad_x0, pad_y0, flip, out_h, out_w):
    """out[oy, ox] = sum_ky,kx kk[ky, kx] * z[oy * down + ky - pad_y0, ox * down + kx - pad_x0]: z = x zero-stuffed by `up` (zero
    outside), kk = k rotated by 180 degrees when flip else k.  x [N,C,H,W], k [kh,kw] -> float64 [N,C,out_h,out_w]."""
    x, k = x.detach().double().cpu(), k.detach().double().cpu()
    n, c, h, w = x.shape
    kh, kw = k.shape
    z = x
    if up > 1:
        z = x.new_zeros(n, c, h * up, w * up)
        z[:, :, ::up, ::up] = x
    # the rows the outputs read are -pad_y0 ... (out_h - 1) * down + kh - 1 - pad_y0 of z: pad (or crop, when negative) to exactly those
    bottom = (out_h - 1) * down + kh - pad_y0 - z.shape[2]
    right = (out_w - 1) * down + kw - pad_x0 - z.shape[3]
    z = F.pad(z, (pad_x0, right, pad_y0, bottom))
    kk = torch.flip(k, (0, 1)) if flip else k
    y = F.conv2d(z.reshape(1, n * c, z.shape[2], z.shape[3]), kk.reshape(1, 1, kh, kw).repeat(n * c, 1, 1, 1), stride=down, groups=n * c)
    assert tuple(y.shape[2:]) == (out_h, out_w), (y.shape, out_h, out_w)
    return y.reshape(n, c, out_h, out_w)


def _epilogue64(v, out_scale, noise, noise_w, bias, slope, gain, absolute):
    """lrelu(out_scale[plane] * v + noise_w * noise[HW] + bias[plane % C], slope) * gain on [N,C,H,W] (plane = sample * C + channel);
    absolute: the same on the magnitudes and without the LeakyReLU -- the scale of the terms each output sums."""
    n, c, h, w = v.shape
    mag = (lambda t: t.abs()) if absolute else (lambda t: t)
    if out_scale is not None:
        v = v * mag(out_scale.detach().double().cpu().reshape(n * c)).reshape(n, c, 1, 1)
    if noise is not None:
        v = v + mag(noise_w.detach().double().cpu().reshape(()) * noise.detach().double().cpu().reshape(h, w))
    if bias is not None:
        channel = torch.arange(n * c) % c
        v = v + mag(bias.detach().double().cpu().reshape(c))[channel].reshape(n, c, 1, 1)
    return v * gain if absolute else torch.where(v > 0, v, v * slope) * gain


def ref_upfirdn(x, k, up, down, pad_x0, pad_y0, flip, out_h, out_w, act=None, slope=SLOPE, gain=GAIN):
    """w2e_upfirdn2d in float64.  act = (out_scale[planes]|None, noise[HW]|None, noise_w|None, bias[C]|None) or None."""
    y = _fir64(x, k, up, down, pad_x0, pad_y0, flip, out_h, out_w)
    return y if act is None else _epilogue64(y, *act, slope, gain, False)


def ref_term_scale(x, k, up, down, pad_x0, pad_y0, flip, out_h, out_w, act=None, slope=SLOPE, gain=GAIN):
    """The same operation on |x|, |k|, |out_scale|, |noise_w * noise| and |bias|, without the LeakyReLU (assert_close_planes' scale)."""
    y = _fir64(x.abs(), k.abs(), up, down, pad_x0, pad_y0, flip, out_h, out_w)
    return y if act is None else _epilogue64(y, *act, slope, gain, True)


def test_reference_reproduces_the_golden_outputs():
    """ref_upfirdn against the reference project's own outputs (tests/golden/ops.npz): every upfirdn.*.y, every .gx through the
    adjoint call functional._UpFirDn2d.backward makes (swapped up / down, k - 1 - pad, un-flipped taps, the input's size), and
    oracle.ops.upfirdn2d on the asymmetric 5x3 case.  Runs without a GPU."""
    from oracle import ops as O
    g = golden("ops")
    for name, shape, kspec, gain, up, down, pad in UPFIRDN_CASES:
        x, k = seeded.tensor("upfirdn." + name, shape), _kernel(kspec, gain)
        kh, kw = k.shape
        h, w = shape[2:]
        out_h, out_w = (h * up + pad[0] + pad[1] - kh) // down + 1, (w * up + pad[0] + pad[1] - kw) // down + 1
        y = ref_upfirdn(x, k, up, down, pad[0], pad[0], True, out_h, out_w)
        assert_close(y, g[f"upfirdn.{name}.y"], 1e-6, f"{name} y")
        gy = seeded.tensor("upfirdn.gy." + name, y.shape)
        gx = ref_upfirdn(gy, k, down, up, kw - 1 - pad[0], kh - 1 - pad[0], False, h, w)
        assert_close(gx, g[f"upfirdn.{name}.gx"], 1e-6, f"{name} gx")
        if kspec == "asym5x3":
            assert_close(y, O.upfirdn2d(x.double(), k.double(), up, down, pad), 1e-12, f"{name} against oracle.ops")
    # the epilogue and the term scale on a hand-checked value: 2 planes of 1 channel... (sample 1 uses bias[1 % 1] = bias[0])
    x1 = torch.tensor([[[[2.0]]], [[[-3.0]]]])
    one = torch.ones(1, 1)
    act = (torch.tensor([0.5, 2.0]), torch.tensor([4.0]), torch.tensor([0.25]), torch.tensor([-1.5]))
    y1 = ref_upfirdn(x1, one, 1, 1, 0, 0, True, 1, 1, act=act, slope=0.1, gain=3.0)
    assert torch.allclose(y1.reshape(2), torch.tensor([(1.0 + 1.0 - 1.5) * 3.0, (-6.0 + 1.0 - 1.5) * 0.1 * 3.0], dtype=torch.float64))
    s1 = ref_term_scale(x1, one, 1, 1, 0, 0, True, 1, 1, act=act, slope=0.1, gain=3.0)
    assert torch.allclose(s1.reshape(2), torch.tensor([(1.0 + 1.0 + 1.5) * 3.0, (6.0 + 1.0 + 1.5) * 3.0], dtype=torch.float64))


# ---- the variant matrix -----------------------------------------------------------------------------------------------------------
def E(kernel, act, planar, planes, src, out, pad, taps=(4, 4), up=1, down=1, xoff=0, yoff=0, tune_blur=0):
    """One matrix entry: the kernel / ACT / PLANAR it was written for; planes = (samples, channels), src = (in_h, in_w), out =
    (out_h, out_w), pad = (pad_x0, pad_y0); taps = (kh, kw) or "asym5x3"; xoff / yoff: floats by which x / y miss 16-byte alignment."""
    return dict(kernel=kernel, act=act, planar=planar, planes=planes, src=src, out=out, pad=pad, taps=taps, up=up, down=down,
                xoff=xoff, yoff=yoff, tune_blur=tune_blur)


FIR_MATRIX = [
    # generic: up-sampling, > 8 taps, out_w < 32 with an epilogue
    E("generic", 0, 0, (1, 3), (32, 32), (64, 64), (2, 2), up=2),              # the RGB-skip Upsample: up 2, pad (2, 1)
    E("generic", 0, 0, (1, 3), (256, 256), (512, 512), (2, 2), up=2),
    E("generic", 0, 0, (2, 2), (20, 40), (31, 62), (2, 2), taps="asym5x3", up=3, down=2),
    E("generic", 0, 0, (2, 3), (40, 48), (40, 48), (4, 4), taps=(9, 9)),
    E("generic", 1, 0, (2, 3), (40, 48), (40, 48), (4, 4), taps=(9, 9)),
    E("generic", 0, 0, (2, 2), (40, 50), (40, 50), (8, 7), taps=(16, 16)),
    E("generic", 1, 0, (2, 2), (33, 37), (30, 36), (5, 8), taps=(12, 16)),
    E("generic", 1, 0, (2, 3), (17, 17), (16, 16), (1, 1)),                    # the tiny blurs of a forward (8^2, 16^2)
    E("generic", 1, 0, (2, 3), (10, 20), (10, 20), (1, 1), taps=(3, 3)),
    E("generic", 1, 0, (2, 3), (9, 9), (8, 8), (1, 1)),
    # down4: 4x4, up 1, no epilogue, not tile-eligible
    E("down4", 0, 0, (1, 3), (64, 64), (32, 32), (1, 1), down=2),             # the adjoint of the RGB-skip Upsample
    E("down4", 0, 0, (2, 3), (33, 47), (16, 23), (1, 1), down=2),
    E("down4", 0, 0, (1, 3), (130, 1024), (65, 512), (1, 1), down=2),
    E("down4", 0, 0, (2, 2), (50, 70), (17, 24), (2, 2), down=3),
    E("down4", 0, 0, (2, 3), (8, 8), (9, 9), (2, 2)),                          # down 1, out_w < 32
    E("down4", 0, 0, (2, 3), (16, 16), (15, 15), (1, 1)),
    E("down4", 0, 0, (1, 2), (20, 31), (18, 31), (2, 0)),
]
# tile: up = down = 1, out_w >= 32, <= 8 taps per axis but not 4x4 -- each tap shape with and without the epilogue
for _taps, _src, _out, _pad in (((1, 1), (40, 32), (40, 32), (0, 0)), ((3, 3), (35, 63), (35, 63), (1, 1)), ((5, 5), (50, 65), (50, 65), (2, 2)),
                                ((8, 8), (45, 130), (45, 130), (3, 4)), ((5, 3), (33, 70), (33, 70), (1, 2)), ((3, 5), (64, 40), (64, 40), (2, 1)),
                                ((3, 3), (60, 100), (50, 90), (-2, -3)), ((8, 8), (70, 140), (40, 130), (-3, 2)), ((2, 7), (31, 260), (33, 257), (3, 1))):
    FIR_MATRIX += [E("tile", _a, 0, (2, 3), _src, _out, _pad, taps=_taps) for _a in (0, 1)]
FIR_MATRIX += [
    # tile4<ACT>: 4x4, source rows not 16-byte aligned (odd in_w, or x one float into its buffer)
    E("tile4", 0, 0, (2, 3), (33, 35), (30, 32), (0, 0)),
    E("tile4", 1, 0, (2, 3), (40, 33), (40, 33), (1, 2)),
    E("tile4", 0, 0, (2, 3), (65, 65), (64, 64), (1, 1)),
    E("tile4", 1, 0, (2, 3), (65, 65), (64, 64), (1, 1)),
    E("tile4", 1, 0, (2, 3), (50, 63), (47, 65), (3, 0)),
    E("tile4", 0, 0, (2, 3), (50, 63), (51, 64), (2, 2)),
    E("tile4", 0, 0, (2, 2), (20, 257), (20, 255), (2, 1)),
    E("tile4", 1, 0, (2, 2), (70, 71), (60, 64), (-1, -2)),
    E("tile4", 0, 0, (2, 3), (40, 64), (41, 65), (2, 2), xoff=1),
    E("tile4", 1, 0, (2, 3), (36, 128), (35, 127), (1, 1), xoff=1),
    E("tile4", 1, 0, (1, 3), (35, 64), (33, 64), (0, 3), xoff=1, yoff=1),
    E("tile4", 0, 0, (1, 3), (30, 259), (29, 258), (1, 1)),                    # (the adjoint of a wide pad-2 blur)
    E("tile4", 1, 0, (1, 3), (30, 261), (31, 260), (2, 1)),
    # blur4<ACT, dense>: 4x4, in_w % 4 == 0 and x aligned, the stream form not eligible
    E("blur4", 0, 0, (2, 3), (64, 64), (65, 65), (2, 2)),
    E("blur4", 1, 0, (2, 3), (40, 128), (39, 127), (1, 1)),
    E("blur4", 0, 0, (2, 3), (32, 32), (31, 33), (2, 1)),
    E("blur4", 1, 0, (2, 3), (36, 64), (30, 50), (-3, -2)),
    E("blur4", 0, 0, (2, 2), (50, 260), (49, 259), (1, 1)),                    # out_w >= 256, pad_x0 != 2
    E("blur4", 1, 0, (2, 2), (40, 256), (40, 258), (3, 2)),
    E("blur4", 0, 0, (2, 2), (70, 256), (71, 257), (2, 2), yoff=1),            # y one float off alignment: no stream form
    E("blur4", 1, 0, (2, 2), (70, 256), (69, 256), (2, 1), yoff=1),
    E("blur4", 0, 0, (4, 8), (545, 252), (544, 250), (1, 1)),                  # 32 planes x 17 tile rows > 512 workgroup rows: several items each
    E("blur4", 1, 0, (4, 8), (545, 252), (544, 250), (1, 1)),
    E("blur4", 0, 0, (1, 3), (66, 512), (65, 513), (2, 2), tune_blur=8),
    # blur4<ACT, planar>: the UP conv's phase-planar source
    E("blur4", 1, 1, (2, 3), (33, 33), (32, 32), (1, 1)),
    E("blur4", 0, 1, (2, 3), (65, 65), (64, 64), (1, 1)),
    E("blur4", 1, 1, (2, 3), (65, 65), (64, 64), (1, 1)),
    E("blur4", 1, 1, (2, 2), (41, 253), (40, 252), (1, 1)),
    E("blur4", 0, 1, (2, 2), (35, 259), (34, 258), (1, 1)),                    # W odd: out_w % 4 != 0 keeps it off the stream kernel
    E("blur4", 1, 1, (2, 2), (35, 259), (34, 258), (1, 1)),
    E("blur4", 0, 1, (2, 3), (33, 65), (34, 62), (0, 2)),
    E("blur4", 1, 1, (2, 2), (30, 257), (31, 256), (2, 3)),                    # out_w >= 256 with pad_x0 != 1
    E("blur4", 1, 1, (1, 3), (67, 513), (66, 512), (1, 1), tune_blur=8),
    E("blur4", 0, 1, (1, 3), (67, 513), (66, 512), (1, 1), tune_blur=8),
]
# stream4<ACT, planar>: out_w >= 256, pad_x0 = 1, in_w = out_w + 1, out_w % 4 == 0; strips of 64 rows
for _a in (0, 1):
    FIR_MATRIX += [
        E("stream4", _a, 1, (2, 2), (5, 257), (1, 256), (1, 0)),
        E("stream4", _a, 1, (2, 2), (63, 261), (63, 260), (1, 1)),
        E("stream4", _a, 1, (2, 2), (64, 513), (64, 512), (1, 2)),
        E("stream4", _a, 1, (2, 2), (63, 517), (65, 516), (1, 3)),
        E("stream4", _a, 1, (1, 2), (130, 1025), (129, 1024), (1, 1)),
        # stream4<ACT, dense>: pad_x0 = 2, in_w % 4 == 0, out_w <= in_w + 1
        E("stream4", _a, 0, (2, 2), (4, 256), (1, 256), (2, 0)),
        E("stream4", _a, 0, (2, 2), (62, 260), (63, 260), (2, 1)),
        E("stream4", _a, 0, (2, 2), (63, 512), (64, 512), (2, 2)),
        E("stream4", _a, 0, (2, 2), (64, 516), (65, 516), (2, 3)),
        E("stream4", _a, 0, (1, 2), (128, 1024), (129, 1024), (2, 2)),
        E("stream4", _a, 0, (2, 2), (64, 256), (65, 257), (2, 2)),             # out_w = in_w + 1: the single last column
        E("stream4", _a, 0, (2, 2), (40, 264), (40, 256), (2, 2)),             # out_w < in_w
        E("stream4", _a, 0, (2, 2), (33, 260), (33, 257), (2, 2)),             # ... and odd: the last column has all four taps
        E("stream4", _a, 0, (2, 2), (22, 260), (20, 258), (2, 1)),
        E("stream4", _a, 0, (2, 2), (20, 260), (21, 259), (2, -1)),
    ]
FIR_MATRIX += [
    E("stream4", 1, 1, (1, 2), (1025, 1025), (1024, 1024), (1, 1)),            # a real layer, once
    E("stream4", 0, 0, (1, 2), (130, 1024), (131, 1025), (2, 2)),
    E("generic", 0, 0, (2, 3), (8, 8), (16, 16), (2, 2), up=2),                # the RGB-skip Upsample below 32 columns (8^2 -> 16^2)
]

# stream4<ACTBWD> through w2e_blur_adjoint_actbwd: (samples, channels), h, w, with noise
ACTBWD_MATRIX = [
    ((2, 2), 2, 256, True), ((2, 2), 64, 260, False), ((2, 3), 130, 256, True), ((1, 2), 64, 1024, True), ((1, 2), 130, 1024, False),
    ((2, 2), 2, 260, False), ((1, 3), 63, 512, True),
]

FIR_VARIANT = re.compile(r"upfirdn variant kernel (\w+) act (\d) planar (\d) actbwd (\d) up (\d+) down (\d+) taps (\d+)x(\d+) (\d+) (\d+)x(\d+) -> (\d+)x(\d+)$")
# the fourteen instantiations the library compiles: (kernel, ACT, PLANAR, ACTBWD); the generic, down4 and tile kernels are not templates
INSTANTIATIONS = ({("generic", None, None, 0), ("down4", None, None, 0), ("tile", None, None, 0), ("tile4", 0, None, 0), ("tile4", 1, None, 0),
                   ("stream4", 0, 0, 1)} | {(kn, a, pl, 0) for kn in ("blur4", "stream4") for a in (0, 1) for pl in (0, 1)})


def taps_of(e):
    if e["taps"] == "asym5x3":
        return 5, 3
    return e["taps"]


def instantiation(kernel, act, planar, actbwd):
    if kernel in ("generic", "down4", "tile"):
        return (kernel, None, None, 0)
    return (kernel, act, None, 0) if kernel == "tile4" else (kernel, act, planar, actbwd)


def width_class(out_w):
    return 0 if out_w < 32 else (1 if out_w < 256 else 2)


def fir_key(kernel, act, planar, actbwd, up, down, kh, kw, out_w):
    """The census key of a launch: kernel and flags, up / down, the tap shape and the class of out_w (< 32, 32-255, >= 256)."""
    return (kernel, act, planar, actbwd, up, down, f"{kh}x{kw}", width_class(out_w))


def covered_fir():
    keys = {fir_key(e["kernel"], e["act"], e["planar"], 0, e["up"], e["down"], *taps_of(e), e["out"][1]) for e in FIR_MATRIX}
    return keys | {fir_key("stream4", 0, 0, 1, 1, 1, 4, 4, w + 1) for _, _, w, _ in ACTBWD_MATRIX}


def parse_fir_variants(lines):
    """[(key, line)] of the "upfirdn variant" lines among the library's tune_print output."""
    out = []
    for ln in lines:
        m = FIR_VARIANT.match(ln)
        if m:
            v = [int(t) for t in m.groups()[1:]]
            out.append((fir_key(m[1], v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[11]), ln))
    return out


def test_matrix_names_every_instantiation():
    """Each of the fourteen instantiations has at least one entry (whose variant line the matrix tests assert): deleting the last
    entry of one fails here.  Runs without a GPU."""
    have = {instantiation(e["kernel"], e["act"], e["planar"], 0) for e in FIR_MATRIX}
    if ACTBWD_MATRIX:
        have.add(("stream4", 0, 0, 1))
    assert len(INSTANTIATIONS) == 14
    assert have == INSTANTIATIONS, f"missing {sorted(INSTANTIATIONS - have, key=str)}, unknown {sorted(have - INSTANTIATIONS, key=str)}"
    for e in FIR_MATRIX:  # the float64 references stay cheap: at most 6 planes at sizes >= 512^2
        if e["out"][0] * e["out"][1] >= 512 * 512 or e["src"][0] * e["src"][1] >= 512 * 512:
            assert e["planes"][0] * e["planes"][1] <= 6, e


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
SAMPLE_SCALE = (1.0, 12.0, 0.08)  # per-sample factor of out_scale (cycled): any two are >= 10x apart
GUARD = 64                        # floats before and after x / y inside their buffers (a multiple of 4: alignment is kept)
SENTINEL = 1234.5


def tap_matrices(e, g):
    """[(name, taps)]: 4x4 entries run the separable blur, a fully non-separable matrix, one with k[0][0] = 0 (and k[3][3] = 0:
    the first tap after the flip) and an exact rank-1 matrix of unequal row and column vectors; others one seeded matrix."""
    if e["taps"] == "asym5x3":
        return [("asym5x3", seeded.tensor("asym5x3", (5, 3)))]
    kh, kw = e["taps"]
    if (kh, kw) != (4, 4):
        return [(f"random {kh}x{kw}", torch.randn(kh, kw, generator=g) / math.sqrt(kh * kw))]
    full = torch.randn(4, 4, generator=g) / 4
    zero = torch.randn(4, 4, generator=g) / 4
    zero[0, 0] = zero[3, 3] = 0.0
    rank1 = torch.outer(torch.tensor([0.25, -0.75, 0.5, 1.25]), torch.tensor([0.25, 0.125, -0.5, 0.375]))  # (dyadic: exactly rank 1 in fp32)
    return [("separable", seeded.fir_kernel(gain=4.0)), ("non-separable", full), ("k00 = 0", zero), ("rank-1", rank1)]


def heavy_planes(g, n, c, h, w):
    """[n,c,h,w]: N(0,1) times per-plane log-normal scales (sigma 1.5), a quarter of the planes (at least one) x30."""
    ps = torch.exp(1.5 * torch.randn(n * c, generator=g))
    ps[torch.randperm(n * c, generator=g)[:max(1, (n * c) // 4)]] *= 30.0
    return torch.randn(n, c, h, w, generator=g) * ps.reshape(n, c, 1, 1)


def epilogue_inputs(g, raw, with_scale):
    """(out_scale|None, noise, noise_w, bias) for the float64 filtered planes `raw`: out_scale 10x apart between samples; the bias of a
    channel and the noise a fraction of the spread of the SMALLEST plane they are added to (both LeakyReLU branches in every plane)."""
    n, c, h, w = raw.shape
    out_scale = None
    sd = raw.reshape(n, c, -1).std(2, unbiased=False)
    if with_scale:
        out_scale = (torch.rand(n, c, generator=g) + 0.5) * torch.tensor([SAMPLE_SCALE[i % 3] for i in range(n)])[:, None]
        sd = sd * out_scale.double()
    bias = (0.4 * (torch.rand(c, generator=g) + 0.5) * torch.sign(torch.randn(c, generator=g)) * sd.amin(0)).float()
    noise = torch.randn(h * w, generator=g)
    noise_w = (0.4 * sd.min()).float().reshape(1)
    return out_scale, noise, noise_w, bias


def guarded(t, off, fill):
    """A copy of t on the GPU that starts GUARD + off floats into a buffer of `fill`: (buffer, view)."""
    buf = torch.full((GUARD + off + t.numel() + GUARD,), fill, device=DEV, dtype=torch.float32)
    v = buf[GUARD + off:GUARD + off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return buf, v


def guards_intact(buf, off, numel, fill):
    head, tail = buf[:GUARD + off], buf[GUARD + off + numel:]
    same = (lambda t: torch.isnan(t).all()) if fill != fill else (lambda t: (t == fill).all())
    return bool(same(head)) and bool(same(tail))


def to_planar(t, fill):
    """[N,C,2h+1,2w+1] -> the UP conv's phase-planar [N,C,2,2,h+1,WP] (WP = W2E_PLANAR_PITCH(w), include/w2e.h), padding = fill."""
    from where2edit_amd import functional as K
    n, c, ih, iw = t.shape
    hp, wp = (ih + 1) // 2, K.planar_pitch((iw - 1) // 2)
    out = torch.full((n, c, 2, 2, hp, wp), fill, dtype=t.dtype)
    for py in range(2):
        for px in range(2):
            sub = t[:, :, py::2, px::2]
            out[:, :, py, px, :sub.shape[2], :sub.shape[3]] = sub
    return out


def entry_id(e):
    kh, kw = taps_of(e)
    flags = f"act{e['act']}" + ("-planar" if e["planar"] else "") + (f"-xoff{e['xoff']}" if e["xoff"] else "") + (f"-yoff{e['yoff']}" if e["yoff"] else "")
    return (f"{e['kernel']}-{flags}-{kh}x{kw}-u{e['up']}d{e['down']}-{e['planes'][0]}x{e['planes'][1]}-{e['src'][0]}x{e['src'][1]}-"
            f"{e['out'][0]}x{e['out'][1]}-pad{e['pad'][0]}_{e['pad'][1]}" + ("-tune8" if e["tune_blur"] else ""))


WORST = {}  # kernel name -> worst plane error seen by the matrix tests of this run (printed by the last test)


def one_variant_line(err):
    lines = [m for ln in err.splitlines() if (m := FIR_VARIANT.match(ln))]
    return (lines[0] if len(lines) == 1 else None), len(lines)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(FIR_MATRIX)), ids=[entry_id(e) for e in FIR_MATRIX])
def test_fir_variant_against_float64(idx, w2e_opt, capfd):
    """One FIR_MATRIX entry through functional._upfirdn2d_raw with every tap matrix in both flips: the variant line names the kernel
    and flags the entry was written for; the result against float64, globally and per plane; x's NaN guards never read, y's
    sentinel guards never written, every output written."""
    from where2edit_amd import functional as K
    e = FIR_MATRIX[idx]
    (n, c), (in_h, in_w), (out_h, out_w), (pad_x0, pad_y0) = e["planes"], e["src"], e["out"], e["pad"]
    up, down, act, planar = e["up"], e["down"], e["act"], e["planar"]
    g = torch.Generator().manual_seed(1000 + idx)
    x = heavy_planes(g, n, c, in_h, in_w)
    xbuf, xg = guarded(to_planar(x, float("nan")) if planar else x, e["xoff"], float("nan"))
    w2e_opt("tune_blur", e["tune_blur"])
    w2e_opt("tune_print", 1)
    failures, worst, launch = [], 0.0, 0
    for kname, k in tap_matrices(e, g):
        kh, kw = k.shape
        tol = tap_tol(kh, kw)
        kg = k.to(DEV)
        for flip in (0, 1):
            what = f"{entry_id(e)} taps {kname} flip {flip}"
            raw = _fir64(x, k, up, down, pad_x0, pad_y0, flip, out_h, out_w)
            scale = _fir64(x.abs(), k.abs(), up, down, pad_x0, pad_y0, flip, out_h, out_w)
            a = a_dev = None
            if act:  # every other launch in the form a forward uses (no out_scale), the others with all four
                a = epilogue_inputs(g, raw, with_scale=launch % 2 == 0)
                ref, scale = _epilogue64(raw, *a, SLOPE, GAIN, False), _epilogue64(scale, *a, SLOPE, GAIN, True)
                neg, pos = (ref < 0).reshape(n * c, -1).any(1), (ref > 0).reshape(n * c, -1).any(1)
                assert bool(neg.all()) and bool(pos.all()), f"{what}: a plane takes one LeakyReLU branch only"
                a_dev = tuple(None if t is None else t.to(DEV) for t in a)
            else:
                ref = raw
            launch += 1
            ybuf = torch.full((GUARD + e["yoff"] + n * c * out_h * out_w + GUARD,), SENTINEL, device=DEV)
            y = ybuf[GUARD + e["yoff"]:GUARD + e["yoff"] + n * c * out_h * out_w].view(n, c, out_h, out_w)
            y.fill_(float("nan"))
            assert y.data_ptr() % 16 == 4 * e["yoff"]
            torch.cuda.synchronize()
            capfd.readouterr()
            K._upfirdn2d_raw(xg, kg, out_h, out_w, up, down, pad_x0, pad_y0, bool(flip), act=a_dev,
                             planar_hw=(in_h, in_w) if planar else None, out=y)
            torch.cuda.synchronize()
            m, count = one_variant_line(capfd.readouterr().err)
            want = (e["kernel"], act, planar, 0, up, down, kh, kw, n * c, in_h, in_w, out_h, out_w)
            got = (m[1],) + tuple(int(t) for t in m.groups()[1:]) if m else None
            if got != want:
                failures.append(f"{what}: ran {got} ({count} variant lines), written for {want}")
                continue
            if not torch.isfinite(y).all():
                failures.append(f"{what}: {int((~torch.isfinite(y)).sum())} outputs not written, or a NaN guard of x read")
                continue
            if not guards_intact(ybuf, e["yoff"], y.numel(), SENTINEL):
                failures.append(f"{what}: wrote outside y")
            try:
                assert_close(y, ref, tol, what)
                worst = max(worst, assert_close_planes(y, ref, scale, tol, what))
            except AssertionError as err:
                failures.append(str(err).split("\n")[0])
    if not guards_intact(xbuf, e["xoff"], xg.numel(), float("nan")):
        failures.append(f"{entry_id(e)}: x's guards changed")
    name = {"tile4": f"tile4<act {act}>", "blur4": f"blur4<act {act}, planar {planar}>", "stream4": f"stream4<act {act}, planar {planar}>"}.get(e["kernel"], e["kernel"])
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"{entry_id(e)}: worst plane error {worst:.2e} over {launch} launches")
    assert not failures, "\n".join(failures)


# ---- the fused activation backward ------------------------------------------------------------------------------------------------
def _sums_error(sums, ref, absref):
    """[planes,3] fp32 sums against float64, relative to each plane's sum of |terms| (a sum without terms must be exactly 0)."""
    s, ref, absref = sums.double().cpu().reshape(-1, 3), ref.reshape(-1, 3), absref.reshape(-1, 3)
    err = (s - ref).abs()
    assert bool((err[absref == 0] == 0).all()), "a sum without terms is not 0"
    return float((err / absref.clamp_min(1e-300))[absref > 0].max())


@pytest.mark.gpu
@pytest.mark.parametrize("planes,h,w,with_noise", ACTBWD_MATRIX, ids=[f"{p[0]}x{p[1]}-{h}x{w}-noise{int(nz)}" for p, h, w, nz in ACTBWD_MATRIX])
def test_actbwd_stream_against_float64(planes, h, w, with_noise, w2e_opt, capfd):
    """w2e_blur_adjoint_actbwd from the definition: gpre = g * gain * (y_fwd > 0 ? 1 : slope), gt = the adjoint blur (pad 2, un-flipped
    taps) of gpre, sums = (sum gpre * pre, sum gpre * noise, sum gpre) with pre = y_fwd / gain (y_fwd > 0) or y_fwd / (gain * slope), as
    w2e_bias_act_bwd_reduce documents it.  gt to FWD_TOL globally and per plane; the sums per plane against the sum of |terms|, to
    SUMS_TOL, beside the unfused pair's error on the same inputs (printed)."""
    from where2edit_amd._lib import call, ptr, stream_ptr
    n, c = planes
    g = torch.Generator().manual_seed(7 * h + w + int(with_noise))
    gy = heavy_planes(g, n, c, h, w)
    y_fwd = heavy_planes(g, n, c, h, w)
    y_fwd = torch.where(y_fwd > 0, y_fwd, y_fwd * SLOPE) * GAIN  # an activated output: both signs in every plane
    noise = torch.randn(h * w, generator=g) if with_noise else None
    gd, yd = gy.double(), y_fwd.double()
    gpre = gd * GAIN * torch.where(yd > 0, 1.0, SLOPE)
    pre = torch.where(yd > 0, yd / GAIN, yd / (GAIN * SLOPE))
    nz = noise.double().reshape(1, 1, h, w) if with_noise else torch.zeros(1, 1, h, w, dtype=torch.float64)
    terms = (gpre * pre, gpre * nz, gpre)
    sums_ref = torch.stack([t.sum((2, 3)) for t in terms], -1)
    sums_abs = torch.stack([t.abs().sum((2, 3)) for t in terms], -1)
    gyb, gyg = guarded(gy, 0, float("nan"))
    yfb, yfg = guarded(y_fwd, 0, float("nan"))
    nzg = noise.to(DEV) if with_noise else None
    # the unfused pair: the baseline of the sums
    gpre_u, sums_u = torch.empty(n, c, h, w, device=DEV), torch.full((n, c, 3), float("nan"), device=DEV)
    call("w2e_bias_act_bwd_reduce", ptr(gyg), ptr(yfg), ptr(nzg), ptr(gpre_u), ptr(sums_u), n, c, h * w, SLOPE, GAIN, stream_ptr())
    unfused = _sums_error(sums_u, sums_ref, sums_abs)
    w2e_opt("tune_print", 1)
    failures, worst, worst_sums = [], 0.0, 0.0
    e = dict(taps=(4, 4))
    for kname, k in tap_matrices(e, g):
        what = f"actbwd {n}x{c} {h}x{w} noise {int(with_noise)} taps {kname}"
        gt_ref = _fir64(gpre, k, 1, 1, 2, 2, 0, h + 1, w + 1)
        gt_abs = _fir64(gpre.abs(), k.abs(), 1, 1, 2, 2, 0, h + 1, w + 1)
        numel = n * c * (h + 1) * (w + 1)
        gtbuf = torch.full((GUARD + numel + GUARD,), SENTINEL, device=DEV)
        gt = gtbuf[GUARD:GUARD + numel].view(n, c, h + 1, w + 1)
        gt.fill_(float("nan"))
        sums = torch.full((n, c, 3), float("nan"), device=DEV)
        kg = k.to(DEV)
        torch.cuda.synchronize()
        capfd.readouterr()
        call("w2e_blur_adjoint_actbwd", ptr(gyg), ptr(yfg), ptr(nzg), ptr(kg), ptr(gt), ptr(sums), n * c, h, w, SLOPE, GAIN, stream_ptr())
        torch.cuda.synchronize()
        m, count = one_variant_line(capfd.readouterr().err)
        want = ("stream4", 0, 0, 1, 1, 1, 4, 4, n * c, h, w, h + 1, w + 1)
        got = (m[1],) + tuple(int(t) for t in m.groups()[1:]) if m else None
        if got != want:
            failures.append(f"{what}: ran {got} ({count} variant lines), written for {want}")
            continue
        if not (torch.isfinite(gt).all() and torch.isfinite(sums).all()):
            failures.append(f"{what}: outputs not written, or a NaN guard read")
            continue
        if not guards_intact(gtbuf, 0, numel, SENTINEL):
            failures.append(f"{what}: wrote outside gt")
        try:
            assert_close(gt, gt_ref, FWD_TOL, what)
            worst = max(worst, assert_close_planes(gt, gt_ref, gt_abs, FWD_TOL, what))
            fused = _sums_error(sums, sums_ref, sums_abs)
            worst_sums = max(worst_sums, fused)
            assert fused <= SUMS_TOL, f"{what}: sums err {fused:.3e} of the plane's sum of |terms| > {SUMS_TOL:.1e} (the unfused pair: {unfused:.3e})"
        except AssertionError as err:
            failures.append(str(err).split("\n")[0])
    if not (guards_intact(gyb, 0, gy.numel(), float("nan")) and guards_intact(yfb, 0, gy.numel(), float("nan"))):
        failures.append("the guards of gy / y_fwd changed")
    WORST["stream4<actbwd>"] = max(WORST.get("stream4<actbwd>", 0.0), worst)
    WORST["sums, fused"] = max(WORST.get("sums, fused", 0.0), worst_sums)
    WORST["sums, unfused pair"] = max(WORST.get("sums, unfused pair", 0.0), unfused)
    print(f"actbwd {n}x{c} {h}x{w}: worst plane error {worst:.2e}; sums: fused {worst_sums:.2e}, unfused pair {unfused:.2e} (held to {SUMS_TOL:.1e})")
    assert not failures, "\n".join(failures)


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def _no_variant_line(capfd):
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert "upfirdn variant" not in err, err


@pytest.mark.gpu
def test_empty_launches_return_without_a_launch(w2e_opt, capfd):
    from where2edit_amd import functional as K
    from where2edit_amd._lib import call, ptr, stream_ptr
    k4 = seeded.fir_kernel(gain=4.0).to(DEV)
    w2e_opt("tune_print", 1)
    capfd.readouterr()
    y = K._upfirdn2d_raw(torch.empty(0, 3, 64, 64, device=DEV), k4, 65, 65, 1, 1, 2, 2, True)
    assert y.shape == (0, 3, 65, 65)
    y = K._upfirdn2d_raw(torch.randn(1, 2, 64, 64, device=DEV), k4, 0, 65, 1, 1, 2, 2, True)
    assert y.shape == (1, 2, 0, 65)
    e = torch.empty(0, 2, 4, 256, device=DEV)
    call("w2e_blur_adjoint_actbwd", ptr(e), ptr(e), None, ptr(k4), ptr(torch.empty(0, 2, 5, 257, device=DEV)), ptr(torch.empty(0, 2, 3, device=DEV)),
         0, 4, 256, SLOPE, GAIN, stream_ptr())
    _no_variant_line(capfd)


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(w2e_opt, capfd):
    """Argument checks that return with a message before anything is launched."""
    from where2edit_amd import functional as K
    from where2edit_amd._lib import call, ptr, stream_ptr
    x = torch.randn(1, 2, 64, 64, device=DEV)
    k4 = seeded.fir_kernel(gain=4.0).to(DEV)
    w2e_opt("tune_print", 1)
    capfd.readouterr()
    with pytest.raises(RuntimeError, match="kernel 17x3 unsupported"):
        K._upfirdn2d_raw(x, torch.randn(17, 3, device=DEV), 48, 62, 1, 1, 0, 0, True)
    with pytest.raises(RuntimeError, match="up/down must be >= 1"):
        K._upfirdn2d_raw(x, k4, 64, 64, 0, 1, 1, 1, True)
    with pytest.raises(RuntimeError, match="noise without noise_w"):
        K._upfirdn2d_raw(x, k4, 63, 63, 1, 1, 1, 1, True, act=(None, torch.randn(63 * 63, device=DEV), None, torch.randn(2, device=DEV)))
    # a phase-planar input allocated with another row pitch than this library's (functional._upfirdn2d_raw checks the shape itself:
    # straight through the ABI)
    pitch = K.planar_pitch(32)
    planar = torch.zeros(1, 2, 2, 2, 33, pitch + 4, device=DEV)
    y = torch.empty(1, 2, 64, 64, device=DEV)
    with pytest.raises(RuntimeError, match="planar input with a row pitch"):
        call("w2e_upfirdn2d", ptr(planar), ptr(k4), ptr(y), 2, 65, 65, 64, 64, 4, 4, 1, 1, 1, 1, 1, 1, pitch + 4, 0, None, None, None, None, 1,
             SLOPE, GAIN, stream_ptr())
    gy, yf = torch.randn(1, 2, 8, 258, device=DEV), torch.randn(1, 2, 8, 258, device=DEV)
    gt, sums = torch.empty(1, 2, 9, 259, device=DEV), torch.empty(1, 2, 3, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        call("w2e_blur_adjoint_actbwd", ptr(gy), ptr(yf), None, ptr(k4), ptr(gt), ptr(sums), 2, 8, 258, SLOPE, GAIN, stream_ptr())
    gy, yf = torch.randn(1, 2, 8, 256, device=DEV), torch.randn(1, 2, 8, 256, device=DEV)
    gt = torch.empty(1, 2, 9, 257, device=DEV)
    w2e_opt("deterministic", "1")
    with pytest.raises(RuntimeError, match="deterministic mode"):
        call("w2e_blur_adjoint_actbwd", ptr(gy), ptr(yf), None, ptr(k4), ptr(gt), ptr(sums), 2, 8, 256, SLOPE, GAIN, stream_ptr())
    _no_variant_line(capfd)


@pytest.mark.gpu
@pytest.mark.parametrize("h,fusable", [(128, True), (64, False)], ids=["128-to-256", "64-to-128"])
def test_styledconv_backward_takes_the_planned_form(h, fusable, w2e_opt, capfd):
    """One up-sampling styled_conv (B 2, 8 -> 8 channels, h^2 -> (2h)^2) backward under the default options, tune_fuse = 0 and
    deterministic = 1: the variant lines of the backward show the form w2e_blur_adjoint_actbwd_plan answers -- at 256 columns (the
    narrowest the fused pass takes) one stream4<ACTBWD> launch and no separate adjoint blur by default, the unfused pair (an
    `actbwd 0` adjoint blur onto 2h + 1) under the other two; at 128 columns the unfused pair under all three.  The input and style
    gradients of the three agree to the figures tests/test_gpu_parity.py holds the fused pass to against the unfused pair
    (test_blur_adjoint_with_fused_activation_backward: 2e-6 for the image-sized gradient, 2e-5 for what the sums feed)."""
    from helpers import rel_err
    from where2edit_amd import functional as K
    b, k, n = 2, 8, 8
    g = torch.Generator().manual_seed(31 + h)
    wt = torch.randn(n, k, 3, 3, generator=g).to(DEV)
    scale = 1.0 / math.sqrt(k * 9)
    packs = (K.conv_pack(wt, scale, False, False), K.conv_pack(wt, scale, True, False))
    wsq = (wt * scale).square().sum((2, 3)).contiguous()
    kernel = seeded.fir_kernel(gain=4.0).to(DEV)
    noise = torch.randn(1, 1, 2 * h, 2 * h, generator=g).to(DEV)
    nw, bias = torch.full((1,), 0.3, device=DEV), (0.1 * torch.randn(n, generator=g)).to(DEV)
    cot = torch.randn(b, n, 2 * h, 2 * h, generator=g).to(DEV)
    x0, s0 = torch.randn(b, k, h, h, generator=g).to(DEV), (torch.rand(b, k, generator=g) + 0.5).to(DEV)

    def run(option, value):
        if option:
            w2e_opt(option, value)
        want_fused = fusable and option is None
        assert K._blur_actbwd_planned(b * n, 2 * h, 2 * h, kernel.shape) == want_fused
        x, s = x0.clone().requires_grad_(True), s0.clone().requires_grad_(True)
        out = K.styled_conv(x, s, wsq, noise, nw, bias, packs, kernel, True)
        torch.cuda.synchronize()
        w2e_opt("tune_print", 1)
        capfd.readouterr()
        grads = torch.autograd.grad((out * cot).sum(), (x, s))
        torch.cuda.synchronize()
        lines = [m for ln in capfd.readouterr().err.splitlines() if (m := FIR_VARIANT.match(ln))]
        w2e_opt("tune_print", 0)
        if option:
            w2e_opt(option, "" if option == "tune_fuse" else 0)
        got = [(m[1], int(m[4]), int(m[12]), int(m[13])) for m in lines]  # kernel, actbwd, out_h, out_w
        if want_fused:
            assert got == [("stream4", 1, 2 * h + 1, 2 * h + 1)], got
        else:
            assert len(got) == 1 and got[0][1:] == (0, 2 * h + 1, 2 * h + 1), got
        return grads

    default, fuse0, det = run(None, None), run("tune_fuse", 0), run("deterministic", 1)
    for name, other in (("tune_fuse = 0", fuse0), ("deterministic = 1", det)):
        print(f"{2 * h}^2, default against {name}: input gradient {rel_err(default[0], other[0]):.2e}, style gradient {rel_err(default[1], other[1]):.2e}")
    for name, other in (("tune_fuse = 0", fuse0), ("deterministic = 1", det)):
        assert_close(default[0], other[0], 2e-6, f"input gradient, default against {name}")
        assert_close(default[1], other[1], 2e-5, f"style gradient, default against {name}")


@pytest.mark.gpu
def test_zz_measured_errors_of_this_run():
    """Prints the worst per-plane error of each kernel over the matrix tests that ran before it (the figures of the header comment)."""
    for name in sorted(WORST):
        print(f"fir worst: {name}: {WORST[name]:.2e}")
    assert all(v == v for v in WORST.values())
