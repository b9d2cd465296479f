"""Every conv kernel variant the host-side dispatchers can pick, forced one by one and compared with float64.

w2e_modconv3x3 / w2e_conv3x3 pick a mode (SAME, per-phase UP, all-phase UP, DOWN), a tile, a split-K factor, the LDS-DMA or
the register pipeline and an epilogue per launch; w2e_wino_fused picks 4 or 8 matrix waves, the block shape, the XCD block
ownership and how many blocks each persistent workgroup walks.  The matrix below (DIRECT_MATRIX; FUSED_SHAPES x FUSED_MW x
FUSED_LAYOUTS x FUSED_EPIS) is the list of variants these tests run; the census at the end collects the variants real eager steps pick (the library's `tune_print`
"variant" lines) and fails when one of them is not in the matrix -- a cost-model change that starts to pick an untested
variant has to add its case here first.  The same census checks the FIR launches of those steps against the matrix of
tests/test_gpu_fir_variants.py.

Inputs are heavy-tailed (log-normal input-channel scales with x30 outliers, log-normal weight row norms, per-sample in / out
scales 10x apart), and every result is held both to the global max-norm (assert_close) and to a per-plane error relative to
the plane's own term scale (assert_close_planes): an error confined to a small output channel, one border or one sample does
not hide below the largest value of the tensor."""
import math
import os
import re

import pytest
import torch

from helpers import assert_close, assert_close_planes

DEV = "cuda"
FWD_TOL = 1e-4  # tests/test_gpu_parity.py: forward results against float64
DOT_TOL = 5e-4  # the fused per-channel dot vector under the global max-norm, as in tests/test_gpu_parity.py (a sum with cancellation);
#                 its per-channel error against the sum of |terms| is held to FWD_TOL
# The per-plane error is held to FWD_TOL everywhere, the Winograd forms included.  Measured on an MI355X over this file's cases
# (worst plane, relative to the plane's own term scale): direct kernels 5.4e-7, fused Winograd 8.7e-6, GEMM form at K = 512 1.8e-6.

# ---- the variant matrix -----------------------------------------------------------------------------------------------------------
# DOWN: tiles 1, 2 and 8 need more patch slots than DOWN's prefetch registers hold (the library refuses them when forced)
DOWN_TILES = (0, 3, 4, 5, 6, 7, 9, 10)
# name -> (mode, all-phase, tiles, tiles run with AND without the LDS-DMA pipeline, epilogues, split-K requests)
# (DMA: every tile it is instantiated for, where its two LDS stages fit: DOWN's tiles 0 / 10 never fit -- they keep the register
# pipeline; the per-phase UP form and the bias + PReLU epilogue have no DMA form)
DIRECT_MATRIX = {
    "same": (0, 0, tuple(range(11)), (0, 1, 2, 8, 9, 10), ("plain", "act", "dot"), (1, 3)),
    "up": (1, 0, tuple(range(11)), (), ("plain",), (1, 2)),
    "upall": (1, 1, (0, 1, 2, 4, 8, 11), (0, 1, 2, 8, 11), ("plain",), (1, 3)),
    "down": (2, 0, DOWN_TILES, (9,), ("plain", "dot"), (1, 3)),
    "same_prelu": (0, 0, tuple(range(11)), (), ("prelu",), (1, 3)),
    "down_prelu": (2, 0, DOWN_TILES, (), ("prelu",), (1, 3)),
}
# a split activation / bias + PReLU runs as the plain kernel and one elementwise pass (the library's "variant" line says so)
SPLIT_EPI = {"act": "act_pass", "prelu": "prelu_pass"}
# shapes (b, k, n, h, w): odd sizes, K and N no multiple of any tile; h, w = output size for DOWN, input size otherwise.
# K = 37: split 3 (SAME / DOWN / all-phase UP, 8-channel slices) = 16 + 16 + 5, split 2 (per-phase UP, 16-channel slices) = 32 + 5
DIRECT_SHAPES = {"same": (2, 37, 70, 19, 45), "up": (2, 37, 70, 13, 19), "down": (2, 37, 70, 11, 21)}

# fused Winograd kernel: block shape TXN -> shape (b, k, n, h, w).  TXN 8: W % 64 != 0, 3 blocks per image, 48 blocks;
# TXN 16: 4 blocks per image, 24 blocks.  Neither image size is a multiple of an XCD's eighth of the blocks, so with xmap the
# block sequence of some workgroup crosses an image boundary (and with round-robin ownership every sequence does)
FUSED_SHAPES = {8: (16, 32, 64, 16, 96), 16: (6, 128, 64, 32, 64)}
FUSED_MW = (4, 8)
# layout -> (tune_xcd, K.FUSED_WGS by TXN, expected xmap, several blocks per workgroup)
FUSED_LAYOUTS = {
    "one": (0, {8: 0, 16: 0}, 0, False),
    "several": (0, {8: 5, 16: 5}, 0, True),
    "xmap_one": (1, {8: 0, 16: 0}, 1, False),
    "xmap_several": (1, {8: 16, 16: 8}, 1, True),
}
FUSED_EPIS = ("plain", "act", "prelu", "dot")
FUSED_ACT = {"plain": 0, "act": 1, "prelu": 2, "dot": 0}

# the GEMM form's K splits the production plan uses at K = 512 (the 2 / 3-way splits are in tests/test_gpu_parity.py)
GEMM_SPLITS = (8, 16)

VARIANT = re.compile(r"modconv variant mode (\d) all (\d) cfg (\d+) splits (\d+) dma (\d) x3 (\d) epi (\w+)")
FUSED_VARIANT = re.compile(r"wino_fused variant act (\d) dot (\d) txn (\d+) mw (\d) xmap (\d) grid (\d+)x(\d+) blocks (\d+)")
MODE_LINE = re.compile(r"modconv mode (\d)( \(all-phase\))? K \d+ N \d+ \d+x\d+ B \d+ -> cfg (\d+) splits (\d+)")


def direct_cases(name):
    """(tile, split request, dma, epilogue) of every launch the matrix runs for one DIRECT_MATRIX entry."""
    _, _, tiles, dma_tiles, epis, splits = DIRECT_MATRIX[name]
    for cfg in tiles:
        for sp in splits:
            for dma in ((0, 1) if cfg in dma_tiles else (0,)):
                for epi in epis:
                    yield cfg, sp, dma, epi


def direct_key(mode, all_phase, cfg, splits, dma, x3, epi):
    return (mode, all_phase, cfg, splits > 1, dma, x3, epi)


def covered_direct():
    keys = set()
    for name, (mode, all_phase, *_rest) in DIRECT_MATRIX.items():
        for cfg, sp, dma, epi in direct_cases(name):
            keys.add(direct_key(mode, all_phase, cfg, sp, dma, 0, SPLIT_EPI.get(epi, epi) if sp > 1 else epi))
    return keys


def fused_key(act, dot, txn, mw, xmap, several):
    return (act, dot, txn, mw, xmap, several)


def covered_fused():
    return {fused_key(FUSED_ACT[epi], int(epi == "dot"), txn, mw, lay[2], lay[3])
            for txn in FUSED_SHAPES for mw in FUSED_MW for lay in FUSED_LAYOUTS.values() for epi in FUSED_EPIS}


def parse_variants(lines):
    """Variant keys of the library's tune_print output, each with the layer line it belongs to: [(kind, key, layer line)]."""
    out, layer = [], None
    for ln in lines:
        if ln.startswith("modconv mode"):
            layer = ln
        elif (m := VARIANT.match(ln)):
            mode, all_phase, cfg, splits, dma, x3 = (int(v) for v in m.groups()[:6])
            out.append(("direct", direct_key(mode, all_phase, cfg, splits, dma, x3, m[7]), layer))
        elif (m := FUSED_VARIANT.match(ln)):
            act, dot, txn, mw, xmap, gx, _, blocks = (int(v) for v in m.groups())
            out.append(("fused", fused_key(act, dot, txn, mw, xmap, blocks > gx), ln))
    return out


def census_misses(found):
    """found: [(kind, key, layer line, where)] -> one message per variant that is not in the matrix."""
    covered = {"direct": covered_direct(), "fused": covered_fused()}
    misses = {}
    for kind, key, layer, where in found:
        if key not in covered[kind] and key not in misses:
            misses[key] = (f"{kind} variant {key} ({'mode, all-phase, cfg, split, dma, x3, epi' if kind == 'direct' else 'act, dot, txn, mw, xmap, several blocks'}) "
                           f"picked by `{layer}` at {where} has no case in the matrix of tests/test_gpu_conv_variants.py: add one")
    return list(misses.values())


# ---- inputs and float64 references --------------------------------------------------------------------------------------------------
SAMPLE_IN = (1.0, 12.0, 0.08)    # per-sample factor of s_in (cycled): any two of them are >= 10x apart
SAMPLE_OUT = (1.0, 1 / 15, 15.0)  # and of s_out


def heavy_inputs(seed, b, k, n, xh, xw):
    """x [b,k,xh,xw], weight [n,k,3,3], s_in [b,k], s_out [b,n]: log-normal (sigma 1.5) input-channel scales with three x30
    outlier channels, log-normal weight row norms, per-sample scale tables >= 10x apart between samples."""
    g = torch.Generator().manual_seed(seed)
    cs = torch.exp(1.5 * torch.randn(k, generator=g))
    cs[torch.randperm(k, generator=g)[:3]] *= 30.0
    x = torch.randn(b, k, xh, xw, generator=g) * cs[None, :, None, None]
    wt = torch.randn(n, k, 3, 3, generator=g)
    wt = wt / wt.flatten(1).norm(dim=1)[:, None, None, None] * torch.exp(1.5 * torch.randn(n, generator=g))[:, None, None, None]
    fi = torch.tensor([SAMPLE_IN[i % 3] for i in range(b)])
    fo = torch.tensor([SAMPLE_OUT[i % 3] for i in range(b)])
    s_in = (torch.rand(b, k, generator=g) + 0.5) * fi[:, None]
    s_out = (torch.rand(b, n, generator=g) + 0.5) * fo[:, None]
    return g, x.to(DEV), wt.to(DEV), s_in.to(DEV), s_out.to(DEV)


def conv_refs(op, x, wt, s_in, s_out):
    """(ref, absref, raw, absraw) of y = op(x * s_in, w) * s_out in float64: absref is the same op on |x * s_in| and |w|, times
    |s_out| -- the scale of the terms each output sums; raw / absraw without s_out (what the fused dot multiplies)."""
    xd = x.double() * s_in.double()[:, :, None, None]
    so = s_out.double()[:, :, None, None]
    raw, absraw = op(xd, wt.double()), op(xd.abs(), wt.double().abs())
    return raw * so, absraw * so.abs(), raw, absraw


def act_refs(ref, absref, noise, nw, bias):
    """StyledConv epilogue lrelu(y + nw * noise + bias, 0.2) * sqrt(2) and its term scale."""
    import torch.nn.functional as F
    pre = ref + nw.double() * noise.double() + bias.double()[None, :, None, None]
    scale = absref + (nw.double() * noise.double()).abs() + bias.double().abs()[None, :, None, None]
    return F.leaky_relu(pre, 0.2) * 2 ** 0.5, scale * 2 ** 0.5


def prelu_refs(ref, absref, bias, slope):
    """bias + PReLU epilogue prelu(y + bias[o], slope[o]) and its term scale."""
    pre = ref + bias.double()[None, :, None, None]
    sl = slope.double()[None, :, None, None]
    return torch.where(pre > 0, pre, sl * pre), (absref + bias.double().abs()[None, :, None, None]) * torch.clamp(sl.abs(), min=1.0)


def dot_refs(raw, absraw, dw):
    """dot[b,o] = sum_p raw * dot_with as [b,n,1,1] planes, and the sum of |terms|."""
    d = dw.double()
    return (raw * d).sum((2, 3))[:, :, None, None], (absraw * d.abs()).sum((2, 3))[:, :, None, None]


def channel_bias(g, absref, frac):
    """A per-channel bias on the scale of that channel's outputs (a bias far above a small channel would hide its error)."""
    return (frac * torch.randn(absref.shape[1], generator=g).to(DEV).double() * absref.mean((0, 2, 3))).float()


# ---- the direct kernels ---------------------------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


def _expected_splits(mode, all_phase, k, sp):
    """The K slices a split request `sp` becomes: slices of whole 8-channel chunks (per-phase UP: 16), the last one ragged."""
    gran = 16 if (mode == 1 and not all_phase) else 8
    return _ceil_div(k, _ceil_div(_ceil_div(k, sp), gran) * gran)


class DirectProblem:
    """One shape of one DIRECT_MATRIX entry: inputs, float64 references of every epilogue, and run(epi) -> (y, dot, canary ok)."""

    CANARY = 1234.5
    TAIL = 4096

    def __init__(self, name):
        import torch.nn.functional as F
        from where2edit_amd import functional as K
        self.name = name
        self.mode, self.all_phase = DIRECT_MATRIX[name][:2]
        b, k, n, h, w = DIRECT_SHAPES[{0: "same", 1: "up", 2: "down"}[self.mode]]
        self.b, self.k, self.n, self.h, self.w = b, k, n, h, w
        self.prelu = name.endswith("_prelu")
        self.down_pad = 1 if self.prelu and self.mode == 2 else 0
        xh, xw = {0: (h, w), 1: (h, w), 2: (2 * h + 1 - self.down_pad, 2 * w + 1 - self.down_pad)}[self.mode]
        g, self.x, wt, self.s_in, self.s_out = heavy_inputs(list(DIRECT_MATRIX).index(name) + 7 * k + n, b, k, n, xh, xw)
        self.pack = K.conv_pack(wt, 1.0, False, False)  # [out, in] weight (UP: the transposed conv's [in, out] weight, permuted)
        if self.mode == 1:
            op = lambda a, ww: F.conv_transpose2d(a, ww.permute(1, 0, 2, 3), stride=2)  # noqa: E731
            self.out_shape = (b, n, 2, 2, h + 1, K.planar_pitch(w))
        else:
            op = (lambda a, ww: F.conv2d(a, ww, padding=1)) if self.mode == 0 else (
                (lambda a, ww: F.conv2d(a, ww, stride=2, padding=1)) if self.down_pad else (lambda a, ww: F.conv2d(a, ww, stride=2)))
            self.out_shape = (b, n, h, w)
        ref, absref, raw, absraw = conv_refs(op, self.x, wt, self.s_in, self.s_out)
        self.refs = {"plain": (ref, absref)}
        self.noise = torch.randn(1, 1, h, w, generator=g).to(DEV)
        self.nw = torch.full((1,), 0.01, device=DEV)
        self.bias = channel_bias(g, absref, 0.3)
        self.slope = (0.25 * torch.randn(n, generator=g)).to(DEV)
        self.dw = torch.randn(*ref.shape, generator=g).to(DEV)
        if self.mode == 0:
            self.refs["act"] = act_refs(ref, absref, self.noise, self.nw, self.bias)
        if self.prelu:
            self.refs["prelu"] = prelu_refs(ref, absref, self.bias, self.slope)
        self.refs["dot"] = (ref, absref)
        self.dot_ref = dot_refs(raw, absraw, self.dw)

    def run(self, epi):
        """One launch into the head of a canary-filled buffer: (y as the plain image, dot or None, the buffer)."""
        from where2edit_amd import functional as K
        from where2edit_amd import irse_hip
        from where2edit_amd._lib import call, ptr, stream_ptr
        numel = math.prod(self.out_shape)
        buf = torch.full((numel + self.TAIL,), self.CANARY, device=DEV)
        y = buf[:numel].view(self.out_shape)
        b, k, n, h, w = self.b, self.k, self.n, self.h, self.w
        dot = None
        if self.prelu:
            irse_hip.conv3x3(self.x, self.pack, n, h, w, mode=self.mode, down_pad=self.down_pad, in_scale=self.s_in, out_scale=self.s_out,
                             bias=self.bias, slope=self.slope, out=y, form=0)
        else:
            act = epi == "act"
            dot = torch.zeros(b, n, device=DEV) if epi == "dot" else None
            call("w2e_modconv3x3", self.mode, ptr(self.x), ptr(self.pack), ptr(self.s_in), ptr(self.s_out), ptr(y), b, k, n, h, w,
                 self.out_shape[-1] if self.mode == 1 else 0, int(act), ptr(self.noise) if act else None, ptr(self.nw) if act else None,
                 ptr(self.bias) if act else None, ptr(self.dw) if dot is not None else None, ptr(dot), stream_ptr())
        torch.cuda.synchronize()
        img = K.unplanar(y, w) if self.mode == 1 else y
        return img, dot, buf

    def canary_errors(self, buf, splits):
        """Nothing behind the output may change; UP: nor the pad columns W+1 .. pitch-1 of the phase-planar rows (a split launch
        zeroes the whole planar buffer first, so there they must be 0)."""
        numel = math.prod(self.out_shape)
        errs = []
        if not torch.all(buf[numel:] == self.CANARY):
            errs.append("wrote past the end of the output")
        if self.mode == 1:
            pad = buf[:numel].view(self.out_shape)[..., self.w + 1:]
            want = 0.0 if splits > 1 else self.CANARY
            if pad.numel() and not torch.all(pad == want):
                errs.append(f"wrote the pad columns past W+1 of the phase-planar rows ({int((pad != want).sum())} values)")
        return errs


def _variant_lines(err, pattern):
    return [m for ln in err.splitlines() if (m := pattern.match(ln))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DIRECT_MATRIX))
def test_direct_conv_variants_against_float64(name, w2e_opt, capfd):
    """Every (tile, split, pipeline, epilogue) of one mode of the direct kernel, forced through tune_cfg / tune_upall / tune_dma, on a
    ragged heavy-tailed shape: against float64 (global and per-plane), against the library's own choice for the shape, nothing
    written outside the output, and the variant line of the launch says the forced variant is the one that ran."""
    prob = DirectProblem(name)
    mode, all_phase = prob.mode, prob.all_phase
    if mode == 1:
        w2e_opt("tune_upall", all_phase)
    defaults = {}
    for epi in DIRECT_MATRIX[name][4]:
        defaults[epi] = prob.run(epi)[:2]
    failures, worst = [], 0.0
    w2e_opt("tune_print", 1)
    capfd.readouterr()
    for cfg, sp, dma, epi in direct_cases(name):
        what = f"{name} cfg {cfg} split {sp} dma {dma} {epi}"
        w2e_opt("tune_cfg", f"{cfg},{sp},{mode}")
        w2e_opt("tune_dma", dma)
        y, dot, buf = prob.run(epi)
        lines = _variant_lines(capfd.readouterr().err, VARIANT)
        splits = _expected_splits(mode, all_phase, prob.k, sp)
        want = (mode, all_phase, cfg, splits, dma, 0, SPLIT_EPI.get(epi, epi) if splits > 1 else epi)
        got = tuple(int(v) for v in lines[-1].groups()[:6]) + (lines[-1][7],) if len(lines) == 1 else None
        if got != want:
            failures.append(f"{what}: ran {got} ({len(lines)} variant lines), asked for {want}")
            continue
        ref, absref = prob.refs[epi]
        try:
            assert_close(y, ref, FWD_TOL, what)
            worst = max(worst, assert_close_planes(y, ref, absref, FWD_TOL, what))
            assert_close(y, defaults[epi][0], FWD_TOL, what + " vs the library's own choice")
            if dot is not None:
                assert_close(dot, prob.dot_ref[0][:, :, 0, 0], DOT_TOL, what + " dot")
                assert_close_planes(dot[:, :, None, None], *prob.dot_ref, FWD_TOL, what + " dot per channel")
                assert_close(dot, defaults[epi][1], DOT_TOL, what + " dot vs the library's own choice")
        except AssertionError as e:
            failures.append(str(e).split("\n")[0])
        failures += [f"{what}: {e}" for e in prob.canary_errors(buf, splits)]
    print(f"{name}: worst plane error {worst:.2e} over {len(list(direct_cases(name)))} variants")
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,cfg,all_phase", [(2, 1, 0), (2, 2, 0), (2, 8, 0), (1, 3, 1), (1, 9, 1)])
def test_forced_tile_that_does_not_fit_is_refused(mode, cfg, all_phase, w2e_opt):
    """A tile forced through tune_cfg passes the selection's own feasibility filters (LDS, patch slots, DOWN's slot cap, an all-phase
    form): one beyond them is refused before anything is launched, never run on a part of its patch."""
    from where2edit_amd import functional as K
    b, k, n, h, w = 2, 16, 32, 9, 13
    x = torch.randn(b, k, 2 * h + 1, 2 * w + 1, device=DEV) if mode == 2 else torch.randn(b, k, h, w, device=DEV)
    pack = K.conv_pack(torch.randn(n, k, 3, 3, device=DEV), 1.0, False, False)
    if mode == 1:
        w2e_opt("tune_upall", all_phase)
    w2e_opt("tune_cfg", f"{cfg},1,{mode}")
    with pytest.raises(RuntimeError, match="forced by tune_cfg|has no all-phase form"):
        K._modconv_raw(mode, x, pack, None, None, h, w)


# ---- the fused Winograd kernel --------------------------------------------------------------------------------------------------------
def _fused_run(K, irse_hip, epi, p):
    if epi == "prelu":
        b, k, n, h, w = p["shape"]
        return irse_hip.conv3x3(p["x"], p["pack"], n, h, w, in_scale=p["s_in"], out_scale=p["s_out"], bias=p["bias"], slope=p["slope"], form=8), None
    h, w = p["shape"][3:]
    if epi == "dot":
        return K._modconv_raw(K.MODE_SAME, p["x"], p["pack"], p["s_in"], p["s_out"], h, w, dot_with=p["dw"])
    act = (p["noise"], p["nw"], p["bias"]) if epi == "act" else None
    return K._modconv_raw(K.MODE_SAME, p["x"], p["pack"], p["s_in"], p["s_out"], h, w, act=act)


@pytest.mark.gpu
@pytest.mark.parametrize("txn", sorted(FUSED_SHAPES))
@pytest.mark.parametrize("mw", FUSED_MW)
def test_fused_winograd_variants_against_float64(mw, txn, w2e_opt, capfd):
    """w2e_wino_fused with 4 and 8 matrix waves (the 768-thread form's half-0 matrix waves run output items), both block shapes,
    round-robin and XCD-contiguous block ownership, one and several blocks per persistent workgroup (sequences that cross an
    image boundary: the next block's in_scale table is another sample's), every epilogue: against float64 (global and per
    plane), against the library's own choice, and the variant line says the forced variant is the one that ran."""
    import torch.nn.functional as F
    from where2edit_amd import functional as K
    from where2edit_amd import irse_hip
    b, k, n, h, w = FUSED_SHAPES[txn]
    g, x, wt, s_in, s_out = heavy_inputs(1000 + txn, b, k, n, h, w)
    ref, absref, raw, absraw = conv_refs(lambda a, ww: F.conv2d(a, ww, padding=1), x, wt, s_in, s_out)
    p = dict(shape=(b, k, n, h, w), x=x, s_in=s_in, s_out=s_out, pack=K.conv_pack(wt, 1.0, False, False),
             noise=torch.randn(1, 1, h, w, generator=g).to(DEV), nw=torch.full((1,), 0.01, device=DEV), bias=channel_bias(g, absref, 0.3),
             slope=(0.25 * torch.randn(n, generator=g)).to(DEV), dw=torch.randn(b, n, h, w, generator=g).to(DEV))
    refs = {"plain": (ref, absref), "dot": (ref, absref), "act": act_refs(ref, absref, p["noise"], p["nw"], p["bias"]),
            "prelu": prelu_refs(ref, absref, p["bias"], p["slope"])}
    dref = dot_refs(raw, absraw, p["dw"])
    saved, saved_wgs = K.WINOGRAD, K.FUSED_WGS
    failures, worst = [], 0.0
    try:
        K.set_winograd(K.FUSED)
        K.FUSED_WGS = 0
        defaults = {epi: _fused_run(K, irse_hip, epi, p) for epi in FUSED_EPIS}
        w2e_opt("tune_mw", mw)
        w2e_opt("tune_print", 1)
        capfd.readouterr()
        for lay, (xcd, wgs, xmap, several) in FUSED_LAYOUTS.items():
            w2e_opt("tune_xcd", xcd)
            K.FUSED_WGS = wgs[txn]
            for epi in FUSED_EPIS:
                what = f"fused mw {mw} txn {txn} {lay} {epi}"
                y, dot = _fused_run(K, irse_hip, epi, p)
                torch.cuda.synchronize()
                lines = _variant_lines(capfd.readouterr().err, FUSED_VARIANT)
                want = fused_key(FUSED_ACT[epi], int(epi == "dot"), txn, mw, xmap, several)
                got = None
                if len(lines) == 1:
                    act, d, t, m, xm, gx, _, blocks = (int(v) for v in lines[0].groups())
                    got = fused_key(act, d, t, m, xm, blocks > gx)
                if got != want:
                    failures.append(f"{what}: ran {got} ({len(lines)} variant lines), asked for {want}")
                    continue
                r, ar = refs[epi]
                try:
                    assert_close(y, r, FWD_TOL, what)
                    worst = max(worst, assert_close_planes(y, r, ar, FWD_TOL, what))
                    assert_close(y, defaults[epi][0], FWD_TOL, what + " vs the library's own choice")
                    if dot is not None:
                        assert_close(dot, dref[0][:, :, 0, 0], DOT_TOL, what + " dot")
                        assert_close_planes(dot[:, :, None, None], *dref, FWD_TOL, what + " dot per channel")
                        assert_close(dot, defaults[epi][1], DOT_TOL, what + " dot vs the library's own choice")
                except AssertionError as e:
                    failures.append(str(e).split("\n")[0])
    finally:
        K.set_winograd(saved)
        K.FUSED_WGS = saved_wgs
    print(f"fused mw {mw} txn {txn}: worst plane error {worst:.2e}")
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("splits", GEMM_SPLITS)
def test_wino_gemm_production_k_splits(splits):
    """The GEMM form with the K splits its plan picks in production at K = 512 (8 at 16^2 batch 8, 16 at 16^2 batch 4), plain, with the
    StyledConv epilogue and with the fused dot: against float64, global and per plane."""
    import torch.nn.functional as F
    from where2edit_amd import functional as K
    b, k, n, h, w = 3, 512, 64, 16, 16
    g, x, wt, s_in, s_out = heavy_inputs(2000 + splits, b, k, n, h, w)
    ref, absref, raw, absraw = conv_refs(lambda a, ww: F.conv2d(a, ww, padding=1), x, wt, s_in, s_out)
    pack = K.conv_pack(wt, 1.0, False, False)
    noise, nw, bias = torch.randn(1, 1, h, w, generator=g).to(DEV), torch.full((1,), 0.01, device=DEV), channel_bias(g, absref, 0.3)
    dw = torch.randn(b, n, h, w, generator=g).to(DEV)
    saved, saved_s = K.WINOGRAD, K.GEMM_SPLITS
    try:
        K.set_winograd(4)
        K.GEMM_SPLITS = splits
        K.WINO_LOG = []
        y, _ = K._modconv_raw(K.MODE_SAME, x, pack, s_in, s_out, h, w)
        assert_close(y, ref, FWD_TOL, "gemm form")
        e0 = assert_close_planes(y, ref, absref, FWD_TOL, "gemm form")
        ya, _ = K._modconv_raw(K.MODE_SAME, x, pack, s_in, s_out, h, w, act=(noise, nw, bias))
        ra, aa = act_refs(ref, absref, noise, nw, bias)
        assert_close(ya, ra, FWD_TOL, "gemm form + act")
        e1 = assert_close_planes(ya, ra, aa, FWD_TOL, "gemm form + act")
        yd, dot = K._modconv_raw(K.MODE_SAME, x, pack, s_in, s_out, h, w, dot_with=dw)
        assert_close(yd, ref, FWD_TOL, "gemm form, dot epilogue y")
        dr, da = dot_refs(raw, absraw, dw)
        assert_close(dot, dr[:, :, 0, 0], DOT_TOL, "gemm form dot")
        assert_close_planes(dot[:, :, None, None], dr, da, FWD_TOL, "gemm form dot per channel")
        log = K.WINO_LOG
    finally:
        K.set_winograd(saved)
        K.GEMM_SPLITS, K.WINO_LOG = saved_s, None
    assert len(log) == 3 and all(f"{splits} K split(s)" in ln and "gemm" in ln for ln in log), log
    print(f"gemm form, {splits} K splits: worst plane error {max(e0, e1):.2e}")


# ---- the census --------------------------------------------------------------------------------------------------------------------
CENSUS_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r05_bench_cfg_selections.txt")


def recorded_direct_keys(lines):
    """(key without epi, layer line) of every direct launch in a tools/cfg_selections.py record (the lines before the variant line
    existed: the tile, split and pipeline come from the "modconv mode" line and its "  lds-dma" / "  bf16x3" lines)."""
    out, cur = [], None
    for ln in lines + ["#"]:
        if ln.startswith("  lds-dma pipeline:") and cur:
            cur[1][4] = int(ln.split(":")[1].strip().startswith("yes"))
        elif ln.startswith("  bf16x3:") and cur:
            cur[1][5] = int(ln.split(":")[1].strip().startswith("yes"))
        else:
            if cur:
                out.append((tuple(cur[1]), cur[0]))
            cur = None
            m = MODE_LINE.match(ln)
            if m:
                cur = (ln, [int(m[1]), int(bool(m[2])), int(m[3]), int(m[4]) > 1, 0, 0])
    return out


def test_census_of_the_recorded_bench_selections():
    """The tile selections recorded from the benchmark's steps (profiles/r05_bench_cfg_selections.txt: workload 2 at batch 4 and 8,
    workload 3 at batch 8) are all in the matrix -- keyed without the epilogue, which that record predates.  Runs without a GPU."""
    covered = {key[:6] for key in covered_direct()}
    lines = open(CENSUS_FILE).read().splitlines()
    rec = recorded_direct_keys(lines)
    assert len(rec) >= 100, f"parsed only {len(rec)} launches from {CENSUS_FILE}"
    misses = {}
    for key, layer in rec:
        if key not in covered and key not in misses:
            misses[key] = (f"direct variant {key} (mode, all-phase, cfg, split, dma, x3) picked by `{layer}` has no case in the matrix of "
                           f"tests/test_gpu_conv_variants.py: add one")
    assert not misses, "\n".join(misses.values())


def _census_steps():
    """(where, fn) of the eager steps whose variants the census collects (each built lazily: one 1024^2 model set at a time)."""
    import bench
    dev = "cuda:0"
    for workload, batches in ((2, (1, 2, 4, 8)), (3, (2, 8))):
        coach = bench.build_coach(1024, max(batches), dev, False, "hip", workload)
        for b in batches:
            w = bench.synthetic_latents(coach.net.decoder, b, 0)
            mask = bench.make_mask(coach, b, 1024, 0, dev) if workload == 3 else None
            yield (f"workload {workload} batch {b}", lambda: coach.train_step(w, mask))
        if workload == 2:  # the paths the default steps do not take, on the same model set
            yield ("workload 2 batch 2, deterministic mode", lambda: _deterministic_step(coach, bench.synthetic_latents(coach.net.decoder, 2, 0)))
            yield ("generator batch 1, train_conv_weights", lambda: _conv_weight_step(coach.net.decoder, bench.synthetic_latents(coach.net.decoder, 1, 0)))
        del coach
        torch.cuda.empty_cache()
    from where2edit_amd.demo_pipeline import invert_and_edit
    imgs, e4e, g, clip, net, text, att = bench.build_config5(dev, 4, 0)
    for b in (1, 4):
        yield (f"workload 5 batch {b}", lambda: invert_and_edit(imgs[:b], e4e, g, clip, net, text[:b], att[:b], attention_layer=13))
    del imgs, e4e, g, clip, net
    torch.cuda.empty_cache()
    yield ("discriminator 1024^2 batch 1, forward and backward", _discriminator_step)
    torch.cuda.empty_cache()


def _deterministic_step(coach, w):
    """One step in deterministic mode: the unfused activation backward + adjoint blur instead of w2e_blur_adjoint_actbwd."""
    from where2edit_amd import _lib
    _lib.set_option("deterministic", "1")
    try:
        coach.train_step(w)
    finally:
        _lib.set_option("deterministic", os.environ.get("W2E_DETERMINISTIC", "0"))


def _conv_weight_step(decoder, w):
    """Generator forward + backward into the conv weights (stylegan2.train_conv_weights); the decoder is frozen again afterwards."""
    from where2edit_amd.stylegan2 import freeze_conv_weights, train_conv_weights
    train_conv_weights(decoder)
    try:
        img, _ = decoder([w.detach()], input_is_latent=True, randomize_noise=False)
        img.square().mean().backward()
        torch.cuda.synchronize()
    finally:
        freeze_conv_weights(decoder)
        for p in decoder.parameters():
            p.grad = None


def _discriminator_step():
    import disc64
    from where2edit_amd.stylegan2 import Discriminator
    d = Discriminator(1024, 2)
    d.load_state_dict(disc64.state_dict(1024, 2, salt=3), strict=True)
    d = d.to("cuda:0")
    x = disc64.images(1, 1024, salt=3).to("cuda:0").requires_grad_(True)
    (d(x) * disc64.cotangent(1, salt=3).to("cuda:0")).sum().backward()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_census_every_variant_real_steps_pick_is_in_the_matrix():
    """The variants the library picks in real eager steps -- workload 2 at batch 1, 2, 4, 8, workload 3 at batch 2, 8, the workload-5
    pipeline at batch 1, 4 -- are all among the variants this file tests against float64; and the FIR variants ("upfirdn variant"
    lines) of the same steps, of a deterministic-mode step, of a conv-weight-gradient step and of a Discriminator forward and
    backward are all in the matrix of tests/test_gpu_fir_variants.py."""
    from test_gpu_fir_variants import covered_fir, parse_fir_variants
    from where2edit_amd.profiling import conv_selections
    found, seen = [], {}
    fir_seen = {}
    for where, fn in _census_steps():
        lines, _ = conv_selections(fn)
        variants = parse_variants(lines)
        assert variants, f"{where}: no variant lines"
        for kind, key, layer in variants:
            found.append((kind, key, layer, where))
            seen.setdefault((kind, key), []).append(where)
        fir = parse_fir_variants(lines)
        assert fir, f"{where}: no upfirdn variant lines"
        for key, line in fir:
            fir_seen.setdefault(key, []).append((where, line))
    for (kind, key), wheres in sorted(seen.items(), key=str):
        print(f"census: {kind} {key}: {len(wheres)} launches, {', '.join(sorted(set(wheres)))}")
    for key, hits in sorted(fir_seen.items(), key=str):
        print(f"census: fir {key}: {len(hits)} launches, {', '.join(sorted({wh for wh, _ in hits}))}")
    misses = census_misses(found)
    covered = covered_fir()
    misses += [f"fir variant {key} (kernel, act, planar, actbwd, up, down, taps, out_w class) picked by `{hits[0][1]}` at {hits[0][0]} has no entry in "
               f"the matrix of tests/test_gpu_fir_variants.py: add one" for key, hits in sorted(fir_seen.items(), key=str) if key not in covered]
    assert not misses, "\n".join(misses)
