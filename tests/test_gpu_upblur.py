"""The up-sampling StyledConv in one launch (w2e_modconv_upblur: all-phase UP conv, tile {1,8,1,8}, with the 4x4 blur, noise, bias
and LeakyReLU in the tile's epilogue) against float64, against the two-launch form it replaces (w2e_modconv3x3 UP +
w2e_upfirdn2d), and through the unchanged backward; and a census: every "modconv upblur variant" line real eager steps print is a
key of this file's matrix.

The form's tile is 16 x 32 input positions and owns SY x SX = 14 x 30 of them (the rest is the blur's recomputed halo).  Shapes:
smaller than one tile, exactly one, one more row / column (a second tile of one row / column), several ragged tiles with ragged
channel counts -- each with noise + bias and with both null -- and one even-width multi-tile shape, because only an even width
with 16-byte aligned tensors takes the float4 stores the 1024^2 layer runs with."""
import math
import re

import pytest
import torch

from helpers import assert_close, assert_close_planes, rel_err
from test_gpu_conv_variants import heavy_inputs
from upblur_ref import upblur_ref

DEV = "cuda"
FWD_TOL = 1e-4   # the project's forward tolerance against float64 (tests/test_gpu_parity.py)
GRAD_TOL = 1e-3  # and its gradient tolerance
SY, SX = 14, 30  # input positions a tile owns
# (h, w, K, N)
SHAPES = {
    "sub_tile": (5, 7, 16, 32),
    "one_tile": (SY, SX, 16, 32),
    "second_tile": (SY + 1, SX + 1, 16, 32),
    "ragged": (2 * SY + 3, 2 * SX + 5, 37, 70),
    "ragged_even": (2 * SY + 3, 2 * SX + 4, 16, 32),
}
UPBLUR_VARIANT = re.compile(r"modconv upblur variant cfg (\d+) th (\d+) tw (\d+) groups (\d+) vec (\d)")
# variant keys (cfg, th, tw, groups, vec) this matrix runs: vec = 1 (float4 stores) needs an even width
MATRIX_KEYS = {(11, 16, 32, 2, 0), (11, 16, 32, 2, 1)}
CANARY, TAIL = 1234.5, 4096  # TAIL a multiple of 4 floats: the output inside the canary buffer stays 16-byte aligned


class Problem:
    """One shape: inputs (batch 2, styles 12x apart), the float64 reference with and without noise + bias, both forms' runs."""

    def __init__(self, name):
        from where2edit_amd import functional as K
        self.h, self.w, self.k, self.n = SHAPES[name]
        self.b = 2
        g, self.x, wt, self.s_in, self.s_out = heavy_inputs(4000 + list(SHAPES).index(name), self.b, self.k, self.n, self.h, self.w)
        self.pack = K.conv_pack(wt, 1.0, False, False)
        self.kernel = (torch.outer(torch.tensor([1., 3., 3., 1.]), torch.tensor([1., 3., 3., 1.])) / 64 * 4).to(DEV)
        self.noise = torch.randn(1, 1, 2 * self.h, 2 * self.w, generator=g).to(DEV)
        self.nw = torch.full((1,), 0.01, device=DEV)
        _, scale0 = upblur_ref(self.x, wt, self.s_in, self.s_out, self.kernel)
        self.bias = (0.3 * torch.randn(self.n, generator=g).double() * scale0.mean((0, 2, 3))).float().to(DEV)
        self.refs = {True: upblur_ref(self.x, wt, self.s_in, self.s_out, self.kernel, self.noise, self.nw, self.bias),
                     False: (upblur_ref(self.x, wt, self.s_in, self.s_out, self.kernel)[0], scale0)}

    def act(self, with_act):
        return (self.noise, self.nw, self.bias) if with_act else (None, None, None)

    def fused(self, with_act):
        """-> (out, the canary buffer around it)"""
        from where2edit_amd._lib import call, ptr, stream_ptr
        b, k, n, h, w = self.b, self.k, self.n, self.h, self.w
        numel = b * n * 4 * h * w
        buf = torch.full((numel + 2 * TAIL,), CANARY, device=DEV)
        out = buf[TAIL:TAIL + numel].view(b, n, 2 * h, 2 * w)
        noise, nw, bias = self.act(with_act)
        call("w2e_modconv_upblur", ptr(self.x), ptr(self.pack), ptr(self.s_in), ptr(self.s_out), ptr(self.kernel), ptr(out), b, k, n, h, w,
             ptr(noise), ptr(nw), ptr(bias), stream_ptr())
        torch.cuda.synchronize()
        return out, buf

    def pair(self, with_act):
        from where2edit_amd import functional as K
        h, w = self.h, self.w
        t, _ = K._modconv_raw(K.MODE_UP, self.x, self.pack, self.s_in, self.s_out, h, w)
        act = (None,) + self.act(with_act)
        if K.fir_planar_ok(self.kernel.shape, 2 * w):
            return K._upfirdn2d_raw(t, self.kernel, 2 * h, 2 * w, 1, 1, 1, 1, True, act=act, planar_hw=(2 * h + 1, 2 * w + 1))
        return K._upfirdn2d_raw(K.unplanar(t, w), self.kernel, 2 * h, 2 * w, 1, 1, 1, 1, True, act=act)


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Problem(name)
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("with_act", [True, False], ids=["noise_bias", "bare"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_upblur_against_float64_and_the_two_launch_form(name, with_act, problems, w2e_opt, capfd):
    """Global and per-plane error against float64 within FWD_TOL; the fused form's worst plane at most twice the two-launch form's
    on the same inputs; nothing written outside the output; the variant line names a key of the matrix."""
    p = problems(name)
    ref, scale = p.refs[with_act]
    w2e_opt("tune_upblur", 1)
    w2e_opt("tune_print", 1)
    capfd.readouterr()
    out, buf = p.fused(with_act)
    lines = [m for ln in capfd.readouterr().err.splitlines() if (m := UPBLUR_VARIANT.match(ln))]
    w2e_opt("tune_print", 0)
    assert len(lines) == 1, lines
    key = tuple(int(v) for v in lines[0].groups())
    assert key in MATRIX_KEYS and key[4] == int(p.w % 2 == 0), key
    what = f"upblur {name} {'noise+bias' if with_act else 'bare'}"
    assert torch.all(buf[:TAIL] == CANARY) and torch.all(buf[-TAIL:] == CANARY), f"{what}: wrote outside the output"
    y_pair = p.pair(with_act)
    e_pair = assert_close_planes(y_pair, ref, scale, FWD_TOL, what + " (two-launch form)")
    g_fused, g_pair = rel_err(out, ref), rel_err(y_pair, ref)
    e_fused = float("nan")
    try:
        e_fused = assert_close_planes(out, ref, scale, FWD_TOL, what)
    finally:
        print(f"{what}: worst plane error fused {e_fused:.2e}, two-launch {e_pair:.2e}; global fused {g_fused:.2e}, two-launch {g_pair:.2e}")
    assert_close(out, ref, FWD_TOL, what)
    assert e_fused <= 2 * e_pair, f"{what}: worst plane error {e_fused:.3e} > 2 x the two-launch form's {e_pair:.3e}"


@pytest.mark.gpu
def test_forcing_the_form_on_bf16x3_or_split_k_raises(problems, w2e_opt):
    from where2edit_amd import functional as K
    p = problems("one_tile")
    w2e_opt("tune_upblur", 1)
    assert K._upblur_planned(p.b, p.k, p.n, p.h, p.w)
    w2e_opt("conv_precision", "bf16x3")
    assert not K._upblur_planned(p.b, p.k, p.n, p.h, p.w)
    with pytest.raises(RuntimeError, match="bf16x3"):
        p.fused(True)
    w2e_opt("conv_precision", "f32")
    w2e_opt("tune_cfg", "11,2,1")
    assert not K._upblur_planned(p.b, p.k, p.n, p.h, p.w)
    with pytest.raises(RuntimeError, match="split-K"):
        p.fused(True)
    w2e_opt("tune_cfg", "")
    w2e_opt("tune_upblur", 0)
    assert not K._upblur_planned(p.b, p.k, p.n, p.h, p.w)


@pytest.mark.gpu
def test_styled_conv_gradients_fused_forward_against_two_launch_forward(w2e_opt):
    """_StyledConv with the fused forward and with the two-launch forward, both through the unchanged backward: the x, s, noise
    weight and bias gradients agree to the gradient tolerance (a multi-tile shape, ragged in both directions)."""
    from where2edit_amd import functional as K
    b, k, n, h, w = 2, 16, 32, SY + 5, SX + 6
    g = torch.Generator().manual_seed(77)
    wt = torch.randn(n, k, 3, 3, generator=g).to(DEV)
    scale = 1.0 / math.sqrt(k * 9)
    packs = (K.conv_pack(wt, scale, False, False), K.conv_pack(wt, scale, True, False))
    wsq = (wt * scale).square().sum((2, 3)).contiguous()
    kernel = (torch.outer(torch.tensor([1., 3., 3., 1.]), torch.tensor([1., 3., 3., 1.])) / 64 * 4).to(DEV)
    noise = torch.randn(1, 1, 2 * h, 2 * w, generator=g).to(DEV)
    cot = torch.randn(b, n, 2 * h, 2 * w, generator=g).to(DEV)
    x0, s0 = torch.randn(b, k, h, w, generator=g).to(DEV), (torch.rand(b, k, generator=g) + 0.5).to(DEV)

    def run(mode):
        w2e_opt("tune_upblur", mode)
        leaves = [x0.clone().requires_grad_(True), s0.clone().requires_grad_(True), torch.full((1,), 0.3, device=DEV).requires_grad_(True),
                  (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(5))).to(DEV).requires_grad_(True)]
        x, s, nw, bias = leaves
        assert K._upblur_planned(b, k, n, h, w) == bool(mode)
        out = K.styled_conv(x, s, wsq, noise, nw, bias, packs, kernel, True)
        grads = torch.autograd.grad((out * cot).sum(), leaves)
        torch.cuda.synchronize()
        return out.detach(), grads

    out1, g1 = run(1)
    out0, g0 = run(0)
    assert_close(out1, out0, FWD_TOL, "styled conv output, fused against two-launch forward")
    for name, a, c in zip(("x", "s", "noise weight", "bias"), g1, g0):
        print(f"gradient {name}: fused against two-launch forward {rel_err(a, c):.2e}")
        assert_close(a, c, GRAD_TOL, f"gradient w.r.t. {name}, fused against two-launch forward")


UP_LAYERS = [(512, 512, 4), (512, 512, 8), (512, 512, 16), (512, 512, 32), (512, 256, 64), (256, 128, 128), (128, 64, 256), (64, 32, 512)]


@pytest.mark.gpu
def test_census_upblur_variants_of_real_steps_are_in_the_matrix():
    """Eager steps of workload 2 at batch 4 and 8 (library defaults): every "modconv upblur variant" line is a key of MATRIX_KEYS,
    and batch 4 prints at least one if the library's own choice (tune_upblur = -1) takes any FFHQ-1024 up layer."""
    import bench
    from where2edit_amd import functional as K
    from where2edit_amd.profiling import conv_selections
    dev = "cuda:0"
    coach = bench.build_coach(1024, 8, dev, False, "hip", 2)
    seen = {}
    for b in (4, 8):
        w = bench.synthetic_latents(coach.net.decoder, b, 0)
        lines, _ = conv_selections(lambda: coach.train_step(w))
        hits = [m for ln in lines if (m := UPBLUR_VARIANT.match(ln))]
        seen[b] = hits
        for m in hits:
            key = tuple(int(v) for v in m.groups())
            assert key in MATRIX_KEYS, f"`{m.string}` (workload 2 batch {b}) has no case in the matrix of tests/test_gpu_upblur.py: add one"
        print(f"census: workload 2 batch {b}: {len(hits)} upblur launches {sorted({m.string for m in hits})}")
    auto_any = any(K._upblur_planned(2 * 4, cin, cout, r, r) for cin, cout, r in UP_LAYERS)  # (the step runs [w; w_hat] as one pass)
    if auto_any:
        assert seen[4], "the library's own choice takes an up layer at batch 4, but the step printed no upblur variant line"
    del coach
    torch.cuda.empty_cache()
