"""The stride-2 input-gradient conv with the ToRGB backward in its dot epilogue (w2e_modconv_down_rgbfold,
modconv_kernel<CONV_DOWN, EPI_DOT_RGB, ...>) against float64 (tests/rgbfold_ref.py), forced over every DOWN tile the epilogue is
instantiated for; through the generator's autograd path (functional.RgbFoldLink) against the float64 oracle with the fold on and
off; and the refusals: a tile that does not fit, the modes the form does not support, a tensor hook on the passed-through
activation.

Inputs are heavy-tailed as in tests/test_gpu_conv_variants.py (log-normal channel scales with x30 outliers, per-sample scales
10x apart); x, the activation whose sign selects the LeakyReLU slope, has both signs in every plane."""
import re

import pytest
import torch

from helpers import KINK_PRONE, GRAD_TOL, assert_close, assert_close_planes, assert_grad_close
from rgbfold_ref import rgbfold_ref
from test_gpu_conv_variants import DOT_TOL, DOWN_TILES, FWD_TOL, MODE_LINE, VARIANT, heavy_inputs

DEV = "cuda"
# (b, k, n, h, w): odd plane size, K and N multiples of no tile, ragged tile borders / whole tiles, 16-byte aligned rows
SHAPES = {"ragged": (2, 37, 70, 11, 21), "vector": (3, 16, 64, 16, 32)}
PREFIX = {"ragged": 0, "vector": 1}  # rows of a no-grad prefix in front of the batch: the launch works on the tail of every tensor
DMA_TILES = (0, 9, 10)  # tiles whose epilogue also exists on the LDS-DMA pipeline
NO_FIT_TILES = (1, 2, 8)  # DOWN never takes them (more patch elements per thread than its prefetch registers hold)
RGBFOLD_VARIANT = re.compile(r"modconv rgbfold variant cfg (\d+) dma (\d) styled (\d) noise (\d) ")
CANARY, TAIL = 1234.5, 4096


class Problem:
    """One shape: inputs, and the float64 reference of each (styled, with_noise) form, computed once."""

    def __init__(self, name):
        from where2edit_amd import functional as K
        self.name = name
        b, k, n, h, w = self.shape = SHAPES[name]
        self.pre = PREFIX[name]
        full = b + self.pre
        gen, g, wt, s_in, s_out = heavy_inputs(7000 + list(SHAPES).index(name), full, k, n, 2 * h + 1, 2 * w + 1)
        self.g, self.s_in, self.s_out, self.wt = g, s_in, s_out, wt
        self.pack = K.conv_pack(wt, 1.0, False, False)
        cs = torch.exp(1.5 * torch.randn(n, generator=gen))
        self.x = (torch.randn(full, n, h, w, generator=gen) * cs[None, :, None, None]).to(DEV)
        assert bool(((self.x > 0).flatten(2).any(2) & (self.x < 0).flatten(2).any(2)).all())
        self.gy = (torch.randn(full, 3, h, w, generator=gen) * torch.exp(torch.randn(3, generator=gen))[None, :, None, None]).to(DEV)
        self.noise = torch.randn(1, 1, h, w, generator=gen).to(DEV)
        self.wsc = torch.randn(3, n, generator=gen).to(DEV)
        self.style = ((torch.rand(full, n, generator=gen) + 0.5) * torch.tensor([(1.0, 12.0, 0.08)[i % 3] for i in range(full)])[:, None]).to(DEV)
        self.wmod = (self.wsc[None] * self.style[:, None, :]).contiguous()
        self._refs = {}

    def tail(self, t):
        return t[self.pre:]

    def rgb(self, styled):
        return (self.wsc, self.tail(self.style)) if styled else (self.tail(self.wmod), None)

    def ref(self, styled, with_noise):
        key = (styled, with_noise)
        if key not in self._refs:
            wrgb, style = self.rgb(styled)
            self._refs[key] = rgbfold_ref(self.tail(self.g), self.wt, self.tail(self.s_in), self.tail(self.s_out), self.tail(self.x),
                                          self.tail(self.gy), wrgb, style, self.noise if with_noise else None)
        return self._refs[key]

    def run(self, styled, with_noise):
        """One launch on the tails, gpre written into the tail of a canary-filled full-batch buffer -> (gpre, dot, sums3, gw, buffer)."""
        from where2edit_amd import functional as K
        b, k, n, h, w = self.shape
        full = b + self.pre
        buf = torch.full((full * n * h * w + TAIL,), CANARY, device=DEV)
        out = buf[:full * n * h * w].view(full, n, h, w)
        wrgb, style = self.rgb(styled)
        gpre, dot, sums3, gw = K._modconv_down_rgbfold_raw(self.tail(self.g), self.pack, self.tail(self.s_in), self.tail(self.s_out), h, w,
                                                           self.tail(self.x), self.tail(self.gy), wrgb, style,
                                                           self.noise if with_noise else None, out=self.tail(out))
        torch.cuda.synchronize()
        return gpre, dot, sums3, gw, buf


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Problem(name)
        return cache[name]
    return get


def check(p, res, ref, what):
    """gpre per plane and under the max-norm; every sum vector under the max-norm (DOT_TOL) and per channel against its sum of
    |terms| (FWD_TOL); nothing written outside the tail rows of the output.  Returns the worst relative errors."""
    gpre, dot, sums3, gw, buf = res
    b, k, n, h, w = p.shape
    numel = (b + p.pre) * n * h * w
    assert torch.all(buf[numel:] == CANARY), f"{what}: wrote past the end of the output"
    assert torch.all(buf[:p.pre * n * h * w] == CANARY), f"{what}: wrote into the no-grad prefix rows"
    worst = {}
    r, a = ref["gpre"]
    assert_close(gpre, r, FWD_TOL, f"{what} gpre")
    worst["gpre"] = assert_close_planes(gpre, r, a, FWD_TOL, f"{what} gpre per plane")
    vecs = {"dot": dot, "sums3 pre": sums3[..., 0], "sums3 noise": sums3[..., 1], "sums3 sum": sums3[..., 2], "gw": gw}
    refs = {"dot": ref["dot"], "sums3 pre": tuple(t[..., 0] for t in ref["sums3"]), "sums3 noise": tuple(t[..., 1] for t in ref["sums3"]),
            "sums3 sum": tuple(t[..., 2] for t in ref["sums3"]), "gw": ref["gw"]}
    for key, got in vecs.items():
        r, a = refs[key]
        if float(r.abs().max()) == 0.0:  # (no noise: the noise sum is exactly 0)
            assert float(got.abs().max()) == 0.0, f"{what} {key}: must be 0"
            continue
        assert_close(got, r, DOT_TOL, f"{what} {key}")
        worst[key] = assert_close_planes(got.reshape(-1, 1, 1, 1), r.reshape(-1, 1, 1, 1), a.reshape(-1, 1, 1, 1), FWD_TOL,
                                         f"{what} {key} against its sum of |terms|")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "no_noise"])
@pytest.mark.parametrize("styled", [True, False], ids=["styled", "plain"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_rgbfold_tiles_against_float64(name, styled, with_noise, problems, w2e_opt, capfd):
    """Every DOWN tile (register pipeline; tiles 0 / 9 / 10 also asked for on the LDS-DMA pipeline) forced through tune_cfg: the plan
    accepts it and the launch matches float64, or -- a tile that does not fit the shape -- the plan refuses it and the launch raises."""
    from where2edit_amd import functional as K
    p = problems(name)
    b, k, n, h, w = p.shape
    ref = p.ref(styled, with_noise)
    w2e_opt("tune_rgbfold", 1)
    w2e_opt("tune_print", 1)
    ran, worst_all = set(), {}
    for cfg, dma in [(c, 0) for c in DOWN_TILES + NO_FIT_TILES] + [(c, 1) for c in DMA_TILES]:
        what = f"{name} cfg {cfg} dma {dma} {'styled' if styled else 'plain'} {'noise' if with_noise else 'no noise'}"
        w2e_opt("tune_cfg", f"{cfg},1,2")
        w2e_opt("tune_dma", dma)
        capfd.readouterr()
        if not K._rgbfold_planned(b, k, n, h, w):
            with pytest.raises(RuntimeError):
                p.run(styled, with_noise)
            assert not RGBFOLD_VARIANT.search(capfd.readouterr().err), f"{what}: refused by the plan, but a launch ran"
            continue
        assert cfg not in NO_FIT_TILES, f"{what}: the plan accepted a tile DOWN cannot stage"
        res = p.run(styled, with_noise)
        err = capfd.readouterr().err.splitlines()
        lines = [m for ln in err if (m := RGBFOLD_VARIANT.match(ln))]
        assert len(lines) == 1 and int(lines[0][1]) == cfg, f"{what}: variant lines {[m.string for m in lines]}"
        assert (int(lines[0][3]), int(lines[0][4])) == (int(styled), int(with_noise)), lines[0].string
        assert sum(bool(MODE_LINE.match(ln)) for ln in err) == 1 and not any(VARIANT.match(ln) for ln in err), err
        got_dma = int(lines[0][2])
        assert got_dma <= dma, what
        for key, e in check(p, res, ref, what).items():
            worst_all[key] = max(worst_all.get(key, 0.0), e)
        ran.add((cfg, got_dma))
    print(f"rgbfold {name} {'styled' if styled else 'plain'} {'noise' if with_noise else 'no noise'}: ran {sorted(ran)}; worst "
          + ", ".join(f"{k2} {v:.2e}" for k2, v in worst_all.items()))
    assert {c for c, d in ran if d == 0} == set(DOWN_TILES), f"every DOWN tile fits these shapes on the register pipeline: {sorted(ran)}"
    assert (9, 1) in ran, f"tile 9 did not run on the LDS-DMA pipeline: {sorted(ran)}"


@pytest.mark.gpu
def test_rgbfold_equals_the_two_kernel_path(problems, w2e_opt):
    """The library's own tile for the shape: the folded launch against the pair it replaces (DOWN conv with the dot epilogue, then
    w2e_torgb_bwd_actbwd), each within the float64 tolerance, so within twice that of each other."""
    from where2edit_amd import functional as K
    from where2edit_amd._lib import call, ptr, stream_ptr
    p = problems("vector")
    b, k, n, h, w = p.shape
    w2e_opt("tune_rgbfold", 1)
    assert K._rgbfold_planned(b, k, n, h, w)
    gpre, dot, sums3, gw, _ = p.run(True, True)
    gx, dot2 = K._modconv_raw(K.MODE_DOWN, p.tail(p.g), p.pack, p.tail(p.s_in), p.tail(p.s_out), h, w, dot_with=p.tail(p.x))
    gpre2, gw2, sums2 = torch.empty_like(gx), torch.zeros(b, n, device=DEV), torch.empty(b, n, 3, device=DEV)
    call("w2e_torgb_bwd_actbwd", ptr(p.tail(p.x)), ptr(p.wsc), ptr(p.tail(p.style)), ptr(p.tail(p.gy)), ptr(gx), ptr(p.noise), ptr(gpre2),
         ptr(gw2), ptr(sums2), b, n, h, w, 0.2, 2 ** 0.5, stream_ptr())
    torch.cuda.synchronize()
    ref = p.ref(True, True)
    assert_close_planes(gpre2, ref["gpre"][0], ref["gpre"][1], FWD_TOL, "two-kernel gpre per plane")
    assert_close(gpre, gpre2, 2 * FWD_TOL, "gpre")
    assert_close(dot, dot2, 2 * DOT_TOL, "dot")
    assert_close(sums3, sums2, 2 * DOT_TOL, "sums3")
    assert_close(gw, gw2, 2 * DOT_TOL, "gw")


@pytest.mark.gpu
def test_rgbfold_plan_refuses_what_the_form_does_not_support(problems, w2e_opt):
    from where2edit_amd import functional as K
    b, k, n, h, w = SHAPES["vector"]  # (K = 16: the library's own choice does not split it)
    for mode, want in ((1, True), (0, False)):
        w2e_opt("tune_rgbfold", mode)
        assert K._rgbfold_planned(b, k, n, h, w) == want, mode
    p = problems("ragged")
    b, k, n, h, w = p.shape
    w2e_opt("tune_rgbfold", 1)
    w2e_opt("tune_cfg", "9,3,2")  # a split-K launch (K = 37: 16 + 16 + 5)
    assert not K._rgbfold_planned(b, k, n, h, w)
    with pytest.raises(RuntimeError, match="split-K"):
        p.run(True, True)
    w2e_opt("tune_cfg", "")
    w2e_opt("deterministic", "1")
    assert not K._rgbfold_planned(b, k, n, h, w)
    with pytest.raises(RuntimeError, match="deterministic"):
        p.run(True, True)
    w2e_opt("deterministic", "0")
    w2e_opt("conv_precision", "bf16x3")
    assert not K._rgbfold_planned(b, k, n, h, w)
    w2e_opt("conv_precision", "f32")
    w2e_opt("tune_cfg", "9,1,2")
    assert K._rgbfold_planned(b, k, n, h, w)


# ---- through autograd: the 64^2 generator -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen64():
    """The seeded 64^2 generator, W+ latents, a cotangent, and the float64 oracle's gradient with respect to the latents."""
    import seeded
    from oracle import stylegan2 as OG
    from where2edit_amd.stylegan2 import Generator, freeze_conv_weights
    size = 64
    sd = seeded.generator_state_dict(size)
    g = Generator(size, 512, 8)
    g.load_state_dict(sd, strict=True)
    g = freeze_conv_weights(g.to(DEV).eval())
    w = seeded.wplus_latents(3, g.n_latent, salt=3)
    r = seeded.tensor("g64.r", (3, 3, size, size))
    sd64 = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}
    wo = w.double().requires_grad_(True)
    io, _ = OG.generator_forward(sd64, [wo], size=size, input_is_latent=True, randomize_noise=False)
    (go,) = torch.autograd.grad((io * r.double()).sum(), wo)
    return g, w, r, go


def _grad_w(g, w, r, prefix):
    from where2edit_amd import functional as K
    wg = w.to(DEV).requires_grad_(True)
    if prefix:  # the merged pass of the training step: [no-grad rows; rows with gradient]
        with K.nograd_prefix(prefix):
            both, _ = g([torch.cat([w[:prefix].to(DEV), wg])], input_is_latent=True, randomize_noise=False)
        img = K.tail_rows(both, prefix)
    else:
        img, _ = g([wg], input_is_latent=True, randomize_noise=False)
    (gw,) = torch.autograd.grad((img * r.to(DEV)).sum(), wg)
    torch.cuda.synchronize()
    return gw


@pytest.mark.gpu
@pytest.mark.parametrize("prefix", [0, 1])
def test_generator64_latent_gradient_with_and_without_the_fold(prefix, gen64, w2e_opt, capfd):
    """The gradient the mapper receives (d loss / d W+) through the same forward with tune_rgbfold = 1 and = 0, each against the
    float64 oracle under the tolerance tests/test_gpu_parity.py holds that gradient to.  The DOWN launches are forced to one unsplit
    tile (5) in both runs: at these sizes the library's own choice splits K, which keeps the two-kernel path."""
    g, w, r, go = gen64
    tol = KINK_PRONE.get("grad_w at 64^2", GRAD_TOL)
    w2e_opt("tune_cfg", "5,1,2")
    w2e_opt("tune_print", 1)
    folds = {}
    for mode in (1, 0):
        w2e_opt("tune_rgbfold", mode)
        capfd.readouterr()
        gw = _grad_w(g, w, r, prefix)
        folds[mode] = sum(bool(RGBFOLD_VARIANT.match(ln)) for ln in capfd.readouterr().err.splitlines())
        assert_grad_close(gw, go, f"grad_w at 64^2, tune_rgbfold {mode}, prefix {prefix}", tol=tol)
    assert folds[0] == 0 and folds[1] == 4, folds  # the levels 4^2 .. 32^2: every ToRGB node with a DOWN conv above it


@pytest.mark.gpu
def test_hook_on_the_passed_through_activation_raises(gen64, w2e_opt, monkeypatch):
    """A tensor hook that replaces the gradient of the activation a ToRGB node passes through: the folded value cannot be un-folded,
    so the ToRGB backward raises instead of handing a wrong gradient on.  Without the fold the same hook is harmless."""
    from where2edit_amd import functional as K
    g, w, r, go = gen64
    real = K.to_rgb

    def hooked(*args, **kwargs):
        out = real(*args, **kwargs)
        if isinstance(out, tuple) and out[1].shape[-1] == 16:
            out[1].register_hook(lambda grad: grad.clone())
        return out

    monkeypatch.setattr(K, "to_rgb", hooked)
    w2e_opt("tune_cfg", "5,1,2")
    w2e_opt("tune_rgbfold", 1)
    with pytest.raises(RuntimeError, match="RgbFoldLink"):
        _grad_w(g, w, r, 0)
    torch.cuda.synchronize()
    w2e_opt("tune_rgbfold", 0)
    assert_grad_close(_grad_w(g, w, r, 0), go, "grad_w at 64^2, hooked activation, tune_rgbfold 0", tol=KINK_PRONE.get("grad_w at 64^2", GRAD_TOL))
