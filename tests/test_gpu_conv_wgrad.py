"""Decoder fine-tuning on the MI355X: the conv-weight gradient of ModulatedConv2d (w2e_modconv_wgrad + w2e_modconv_wgrad_finish)
against float64 -- kernel level (SAME / UP / centre tap / DOWN / DOWN-CENTRE, ragged channels, guard canaries), module level (the reference's own
gradients in tests/golden/modconv_wgrad.npz), generator level (the oracle's float64 autograd), bit reproducibility, graph
capture with an optimizer step between replays, and the frozen path launching none of it."""
import ctypes

import pytest
import torch

import seeded
from helpers import GRAD_TOL, assert_close, assert_close_planes, assert_grad_close, golden, rel_err
from make_golden import MODCONV_CASES, modconv_inputs
from make_golden_wgrad import STYLED_CASES, styled_inputs
from oracle import stylegan2 as OG

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 1234.5
MEASURED = []  # (case, worst plane error): printed by test_zz_report
KERNEL_TOL = 1e-6  # per (o,i) plane against float64; measured <= 2.9e-7 for K = 16 ... 2 Mi (heavy-tailed inputs)


def _heavy(shape, gen):
    """Heavy-tailed values: a normal times a log-normal spread of magnitudes."""
    return torch.randn(shape, generator=gen) * torch.exp(1.5 * torch.randn(shape, generator=gen))


def _reference_c(mode, g, x, d, s):
    """C [Cout,Cin,taps] in float64 on the device (9 dgemms over the shifted operand).  Modes 3 / 4 (DOWN / DOWN-CENTRE): g on the
    output grid [h,w], x the [2h+1,2w+1] blurred input sampled at (2y + ky, 2x + kx); mode 4 the (1,1) tap only."""
    g, x = g.double(), x.double()
    if d is not None:
        g = g * d.double()[:, :, None, None]
    sx = x * s.double()[:, :, None, None]
    b, cin, h, w = x.shape
    cout = g.shape[1]
    taps = [(1, 1)] if mode in (2, 4) else [(ky, kx) for ky in range(3) for kx in range(3)]
    out = []
    for ky, kx in taps:
        if mode == 1:
            a = g[:, :, ky:ky + 2 * h:2, kx:kx + 2 * w:2]
            bb = sx
        elif mode >= 3:
            a = g
            bb = sx[:, :, ky:ky + 2 * g.shape[2]:2, kx:kx + 2 * g.shape[3]:2]
        else:
            a = g
            bb = torch.nn.functional.pad(sx, (1, 1, 1, 1))[:, :, ky:ky + h, kx:kx + w]
        am = a.permute(1, 0, 2, 3).reshape(cout, -1)
        bm = bb.permute(1, 0, 2, 3).reshape(cin, -1)
        out.append(am @ bm.t())
    return torch.stack(out, 2)


def _raw_wgrad(mode, g, x, d, s, guard=64):
    """The two kernels on guarded buffers: slab and dW each carry `guard` canary floats past their end."""
    from where2edit_amd import _lib
    from where2edit_amd._lib import call, ptr, stream_ptr
    _lib.load()
    b, cin, h, w = x.shape
    if mode >= 3:  # DOWN / DOWN-CENTRE take the size of g; x is [2h+1, 2w+1]
        h, w = g.shape[2], g.shape[3]
    cout = g.shape[1]
    taps = 1 if mode in (2, 4) else 9
    sp = ctypes.c_int(0)
    call("w2e_modconv_wgrad_plan", mode, b, cin, cout, h, w, ctypes.byref(sp))
    n = taps * cout * cin
    slab = torch.full((sp.value * n + guard,), CANARY, device=DEV)
    dw = torch.full((n + guard,), CANARY, device=DEV)
    call("w2e_modconv_wgrad", mode, ptr(g), ptr(x), ptr(d), ptr(s), ptr(slab), b, cin, cout, h, w, sp.value, stream_ptr())
    call("w2e_modconv_wgrad_finish", ptr(slab), sp.value, None, None, None, None, None, None, None, ptr(dw), b, cin, cout, taps, 1.0,
         stream_ptr())
    torch.cuda.synchronize()
    assert torch.all(slab[sp.value * n:] == CANARY), "w2e_modconv_wgrad wrote past its slabs"
    assert torch.all(dw[n:] == CANARY), "w2e_modconv_wgrad_finish wrote past dW"
    # dw is [Cout][Cin][taps]: the layout of C
    return dw[:n].view(cout, cin, taps), sp.value


KERNEL_CASES = [
    # mode, B, cin, cout, h, w
    (0, 1, 3, 12, 4, 4),
    (0, 2, 12, 20, 7, 9),
    (0, 4, 36, 3, 16, 16),
    (0, 8, 20, 36, 5, 33),
    (0, 2, 64, 64, 64, 64),
    (0, 1, 20, 12, 256, 256),
    (1, 1, 12, 3, 4, 4),
    (1, 2, 3, 20, 9, 6),
    (1, 4, 36, 12, 16, 16),
    (1, 8, 20, 36, 8, 8),
    (1, 1, 12, 20, 128, 128),
    (2, 3, 16, 3, 6, 6),
    (2, 2, 36, 20, 33, 17),
    (2, 1, 3, 12, 256, 256),
    # DOWN / DOWN-CENTRE: h, w are the size of g, x is [2h+1, 2w+1]
    (3, 3, 20, 3, 4, 4),
    (3, 2, 12, 20, 5, 33),
    (3, 1, 3, 36, 9, 6),
    (3, 4, 36, 12, 16, 16),
    (4, 3, 3, 12, 7, 9),
    (4, 2, 12, 20, 5, 33),
    (4, 1, 36, 3, 9, 6),
    (4, 4, 20, 36, 16, 16),
]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[f"m{c[0]}_b{c[1]}_{c[2]}x{c[3]}_{c[4]}x{c[5]}" for c in KERNEL_CASES])
def test_wgrad_kernel_against_float64_correlation(case):
    mode, b, cin, cout, h, w = case
    gen = torch.Generator().manual_seed(hash(case) % (2 ** 31))
    gh, gw = (2 * h + 1, 2 * w + 1) if mode == 1 else (h, w)
    xh, xw = (2 * h + 1, 2 * w + 1) if mode >= 3 else (h, w)
    g = _heavy((b, cout, gh, gw), gen).to(DEV)
    x = _heavy((b, cin, xh, xw), gen).to(DEV)
    d = (torch.rand(b, cout, generator=gen) + 0.5).to(DEV)
    s = _heavy((b, cin), gen).to(DEV)
    dw, splits = _raw_wgrad(mode, g, x, d, s)
    ref = _reference_c(mode, g, x, d, s)
    absref = _reference_c(mode, g.abs(), x.abs(), d, s.abs())
    k = b * h * w
    e = assert_close_planes(dw, ref, absref, KERNEL_TOL, f"wgrad {case}")
    MEASURED.append((f"mode {mode} B{b} {cin}->{cout} {h}x{w} (K {k}, {splits} splits)", e))


def test_wgrad_kernel_1024_32ch_batch2():
    gen = torch.Generator().manual_seed(1024)
    b, c, h = 2, 32, 1024
    g = _heavy((b, c, h, h), gen).to(DEV)
    x = _heavy((b, c, h, h), gen).to(DEV)
    d = (torch.rand(b, c, generator=gen) + 0.5).to(DEV)
    s = _heavy((b, c), gen).to(DEV)
    dw, splits = _raw_wgrad(0, g, x, d, s)
    ref = _reference_c(0, g, x, d, s)
    absref = _reference_c(0, g.abs(), x.abs(), d, s.abs())
    e = assert_close_planes(dw, ref, absref, KERNEL_TOL, "wgrad 1024^2")
    MEASURED.append((f"mode 0 B2 32->32 1024x1024 (K {b * h * h}, {splits} splits)", e))


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
def test_wgrad_is_bit_reproducible(det, w2e_opt):
    from where2edit_amd import functional as K
    w2e_opt("deterministic", "1" if det else "0")
    gen = torch.Generator().manual_seed(5)
    b, cin, cout, h = 4, 64, 32, 128
    gpre, x = _heavy((b, cout, h, h), gen).to(DEV), _heavy((b, cin, h, h), gen).to(DEV)
    s, d = _heavy((b, cin), gen).to(DEV), (torch.rand(b, cout, generator=gen) + 0.5).to(DEV)
    dz = torch.randn(b, cout, generator=gen).to(DEV)
    weight = torch.randn(1, cout, cin, 3, 3, generator=gen).to(DEV)
    runs = [K.modconv_wgrad(K.WGRAD_SAME, gpre, x, d, s, weight, 0.1, dz=dz) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------ module level
def _modconv_module(name, cin, cout, k, demod, up, i):
    from where2edit_amd.stylegan2 import ModulatedConv2d, train_conv_weights
    m = ModulatedConv2d(cin, cout, k, 512, demodulate=demod, upsample=up)
    sd = {"weight": i["weight"], "modulation.weight": i["mod_w"], "modulation.bias": i["mod_b"]}
    if up:
        sd["blur.kernel"] = seeded.fir_kernel(gain=4.0)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.requires_grad_(False)
    return train_conv_weights(m)


@pytest.mark.parametrize("case", MODCONV_CASES, ids=[c[0] for c in MODCONV_CASES])
def test_modulated_conv2d_weight_gradient_matches_the_reference(case):
    name, cin, cout, k, demod, up, b, h = case
    g = golden("modconv_wgrad")
    i = modconv_inputs(name, cin, cout, k, b, h)
    m = _modconv_module(name, cin, cout, k, demod, up, i)
    x, w = i["x"].to(DEV).requires_grad_(True), i["w"].to(DEV).requires_grad_(True)
    y, _ = m(x, w)
    gy = seeded.tensor(f"modconv.{name}.gy", y.shape).to(DEV)
    gx, gw, gweight = torch.autograd.grad(y, (x, w, m.weight), gy)
    assert gweight.shape == m.weight.shape
    assert_close(gweight, g[f"{name}.gweight"], 1e-4, f"{name} gweight")
    assert_close(gx, g[f"{name}.gx"], 1e-4, f"{name} gx")
    assert_close(gw, g[f"{name}.gw"], 1e-4, f"{name} gw")


@pytest.mark.parametrize("case", STYLED_CASES, ids=[c[0] for c in STYLED_CASES])
def test_styled_conv_weight_gradient_matches_the_reference(case):
    from where2edit_amd.stylegan2 import StyledConv, train_conv_weights
    name, cin, cout, up, b, h = case
    g = golden("modconv_wgrad")
    i = styled_inputs(name, cin, cout, b, h, up)
    m = StyledConv(cin, cout, 3, 512, upsample=up)
    sd = {"conv.weight": i["weight"], "conv.modulation.weight": i["mod_w"], "conv.modulation.bias": i["mod_b"],
          "noise.weight": i["noise_w"], "activate.bias": i["bias"]}
    if up:
        sd["conv.blur.kernel"] = seeded.fir_kernel(gain=4.0)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    train_conv_weights(m)
    x, w = i["x"].to(DEV).requires_grad_(True), i["w"].to(DEV).requires_grad_(True)
    y, _ = m(x, w, noise=i["noise"].to(DEV))
    assert m._act_noise is not None or up  # the fused epilogue ran
    gy = seeded.tensor(f"wgrad.{name}.gy", y.shape).to(DEV)
    grads = torch.autograd.grad(y, (x, w, m.conv.weight, m.noise.weight, m.activate.bias), gy)
    assert_close(y, g[f"{name}.y"], 1e-4, f"{name} y")
    for got, key in zip(grads, ("gx", "gw", "gweight", "g_noise", "g_bias")):
        assert_close(got, g[f"{name}.{key}"], 1e-4, f"{name} {key}")


# ------------------------------------------------------------------------------------------ generator level
def _generator(size, sd):
    from where2edit_amd.stylegan2 import Generator, train_conv_weights
    g = Generator(size, 512, 8)
    g.load_state_dict(sd, strict=True)
    g = g.to(DEV).eval()
    return train_conv_weights(g)


def _conv_params(g):
    from where2edit_amd.stylegan2 import ModulatedConv2d
    return [(n, m.weight) for n, m in g.named_modules() if isinstance(m, ModulatedConv2d)]


def _oracle_grads(sd, w, r, size, keys, dtype):
    s = {k: v.to(dtype).requires_grad_(k in keys) for k, v in sd.items()}
    wo = w.to(dtype).requires_grad_(True)
    io, _ = OG.generator_forward(s, [wo], size=size, input_is_latent=True, randomize_noise=False)
    return torch.autograd.grad((io * r.to(dtype)).sum(), [wo] + [s[k] for k in keys])


@pytest.mark.parametrize("size,b", [(256, 2), (1024, 1)])
def test_generator_gradients_match_the_float64_oracle(size, b, w2e_opt):
    """Generator(size), every conv weight trained (Winograd forms on their default selection), against the oracle's float64 autograd:
    the W+ gradient, every conv-weight gradient and the noise-strength / activation-bias gradients, at cosine >= 0.99999 and a max-norm
    error of GRAD_TOL or -- where the oracle's OWN fp32 autograd (the reference's arithmetic on stock ops) lands further than that from
    float64 on some gradient of this generator -- twice that distance.  LeakyReLU kinks (a pre-activation within rounding of 0 flips
    its slope 0.2 <-> 1) put the fp32 oracle's conv-weight gradients up to 2.4e-3 from float64 at 256^2 (measured); the HIP path
    measured up to 2e-3 in the default mode, and once 3.9e-3 (a kink flipped by the forward's split-K atomics), so the test runs in
    the deterministic mode (one fixed evaluation order) and allows twice the oracle's own fp32 distance."""
    w2e_opt("deterministic", "1")
    sd = seeded.generator_state_dict(size)
    g = _generator(size, sd)
    w = seeded.wplus_latents(b, g.n_latent, salt=41)
    r = seeded.tensor(f"wgrad.gen{size}.r", (b, 3, size, size))
    wg = w.to(DEV).requires_grad_(True)
    img, _ = g([wg], input_is_latent=True, randomize_noise=False)
    convs = _conv_params(g)
    # (noise strengths / biases at 256^2 only: at 1024^2 a noise-strength gradient is a sum over 2^20 pixels that cancels to a few
    # per cent of its terms, so its max-norm error measures that cancellation, not this feature -- 3e-2 measured)
    others = [(n, p) for n, p in g.named_parameters() if n.endswith(("noise.weight", "activate.bias"))] if size <= 256 else []
    grads = torch.autograd.grad((img * r.to(DEV)).sum(), [wg] + [p for _, p in convs] + [p for _, p in others])
    keys = [n + ".weight" for n, _ in convs] + [n for n, _ in others]
    ref = _oracle_grads(sd, w, r, size, keys, torch.float64)
    f32 = _oracle_grads(sd, w, r, size, keys, torch.float32)
    tol = max(GRAD_TOL, 2.0 * max(rel_err(own, want) for own, want in zip(f32, ref)))
    for got, want, k in zip(grads, ref, ["grad_w"] + keys):
        assert got.shape == want.shape, k
        assert_grad_close(got, want, f"generator {size} {k}", tol=tol, cos_min=0.99999)


def test_nograd_prefix_rows_do_not_change_the_weight_gradient(w2e_opt):
    """The merged [w; w_hat] pass (functional.nograd_prefix): whatever the prefix rows hold, the conv-weight gradients are the same
    bits (deterministic mode: the per-sample forward is then bit-reproducible, so no LeakyReLU kink can flip between the runs)."""
    from where2edit_amd import functional as K
    w2e_opt("deterministic", "1")
    size, n = 64, 2
    g = _generator(size, seeded.generator_state_dict(size))
    w1 = seeded.wplus_latents(n, g.n_latent, salt=52).to(DEV)
    r = seeded.tensor("wgrad.prefix.r", (n, 3, size, size)).to(DEV)
    convs = [p for _, p in _conv_params(g)]
    runs = []
    for salt in (51, 53):
        w0 = seeded.wplus_latents(n, g.n_latent, salt=salt).to(DEV)
        with K.nograd_prefix(n):
            both, _ = g([torch.cat([w0, w1])], input_is_latent=True, randomize_noise=False)
        runs.append(torch.autograd.grad((K.tail_rows(both, n) * r).sum(), convs))
    img, _ = g([w1], input_is_latent=True, randomize_noise=False)
    alone = torch.autograd.grad((img * r).sum(), convs)
    for a, b, c in zip(*runs, alone):
        assert torch.equal(a, b)
        assert torch.allclose(a, c, rtol=0, atol=5e-3 * c.abs().max().item())  # (batch 4 vs 2: other tiles, other rounding)


def test_generator_weight_gradient_bit_reproducible_in_deterministic_mode(w2e_opt):
    w2e_opt("deterministic", "1")
    size = 64
    g = _generator(size, seeded.generator_state_dict(size))
    w = seeded.wplus_latents(2, g.n_latent, salt=61).to(DEV)
    r = seeded.tensor("wgrad.det.r", (2, 3, size, size)).to(DEV)
    convs = [p for _, p in _conv_params(g)]
    runs = []
    for _ in range(2):
        img, _ = g([w], input_is_latent=True, randomize_noise=False)
        runs.append(torch.autograd.grad((img * r).sum(), convs))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_captured_fine_tuning_step_replays_with_the_live_weights(w2e_opt):
    """Generator forward + the CLIP preprocessing + backward into the trained conv weights, captured through coach.capture_graph
    (memset_guard included), with an eager Adam step between replays: two replays equal two eager steps.  (Deterministic mode: in
    the default mode the forward's split-K atomics may flip a LeakyReLU kink between any two runs.)"""
    from where2edit_amd import coach
    from where2edit_amd import functional as K
    w2e_opt("deterministic", "1")
    size, b = 64, 2
    sd = seeded.generator_state_dict(size)
    w = seeded.wplus_latents(b, 10, salt=71).to(DEV)
    gclip = seeded.tensor("wgrad.capture.gclip", (b, 3, 224, 224)).to(DEV)

    def make():
        g = _generator(size, sd)
        g.requires_grad_(False)
        from where2edit_amd.stylegan2 import train_conv_weights
        train_conv_weights(g)
        params = [p for _, p in _conv_params(g)]
        return g, params, torch.optim.Adam(params, lr=1e-2)

    def body_of(g, params):
        def body():
            for p in params:
                p.grad = None
            img, _ = g([w], input_is_latent=True, randomize_noise=False)
            K.clip_preprocess(img).backward(gclip)
            return img
        return body

    g_e, p_e, opt_e = make()
    eager_grads = []
    body_e = body_of(g_e, p_e)
    for _ in range(2):
        body_e()
        eager_grads.append([p.grad.clone() for p in p_e])
        opt_e.step()
    torch.cuda.synchronize()

    g_c, p_c, opt_c = make()
    graph, _ = coach.capture_graph(body_of(g_c, p_c), "fine-tuning step", torch.device(DEV), leaves=p_c)
    static = [p.grad for p in p_c]
    for step in range(2):
        graph.replay()
        for p, gr in zip(p_c, static):
            p.grad = gr
        torch.cuda.synchronize()
        for a, e in zip(static, eager_grads[step]):
            assert_close(a, e, 1e-6, f"replay {step} dW")
        opt_c.step()
    for a, e in zip(p_c, p_e):
        assert_close(a.detach(), e.detach(), 1e-6, "weights after two steps")


def test_frozen_decoder_backward_launches_no_wgrad_kernel():
    from where2edit_amd.stylegan2 import Generator, freeze_conv_weights
    size = 64
    g = Generator(size, 512, 8)
    g.load_state_dict(seeded.generator_state_dict(size), strict=True)
    g = freeze_conv_weights(g.to(DEV))
    w = seeded.wplus_latents(2, g.n_latent, salt=81).to(DEV).requires_grad_(True)
    for _ in range(2):  # (the second pass is the cached, steady-state one)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            img, _ = g([w], input_is_latent=True, randomize_noise=False)
            img.backward(torch.ones_like(img))
            torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    assert any("modconv" in n for n in names)  # (the profile saw the conv kernels)
    assert not any("wgrad" in n or "wsq" in n for n in names), sorted(n for n in names if "wgrad" in n or "wsq" in n)


def test_zz_report():
    for what, e in MEASURED:
        print(f"wgrad kernel plane error {e:.3e}  {what}")
