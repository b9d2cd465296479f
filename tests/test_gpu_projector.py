"""The projector end to end on the seeded size-32 generator with the seeded LPIPS at lpips_size = 16 (a 2x2 loss front): the noise-map
gradient of the fused StyledConv against CPU autograd through oracle/, one whole loss of step 0 against the float64 references
(tests/lpips_ref.py, tests/projector_ref.py), and where2edit_amd.project itself."""
import pytest
import torch

import lpips_ref
import projector_ref as R
import seeded
from helpers import assert_close, assert_grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE, LPIPS_SIZE = 32, 16
U = 2.0 ** -24


@pytest.fixture(scope="module")
def sd():
    return seeded.generator_state_dict(SIZE)


@pytest.fixture(scope="module")
def sd64(sd):
    return {k: v.double() for k, v in sd.items()}


@pytest.fixture(scope="module")
def g_ema(sd):
    from where2edit_amd.stylegan2 import Generator
    g = Generator(SIZE, 512, 8)
    g.load_state_dict(sd, strict=True)
    return g.to(DEV).eval().requires_grad_(False)


@pytest.fixture(scope="module")
def lpips():
    from where2edit_amd.lpips import LPIPS
    return LPIPS().to(DEV)


def _noise_shapes(g):
    return [tuple(n.shape) for n in g.make_noise()]


def _noises(g, batch=1, salt=0):
    return [seeded.tensor(f"projector.noise{i}", (batch,) + s[1:], salt=salt) for i, s in enumerate(_noise_shapes(g))]


def _oracle(sdx, w, noises, r, dtype):
    """(image, gradients of sum(image * r) to [w] + noises) by CPU autograd through oracle.stylegan2, in `dtype`."""
    from oracle import stylegan2 as OG
    wo = w.to(dtype).requires_grad_(True)
    no = [n.to(dtype).requires_grad_(True) for n in noises]
    io, _ = OG.generator_forward(sdx, [wo], size=SIZE, input_is_latent=True, noise=no)
    return io.detach(), torch.autograd.grad((io * r.to(dtype)).sum(), [wo] + no)


def _mode(mode, w2e_opt, monkeypatch):
    from where2edit_amd import functional as K
    if mode == "deterministic":
        w2e_opt("deterministic", "1")
    elif mode == "winograd0":
        monkeypatch.setattr(K, "WINOGRAD", False)


@pytest.mark.parametrize("mode", ["default", "deterministic", "winograd0"])
def test_noise_maps_get_their_gradient(g_ema, sd, sd64, mode, w2e_opt, monkeypatch):
    """One forward + backward with requires_grad on every [1,1,H,W] noise map: every .grad is there and agrees with CPU autograd through
    oracle.stylegan2 on the same state dict (the project's end-to-end gradient bound, helpers.assert_grad_close at 1e-3); and the pass is
    otherwise the one it was -- the image bit for bit, the latent gradient bit for bit where the launches are the same and run in a fixed
    order (deterministic mode), to the end-to-end bound elsewhere (the wide up-sampling layers swap the fused activation-backward + blur
    for the two-kernel form).

    The oracle runs in float64.  A noise-map gradient is, per pixel, a sum over the layer's 512 planes, so ONE LeakyReLU whose
    pre-activation lies within fp32 rounding of 0 -- its slope then flips 0.2 <-> 1 between two fp32 evaluation orders -- moves that
    pixel by about 1/30 of its size: far more visible than in any gradient the suite compared before.  On these inputs (latent salt 3)
    the oracle's OWN fp32 gradient is 2.3e-3 (map 3), 6.0e-3 (map 4) and 1.3e-2 (map 5, one pixel) from its float64 gradient, while the
    HIP gradients are within 4e-6 of float64 on every map (measured on an MI355X; salts 13 and 23 have no such flip and all three agree
    to 3e-6).  The fp32 oracle's own error is printed beside each comparison."""
    _mode(mode, w2e_opt, monkeypatch)
    w = seeded.wplus_latents(1, g_ema.n_latent, salt=3)
    r = seeded.tensor("projector.r", (1, 3, SIZE, SIZE))
    noises = _noises(g_ema)
    wg = w.to(DEV).requires_grad_(True)
    ng = [n.to(DEV).requires_grad_(True) for n in noises]
    img, _ = g_ema([wg], input_is_latent=True, noise=ng)
    (img * r.to(DEV)).sum().backward()
    assert all(n.grad is not None and n.grad.shape == n.shape for n in ng), [n.grad is None for n in ng]
    io, grads = _oracle(sd64, w, noises, r, torch.float64)
    _, grads32 = _oracle(sd, w, noises, r, torch.float32)
    assert_close(img, io, 1e-3, f"image ({mode})")
    assert_grad_close(wg.grad, grads[0], f"projector: latent gradient beside the noise maps ({mode})")
    for i, (n, go, g32) in enumerate(zip(ng, grads[1:], grads32[1:])):
        print(f"noise map {i} ({mode}): the fp32 oracle is {float((g32.double() - go).abs().max() / go.abs().max()):.2e} from its float64")
        assert_grad_close(n.grad, go, f"projector: noise-map gradient {i} {tuple(n.shape[2:])} ({mode})")
    # the same pass with no map requiring a gradient
    w2 = w.to(DEV).requires_grad_(True)
    img2, _ = g_ema([w2], input_is_latent=True, noise=[n.to(DEV) for n in noises])
    (g2,) = torch.autograd.grad((img2 * r.to(DEV)).sum(), w2)
    if mode == "deterministic":
        assert torch.equal(img2, img) and torch.equal(g2, wg.grad)
    else:  # (outside deterministic mode the forward's split-K sums and the backward's dot epilogues join with atomics: no two runs agree bit for bit)
        assert_close(img2, img, 1e-5, f"image with and without noise-map gradients ({mode})")
        assert_grad_close(wg.grad, g2, f"projector: latent gradient with and without noise-map gradients ({mode})")


def test_shared_and_per_sample_maps_under_a_batch_of_two(g_ema, sd64, w2e_opt):
    """Shared [1,1,H,W] maps under a batch of 2 (the fused form sums both samples' planes) against the float64 oracle to the end-to-end
    bound, in deterministic mode so that the result is the same on every run.  Per-sample [2,1,H,W] maps (the unfused composition,
    autograd's own gradient -- nothing of this change computes it): it runs, every gradient is there and finite and points the oracle's
    way (cosine).  Its max-norm is printed, not held: a per-pixel sum over 512 planes shows a single LeakyReLU kink flip (see
    test_noise_maps_get_their_gradient), and the unfused composition's rounding puts several on these inputs: measured on an MI355X,
    default mode 3.0e-3 in one run and under 1e-3 in another on map 5, deterministic mode 1.3e-4 ... 1.9e-3 over the seven maps, cosine
    1.000000 every time (the fused form on the shared maps of the same pass: 2e-7 ... 4e-6)."""
    w2e_opt("deterministic", "1")
    w = seeded.wplus_latents(2, g_ema.n_latent, salt=4)
    r = seeded.tensor("projector.r2", (2, 3, SIZE, SIZE))
    for batch in (1, 2):
        noises = _noises(g_ema, batch, salt=batch)
        wg = w.to(DEV).requires_grad_(True)
        ng = [n.to(DEV).requires_grad_(True) for n in noises]
        img, _ = g_ema([wg], input_is_latent=True, noise=ng)
        (img * r.to(DEV)).sum().backward()
        _, grads = _oracle(sd64, w, noises, r, torch.float64)
        for i, (n, go) in enumerate(zip(ng, grads[1:])):
            assert n.grad is not None and n.grad.shape == n.shape and bool(torch.isfinite(n.grad).all())
            if batch == 1:
                assert_grad_close(n.grad, go, f"projector: shared noise-map gradient {i} under a batch of 2")
            else:
                a, b = n.grad.double().cpu().flatten(), go.flatten()
                print(f"per-sample noise-map gradient {i}: max-norm rel err {float((a - b).abs().max() / b.abs().max()):.2e}")
                assert float(torch.dot(a, b) / (a.norm() * b.norm())) >= 0.9999, i


def test_noise_map_gradients_on_the_wide_layers(monkeypatch):
    """The two branches of _StyledConv.backward that the 32^2 generator does not reach, on the smallest generator that has both (256^2:
    w2e_blur_adjoint_actbwd needs a width of 256, the ToRGB-folded stride-2 launch runs at 128^2 and up), default mode (both refuse the
    deterministic one).  Which launches run is read from the calls: with the maps requiring grad the 256-wide up-sampling layer gives up
    the fused activation-backward + blur (it never writes the pre-blur gradient) and every layer runs w2e_noise_grad, the folded launch
    still feeds the layer below it its pre-activation gradient; without, the fused form runs as before and w2e_noise_grad never.

    What is held.  (1) An identity of the backward itself, free of every LeakyReLU decision: the map's gradient is noise_w * sum_planes
    gpre and the strength's gradient (existing code: the second of the layer's three sums) is sum_planes,p gpre * noise, both from the same
    gpre, so sum_p g_noise[p] noise[p] = noise_w * g_noise_w.  Two fp32 summation orders of planes * pixels terms: held to 1e-3 of
    sum_p |g_noise[p] noise[p]| (chains of a few hundred additions, ~2e-5 of the sum of |terms|, which is about sqrt(planes) times that
    scale); a gradient taken after the blur, a missing plane or the rows of another sample break it outright.  (2) Against the float64
    oracle: the cosine of every map to 0.9999, and the latent gradient (below).  The max-norm of the maps is printed, not held: with up to
    128 * 65536 activations per layer some LeakyReLU pre-activation lies within fp32 rounding of 0 in every pass, its slope flips, and
    the flips of the layers above reach every map below them through the backward.  Measured on an MI355X: maps 0 ... 2 are 3.7e-4 ...
    8.1e-4 from float64 with no pixel beyond 1e-3, map 3 (16^2) 1.8e-3 with 4 of its 256 pixels beyond -- a first version of this test
    allowed each map ten times the flips to be expected in its own layer (2 there) and failed on exactly that: it had left the flips
    handed down from above out of the count."""
    from where2edit_amd import functional as K
    from where2edit_amd.stylegan2 import Generator
    size = 256
    sd = seeded.generator_state_dict(size)
    g = Generator(size, 512, 8)
    g.load_state_dict(sd, strict=True)
    g = g.to(DEV).eval().requires_grad_(False)
    strengths = [m.noise.weight.requires_grad_(True) for m in [g.conv1] + list(g.convs)]  # (for the identity; in the maps' order)
    w = seeded.wplus_latents(1, g.n_latent, salt=3)
    r = seeded.tensor("projector.r256", (1, 3, size, size))
    noises = [seeded.tensor(f"projector.noise{i}", tuple(n.shape)) for i, n in enumerate(g.make_noise())]
    calls = []
    real = K.call
    monkeypatch.setattr(K, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    wg = w.to(DEV).requires_grad_(True)
    ng = [n.to(DEV).requires_grad_(True) for n in noises]
    img, _ = g([wg], input_is_latent=True, noise=ng)
    grads = torch.autograd.grad((img * r.to(DEV)).sum(), [wg] + ng + strengths)
    grads, g_strengths = grads[:1 + len(ng)], grads[1 + len(ng):]
    with_maps, calls[:] = list(calls), []
    w2 = w.to(DEV).requires_grad_(True)
    img2, _ = g([w2], input_is_latent=True, noise=[n.to(DEV) for n in noises])
    (g2,) = torch.autograd.grad((img2 * r.to(DEV)).sum(), w2)
    without = list(calls)
    monkeypatch.undo()
    assert with_maps.count("w2e_noise_grad") == len(noises) == 13 and "w2e_noise_grad" not in without
    assert "w2e_blur_adjoint_actbwd" in without and "w2e_blur_adjoint_actbwd" not in with_maps
    assert "w2e_modconv_down_rgbfold" in with_maps and with_maps.count("w2e_modconv_down_rgbfold") == without.count("w2e_modconv_down_rgbfold")
    for i, (gn, n, nw, gnw) in enumerate(zip(grads[1:], noises, strengths, g_strengths)):
        terms = gn.double().cpu() * n.double()
        lhs, rhs = float(terms.sum()), float(nw.double()) * float(gnw.double())
        print(f"noise map {i} at 256^2: sum g_noise * noise {lhs:.6e}, noise_w * g_noise_w {rhs:.6e}, scale {float(terms.abs().sum()):.3e}")
        assert abs(lhs - rhs) <= 1e-3 * float(terms.abs().sum()), (i, lhs, rhs)
    sd64 = {k: v.double() for k, v in sd.items()}
    wo = w.double().requires_grad_(True)
    no = [n.double().requires_grad_(True) for n in noises]
    from oracle import stylegan2 as OG
    io, _ = OG.generator_forward(sd64, [wo], size=size, input_is_latent=True, noise=no)
    ref = torch.autograd.grad((io * r.double()).sum(), [wo] + no)
    assert_close(img, io.detach(), 1e-3, "image at 256^2")
    for i, (a, b) in enumerate(zip(grads[1:], ref[1:])):
        a, b = a.double().cpu().flatten(), b.flatten()
        off = int(((a - b).abs() > 1e-3 * b.abs().max()).sum())
        cos = torch.dot(a, b) / (a.norm() * b.norm())
        print(f"noise map {i} at 256^2: cosine {float(cos):.7f}, {off} of {a.numel()} pixels beyond 1e-3, "
              f"max-norm {float((a - b).abs().max() / b.abs().max()):.2e}")
        assert float(cos) >= 0.9999, (i, float(cos))
    # the latent gradient: the same flips, spread over 18 x 512 numbers.  Held to the 5e-3 that helpers.KINK_PRONE gives the latent
    # gradients of the generators below 1024^2 for this very reason (its 64^2 entries: 9.2e-4 ... 1.67e-3 measured), with and without the
    # maps' gradients alike; measured here on an MI355X with them: 1.1e-3, cosine 0.9999996.
    assert_grad_close(grads[0], ref[0], "projector: latent gradient beside the noise maps at 256^2", tol=5e-3)
    assert_grad_close(g2, ref[0], "projector: latent gradient without noise-map gradients at 256^2", tol=5e-3)


def _hip_activations(model, x):
    """{conv index: post-ReLU activation} of the HIP forward over the merged batch x (the `route` of lpips_ref.taps)."""
    from where2edit_amd import irse_hip as IR
    from where2edit_amd import vgg16 as V
    plan, acts = model.plan(), {}
    with torch.no_grad():
        h = IR.affine_act(x.contiguous(), plan.a, plan.b)
        for k in range(5):
            outs = V.slice_fwd(plan, k, h)
            acts.update(zip(V.SLICE_CONVS[k], outs))
            h = outs[-1]
    return {i: a.cpu() for i, a in acts.items()}


def test_one_whole_loss_against_float64(g_ema, sd64, lpips, w2e_opt):
    """LPIPS(small, target).sum() + 1e5 L(noises) + 0.7 MSE of step 0, on the GPU pass's own image.  Values: LPIPS to the 1e-4 the LPIPS
    module is held to against float64 (tests/test_gpu_lpips.py), the regulariser and the MSE to the bounds of
    tests/test_gpu_projector_kernels.py (three pyramid levels at most here: 4 * 2 + 4 = 12 roundings of the term scale; small to the
    front's f^2 + 1 = 5 roundings, under 1e-6; the MSE, a mean of squares of differences of small, to 1e-5).  Gradients: float64
    autograd from the image back (LPIPS with the HIP forward's discrete decisions, as test_gpu_lpips compares), then the float64 CPU
    oracle from the image to the latent and the maps, plus the regulariser's float64 gradient: the project's end-to-end gradient
    bound."""
    from oracle import stylegan2 as OG
    import where2edit_amd as W
    w2e_opt("deterministic", "1")
    weight, mse_w = 1e5, 0.7
    w = seeded.wplus_latents(1, g_ema.n_latent, salt=5)
    noises = _noises(g_ema, salt=5)
    target = torch.tanh(seeded.tensor("projector.target", (1, 3, LPIPS_SIZE, LPIPS_SIZE), 0.8))
    wg = w.to(DEV).requires_grad_(True)
    ng = [n.to(DEV).requires_grad_(True) for n in noises]
    tg = target.to(DEV)
    img, _ = g_ema([wg], input_is_latent=True, noise=ng)
    small, mse = W.loss_front(img, tg)
    p = lpips(small, tg).sum()
    reg = W.noise_regularize(ng)
    loss = p + weight * reg + mse_w * mse
    loss.backward()
    # float64 from the GPU's image on
    lp64 = {k: v.detach().cpu().double() for k, v in lpips.state_dict().items()}
    img64 = img.detach().cpu().double().requires_grad_(True)
    small64, mse64 = R.front(img64, target.double(), SIZE // LPIPS_SIZE)
    p64 = lpips_ref.lpips(lp64, small64, target.double())[0].sum()
    n64 = [n.double().requires_grad_(True) for n in noises]
    reg64 = R.noise_regularize(n64)
    assert_close(small, small64.detach(), 1e-6, "small")
    assert_close(p, p64.detach(), 1e-4, "LPIPS term")
    assert_close(mse, mse64.detach(), 1e-5, "MSE term")
    reg_scale = sum(R.noise_regularize_scales(n.double())[0] for n in noises)
    assert abs(float(reg) - float(reg64)) <= 12 * U * float(reg_scale), (float(reg), float(reg64))
    total64 = float(p64) + weight * float(reg64) + mse_w * float(mse64)
    assert abs(float(loss) - total64) <= 1e-4 * float(p64) + weight * 12 * U * float(reg_scale) + 1e-5 * mse_w * float(mse64) + 2 * U * total64
    route = _hip_activations(lpips, torch.cat([small.detach(), tg]))
    routed = lpips_ref.lpips(lp64, small64, target.double(), route=route)[0].sum()
    (g_img64,) = torch.autograd.grad(routed + mse_w * mse64, img64)
    g_reg64 = torch.autograd.grad(weight * reg64, n64)
    wo = w.double().requires_grad_(True)
    no = [n.double().requires_grad_(True) for n in noises]
    io, _ = OG.generator_forward(sd64, [wo], size=SIZE, input_is_latent=True, noise=no)
    grads = torch.autograd.grad(io, [wo] + no, grad_outputs=g_img64)
    assert_grad_close(wg.grad, grads[0], "projector: whole-loss gradient to the latent")
    for i, (n, go, gr) in enumerate(zip(ng, grads[1:], g_reg64)):
        assert_grad_close(n.grad, go + gr, f"projector: whole-loss gradient to noise map {i}")


def _target(g_ema, toward=0.5):
    """G(w*) at the LPIPS size for a known w*: a mapped sample pulled `toward` the mean latent, under seeded noise maps."""
    import where2edit_amd as W
    with torch.no_grad():
        mean, _ = W.latent_statistics(g_ema, 4096, torch.Generator().manual_seed(1))
        wz = g_ema.style(seeded.tensor("projector.z", (1, 512)).to(DEV))
        w_star = mean + toward * (wz - mean)
        img, _ = g_ema([w_star], input_is_latent=True, noise=[n.to(DEV) for n in _noises(g_ema, salt=9)])
        target, _ = W.loss_front(img, torch.zeros(1, 3, LPIPS_SIZE, LPIPS_SIZE, device=DEV))
    return target


def _stock_project(g_ema, target, lpips, steps, lr, seed, mse=0.0, weight=1e5):
    """where2edit_amd.project's loop with the projector's own arithmetic as the literal expressions of projector.py on stock torch ops --
    the regulariser (torch.roll, reshape(...).mean([3, 5])), the normalisation (mean / std), the down-sampling and F.mse_loss --, with
    torch.optim.Adam, and with the maps handed over as [1,H,W] views, which sends every StyledConv through the unfused composition where
    autograd gives the noise gradient.  The random draws are project's, in project's order.  -> (loss history, MSE history, latent)."""
    import where2edit_amd as W
    from where2edit_amd.projector import _randn
    gen = torch.Generator().manual_seed(seed)
    mean, std = W.latent_statistics(g_ema, 10000, gen)
    latent = mean.detach().clone().repeat(target.shape[0], 1).contiguous().requires_grad_(True)
    noises = [_randn(tuple(n.shape), DEV, gen).contiguous().requires_grad_(True) for n in g_ema.make_noise()]
    opt = torch.optim.Adam([latent] + noises, lr=lr)
    f = g_ema.size // target.shape[2]
    losses, mses = [], []
    for i in range(steps):
        t = i / steps
        opt.param_groups[0]["lr"] = R.get_lr(t, lr)
        strength = std * (0.05 * max(0.0, 1.0 - t / 0.75) ** 2)
        img, _ = g_ema([latent + _randn(latent.shape, DEV, gen) * strength], input_is_latent=True, noise=[n[0] for n in noises])
        small, m = R.front(img, target, f)
        loss = lpips(small, target).sum() + weight * R.noise_regularize(noises) + mse * m
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            for n in noises:
                n.copy_(R.noise_normalize(n))
        losses.append(loss.detach())
        mses.append(m.detach())
    return torch.stack(losses), torch.stack(mses), latent.detach()


PROJECT_LR = 0.01


def test_project_descends_and_is_reproducible(g_ema, lpips, w2e_opt):
    """30 steps of the projector's own loss (LPIPS + 1e5 L, mse = 0) from the mean latent towards G(w*): the total loss and the MSE to the
    target end below where they started, every map ends with mean 0 and std 1 (to a few fp32 roundings of a mean over up to 1024
    elements: 1e-6), and two runs from the same seed agree bit for bit in deterministic mode.

    lr = 0.01, not projector.py's 0.1, which is sized for 1000 steps.  Adam moves a coordinate by at most lr per step; w* lies 0.32 (rms
    per coordinate) from the mean latent, so 30 steps at 0.01 can just cover that distance, while at 0.1 they can overshoot it tenfold --
    and do, on the HIP loop and on the stock-op loop alike (test_project_behaves_as_the_stock_op_loop runs both at both rates).  Moving w*
    nearer the mean does not help there: it only lowers the MSE the run starts from.  Measured on an MI355X at lr 0.01: total loss
    36185 -> 10097, MSE 2.05 -> 0.83."""
    import where2edit_amd as W
    w2e_opt("deterministic", "1")
    target = _target(g_ema)
    seen = []
    runs = [W.project(g_ema, target, steps=30, lr=PROJECT_LR, lpips=lpips, lpips_size=LPIPS_SIZE, generator=torch.Generator().manual_seed(5),
                      callback=(lambda i, loss, img: seen.append(i)) if k == 0 else None) for k in range(2)]
    a, b = runs
    assert seen == list(range(30))
    assert a.latent.shape == (1, 512) and a.img.shape == (1, 3, SIZE, SIZE) and a.loss.shape == (30,) and a.mse.shape == (30,)
    assert [tuple(n.shape) for n in a.noises] == _noise_shapes(g_ema)
    print("loss", [round(float(v), 4) for v in a.loss], "\nmse", [round(float(v), 5) for v in a.mse])
    assert bool(torch.isfinite(a.loss).all())
    assert float(a.loss[-1]) < float(a.loss[0])
    assert float(a.mse[-1]) < float(a.mse[0])
    _, mse_end = W.loss_front(a.img, target)
    assert float(mse_end) < float(a.mse[0])
    for n in a.noises:
        d = n.double()
        assert abs(float(d.mean())) < 1e-6 and abs(float(d.std()) - 1) < 1e-6, (tuple(n.shape), float(d.mean()), float(d.std()))
    assert torch.equal(a.latent, b.latent) and torch.equal(a.img, b.img) and torch.equal(a.loss, b.loss)
    assert all(torch.equal(x, y) for x, y in zip(a.noises, b.noises))


@pytest.mark.parametrize("lr", [PROJECT_LR, 0.1])
def test_project_behaves_as_the_stock_op_loop(g_ema, lpips, lr, w2e_opt):
    """The same 30 steps (mse = 0, the same seed, so the same draws) on where2edit_amd.project and on _stock_project.  Step 0 runs at
    learning rate 0 on identical inputs: the two losses there agree to 1e-4 (LPIPS's own bound against float64; the regulariser carries
    the total and is far tighter).  After that two fp32 loops part slowly, so what is held is the behaviour: at lr 0.01 both loops end
    below their start in loss and in MSE; at projector.py's 0.1 -- thirty steps of a rate meant for a thousand -- each loop's MSE moves
    the same way as the other's (both rise, measured on the HIP loop 2.05 -> 14.9, while the total loss, carried by the regulariser,
    falls 36185 -> 592): the overshoot is the algorithm's on these random LPIPS weights, not the kernels'."""
    import where2edit_amd as W
    w2e_opt("deterministic", "1")
    target = _target(g_ema)
    hip = W.project(g_ema, target, steps=30, lr=lr, lpips=lpips, lpips_size=LPIPS_SIZE, generator=torch.Generator().manual_seed(5))
    s_loss, s_mse, s_latent = _stock_project(g_ema, target, lpips, 30, lr, 5)
    print(f"lr {lr}: HIP loss {float(hip.loss[0]):.1f} -> {float(hip.loss[-1]):.1f}, MSE {float(hip.mse[0]):.3f} -> {float(hip.mse[-1]):.3f}; "
          f"stock loss {float(s_loss[0]):.1f} -> {float(s_loss[-1]):.1f}, MSE {float(s_mse[0]):.3f} -> {float(s_mse[-1]):.3f}; "
          f"latents apart {float((hip.latent - s_latent).abs().max()):.3f}")
    assert_close(hip.loss[0], s_loss[0], 1e-4, "loss of step 0, HIP against stock ops")
    assert_close(hip.mse[0], s_mse[0], 1e-4, "MSE of step 0, HIP against stock ops")
    assert float(hip.loss[-1]) < float(hip.loss[0]) and float(s_loss[-1]) < float(s_loss[0])
    assert (float(hip.mse[-1]) < float(hip.mse[0])) == (float(s_mse[-1]) < float(s_mse[0]))
    if lr == PROJECT_LR:
        assert float(hip.mse[-1]) < float(hip.mse[0]) and float(s_mse[-1]) < float(s_mse[0])


def test_project_with_the_mse_term(g_ema, lpips):
    """projector.py's --mse at its default learning rate: 30 steps with mse = 1 lower the total loss and the MSE (measured 36187 -> 592 and
    2.05 -> 0.15)."""
    import where2edit_amd as W
    r = W.project(g_ema, _target(g_ema), steps=30, mse=1.0, lpips=lpips, lpips_size=LPIPS_SIZE, generator=torch.Generator().manual_seed(5))
    assert float(r.loss[-1]) < float(r.loss[0]) and float(r.mse[-1]) < float(r.mse[0])


def test_project_w_plus_latent_init_mse_and_batch_2(g_ema, lpips):
    import where2edit_amd as W
    target = _target(g_ema)
    gen = lambda: torch.Generator().manual_seed(6)  # noqa: E731
    r = W.project(g_ema, target, steps=3, w_plus=True, mse=0.5, lpips=lpips, lpips_size=LPIPS_SIZE, generator=gen(), n_mean_latent=512)
    assert r.latent.shape == (1, g_ema.n_latent, 512) and bool(torch.isfinite(r.loss).all()) and bool(torch.isfinite(r.img).all())
    assert not torch.equal(r.latent[0, 0], r.latent[0, -1])  # the rows are optimised separately
    init = seeded.wplus_latents(1, g_ema.n_latent, salt=7).to(DEV)
    r = W.project(g_ema, target, steps=3, latent_init=init, lpips=lpips, lpips_size=LPIPS_SIZE, generator=gen(), n_mean_latent=512)
    assert r.latent.shape == init.shape and not torch.equal(r.latent, init) and float((r.latent - init).abs().max()) < 1.0
    assert bool(torch.isfinite(r.loss).all())
    r0 = W.project(g_ema, target, steps=0, latent_init=init, lpips=lpips, lpips_size=LPIPS_SIZE, generator=gen(), n_mean_latent=512)
    assert torch.equal(r0.latent, init) and r0.loss.numel() == 0
    # B = 2: per-sample maps, the unfused composition
    r = W.project(g_ema, target.repeat(2, 1, 1, 1), steps=2, lpips=lpips, lpips_size=LPIPS_SIZE, generator=gen(), n_mean_latent=512)
    assert r.latent.shape == (2, 512) and [tuple(n.shape) for n in r.noises] == [(2,) + s[1:] for s in _noise_shapes(g_ema)]
    assert bool(torch.isfinite(r.loss).all()) and bool(torch.isfinite(r.img).all())
    out = W.save_projection(None, r, ["a", "b"])
    assert out["b"]["noise"][0].shape == (1, 1, 4, 4) and out["a"]["latent"].shape == (512,)
    with pytest.raises(ValueError, match="target must be"):
        W.project(g_ema, torch.zeros(1, 3, SIZE, SIZE, device=DEV), steps=1, lpips=lpips, lpips_size=LPIPS_SIZE)
