"""LPIPS-VGG v0.1 on the HIP kernels (where2edit_amd.lpips, csrc/lpips.hip): the head's forward and backward alone against float64
of the same fp32 inputs, the module against the float64 restatement (tests/lpips_ref.py, checked on the host by
test_lpips_ref_host.py), one hipGraph capture of forward + backward, and evaluation.lpips_distance."""
import pytest
import torch

import lpips_ref as R
import seeded
from helpers import assert_close, assert_grad_close, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (C, h, w).  The first seven are the taps' shapes at small inputs; the rest walk the kernel's other paths: 16 pixel lanes with float4
# groups (64 <= pixels / 4 < 4096), 64 lanes with float4 groups and with single pixels (odd pixel count), and more tiles than the
# 1024 workgroups per image of either kernel (they then stride over their tiles).
HEAD_SHAPES = [(64, 1, 1), (64, 3, 5), (128, 17, 23), (256, 8, 8), (512, 2, 2), (512, 14, 14), (512, 1, 1),
               (64, 16, 16), (64, 128, 128), (16, 65, 65), (16, 520, 512)]
LARGE = [(64, 128, 128), (16, 520, 512)]  # batch 1 only in the tests that walk many variants: their float64 side is the cost
HEAD_TOL = 1e-5


def _pair(shape, batch, batch1, scale=1.0, near=False):
    """Post-ReLU noise, as a tap is.  The 16-channel shapes draw it around +1 (16% zeros instead of half): with so few channels plain
    noise leaves pixels with ONE live channel, where the masked gradient is 0 in exact arithmetic and, in any fp32 evaluation, a few
    ulp of two cancelling terms that grow like 1 / n -- at 520 x 512 the largest such residue decides the max-norm error (measured:
    the kernel 1.3e-5, the closed form in fp32 on the CPU 2.6e-6, at 2 and 4 channels the CPU's own 2e-4).  No tap has under 64."""
    c, h, w = shape
    mean = 1.0 if c < 64 else 0.0
    f0 = torch.relu(seeded.tensor(f"lp.f0{shape}{batch}", (batch, c, h, w), mean=mean)) * scale
    if near:
        f1 = torch.relu(f0[:batch1] + 0.01 * scale * seeded.tensor(f"lp.noise{shape}{batch}", (batch1, c, h, w)))
    else:
        f1 = torch.relu(seeded.tensor(f"lp.f1{shape}{batch}", (batch1, c, h, w), mean=mean)) * scale
    lin = seeded.tensor(f"lp.lin{shape}", (c,)).abs() / c
    return f0, f1, lin


def _plant_zero_pixels(f0, f1):
    """All-zero feature vectors in f0 only, in f1 only and in both (as many of the three as the map has pixels)."""
    p = f0.shape[2] * f0.shape[3]
    v0, v1 = f0.flatten(2), f1.flatten(2)
    v0[:, :, 0] = 0
    if p > 1:
        v1[:, :, p - 1] = 0
    if p > 2:
        v0[:, :, p // 2] = 0
        v1[:, :, p // 2] = 0
    return [0] + ([p - 1] if p > 1 else []) + ([p // 2] if p > 2 else [])


def _fwd(f0, f1, lin):
    from where2edit_amd.lpips import head_fwd
    return head_fwd(f0.to(DEV), f1.to(DEV), lin.to(DEV)).cpu()


# ---------------------------------------------------------------------------------------------- the head, forward
@pytest.mark.parametrize("shape,batch", [(s, b) for s in HEAD_SHAPES for b in (1, 3) if b == 1 or s not in LARGE])
def test_head_forward_matches_float64(shape, batch):
    for batch1 in sorted({batch, 1}):
        for scale in (1.0, 1e-3, 1e3):
            f0, f1, lin = _pair(shape, batch, batch1, scale)
            got, ref = _fwd(f0, f1, lin), R.head(f0.double(), f1.double(), lin.double())
            e = rel_err(got, ref)
            print(f"{shape} batch {batch}/{batch1} scale {scale:g}: {e:.2e}")
            assert e <= HEAD_TOL, (shape, batch, batch1, scale, e)
        # near-equal inputs: the difference form holds this, the expansion cannot (test_lpips_ref_host.py)
        f0, f1, lin = _pair(shape, batch, batch1, near=True)
        got, ref = _fwd(f0, f1, lin), R.head(f0.double(), f1.double(), lin.double())
        print(f"{shape} batch {batch}/{batch1} near-equal: {rel_err(got, ref):.2e}")
        assert rel_err(got, ref) <= HEAD_TOL, (shape, batch, batch1, "near-equal", rel_err(got, ref))


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_forward_zero_on_equal_inputs_finite_at_zero_norm_and_bit_reproducible(shape):
    f0, f1, lin = _pair(shape, 3, 3)
    assert torch.equal(_fwd(f0, f0.clone(), lin), torch.zeros(3))
    assert torch.equal(_fwd(f0, f0[:1].clone(), lin)[:1], torch.zeros(1))
    a, b = _fwd(f0, f1, lin), _fwd(f0, f1, lin)
    assert torch.equal(a, b)
    # out[b] does not depend on the batch it was computed in, and the broadcast f1 equals the repeated one bit for bit
    assert torch.equal(_fwd(f0[1:2].contiguous(), f1[1:2].contiguous(), lin), a[1:2])
    assert torch.equal(_fwd(f0, f1[:1].contiguous(), lin), _fwd(f0, f1[:1].expand_as(f0).contiguous(), lin))
    _plant_zero_pixels(f0, f1)
    got, ref = _fwd(f0, f1, lin), R.head(f0.double(), f1.double(), lin.double())
    assert torch.isfinite(got).all() and rel_err(got, ref) <= HEAD_TOL, (got, ref)


# ---------------------------------------------------------------------------------------------- the head, backward
def _bwd(f0, f1, lin, gout, want_g1, prior=None, relu=True):
    from where2edit_amd.lpips import head_bwd
    g0 = prior[0].to(DEV) if prior else None
    g1 = prior[1].to(DEV) if prior and want_g1 else None
    g0, g1 = head_bwd(f0.to(DEV), f1.to(DEV), lin.to(DEV), gout.to(DEV), g0=g0, g1=g1, want_g1=want_g1, accumulate=prior is not None, relu=relu)
    return g0.cpu(), (g1.cpu() if want_g1 else None)


def _variant(g, f, prior, relu):
    """What the kernel is asked for, from the head's plain gradient g at f: + what the tensor held (accumulate), then the mask."""
    g = g if prior is None else g + prior.to(g.dtype)
    return g * (f > 0) if relu else g


def _held(got, own, ref, what):
    """rel_err(got, ref) <= 1e-5 -- unless the closed form evaluated in fp32 on the CPU (`own`, the same variant) is itself more than
    5e-6 from float64 on this input: then twice that distance.  Measured on the host for these inputs: 6e-8 ... 3e-7 on the random
    pairs at every scale, masked or not; 1.5e-6 ... 1.06e-5 on the near-equal pairs (e = u0 - u1 is a difference of nearly equal
    fp32 numbers there, whatever evaluates it), worst at (512,14,14) and (512,1,1) -- DESIGN.md K19."""
    e, mine = rel_err(got, ref), rel_err(own, ref)
    tol = 2 * mine if mine > 5e-6 else HEAD_TOL
    print(f"{what}: {e:.2e} (fp32 CPU {mine:.2e}, held to {tol:.1e})")
    assert e <= tol, (what, e, mine, tol)


@pytest.mark.parametrize("shape,batch", [(s, b) for s in HEAD_SHAPES for b in (1, 3) if b == 1 or s not in LARGE])
def test_head_backward_matches_the_closed_form_in_float64(shape, batch):
    gout = seeded.tensor(f"lp.gout{shape}", (batch,))
    for scale in (1.0, 1e-3, 1e3):
        f0, f1, lin = _pair(shape, batch, batch, scale)
        ref = R.head_grad(f0.double(), f1.double(), lin.double(), gout.double())
        own = R.head_grad(f0, f1, lin, gout)
        # what the next slice would have left in g0 / g1: the head's own size, so that both addends count
        amp = max(float(t.abs().max()) for t in ref)
        priors = (seeded.tensor(f"lp.p0{shape}", tuple(f0.shape), amp), seeded.tensor(f"lp.p1{shape}", tuple(f0.shape), amp))
        for relu in (True, False):
            for pr in (None, priors):
                got = _bwd(f0, f1, lin, gout, True, pr, relu)
                for side, f in enumerate((f0, f1)):
                    p = None if pr is None else pr[side]
                    _held(got[side], _variant(own[side], f, p, relu), _variant(ref[side], f, p, relu),
                          f"{shape} batch {batch} scale {scale:g} relu {relu} accumulate {pr is not None} g{side}")
    # g0 alone, with equal batches and with a broadcast f1; near-equal inputs
    for batch1, near in ((batch, False), (1, False), (batch, True)):
        f0, f1, lin = _pair(shape, batch, batch1, near=near)
        g0, none = _bwd(f0, f1, lin, gout, False)
        assert none is None
        ref = R.head_grad(f0.double(), f1.double(), lin.double(), gout.double())[0]
        _held(g0, _variant(R.head_grad(f0, f1, lin, gout)[0], f0, None, True), _variant(ref, f0, None, True),
              f"{shape} batch {batch}/{batch1} near {near} g0")


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_backward_at_zero_norm_pixels_and_on_equal_inputs(shape):
    f0, f1, lin = _pair(shape, 2, 2)
    gout = seeded.tensor(f"lp.gout0{shape}", (2,))
    planted = _plant_zero_pixels(f0, f1)
    g0, g1 = _bwd(f0, f1, lin, gout, True)
    ref = R.head_grad(f0.double(), f1.double(), lin.double(), gout.double())
    own = R.head_grad(f0, f1, lin, gout)
    assert torch.isfinite(g0).all() and torch.isfinite(g1).all()
    _held(g0, _variant(own[0], f0, None, True), _variant(ref[0], f0, None, True), f"{shape} planted zero pixels g0")
    _held(g1, _variant(own[1], f1, None, True), _variant(ref[1], f1, None, True), f"{shape} planted zero pixels g1")
    v0, v1 = g0.flatten(2), g1.flatten(2)
    assert not v0[:, :, planted[0]].any()  # behind the ReLU mask a zero-norm pixel's gradient is exactly 0
    if len(planted) > 1:
        assert not v1[:, :, planted[1]].any()
    if len(planted) > 2:
        assert not v0[:, :, planted[2]].any() and not v1[:, :, planted[2]].any()
    # unmasked: still finite, still the closed form under the convention
    g0, g1 = _bwd(f0, f1, lin, gout, True, relu=False)
    assert torch.isfinite(g0).all() and torch.isfinite(g1).all()
    _held(g0, own[0], ref[0], f"{shape} planted zero pixels, unmasked g0")
    _held(g1, own[1], ref[1], f"{shape} planted zero pixels, unmasked g1")
    # equal inputs: e = 0 exactly, so the gradient is exactly 0; two calls are bit-equal
    g0, g1 = _bwd(f0, f0.clone(), lin, gout, True)
    assert not g0.any() and not g1.any()
    a, b = _bwd(f0, f1, lin, gout, True), _bwd(f0, f1, lin, gout, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def model():
    from where2edit_amd.lpips import LPIPS
    return LPIPS().to(DEV)


@pytest.fixture(scope="module")
def sd64(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


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


def test_vgg16_and_lpips_run_one_trunk(model, w2e_opt):
    """Vgg16 holding LPIPS's first ten convolutions gives, on the scaled input, the bits of LPIPS's own first four taps: the same
    inputs in the same batch through the same calls (deterministic mode; odd height and width, so every pool floors)."""
    from where2edit_amd import irse_hip as IR
    from where2edit_amd.perceptual_loss import Vgg16, feature_state_dict
    w2e_opt("deterministic", "1")
    vgg = Vgg16()
    vgg.load_state_dict(feature_state_dict(model.net.state_dict()), strict=True)  # its `slice{k}.{i}.*` keys; slice5 is ignored
    vgg = vgg.to(DEV)
    x = torch.cat(R.inputs((2, 3, 33, 47))).to(DEV)
    plan = model.plan()
    acts = _hip_activations(model, x)
    with torch.no_grad():
        outs = vgg(IR.affine_act(x, plan.a, plan.b))
    for name, o, i in zip(outs._fields, outs, (2, 7, 14, 21)):
        assert torch.equal(o.cpu(), acts[i]), name


@pytest.mark.parametrize("wino", ["auto", False])
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (2, 3, 33, 47), (1, 3, 64, 48)])
def test_module_matches_float64_with_input_gradients(model, sd64, shape, wino, w2e_opt):
    """The distance and the five terms against float64's own forward; the gradients to in0 and in1 against float64 with the HIP
    forward's discrete decisions (ReLU signs, pool windows), as the Vgg16 tests compare them.  Deterministic mode, so that the
    forward that is differentiated and the one the decisions are read from are the same bits."""
    from where2edit_amd import functional as K
    w2e_opt("deterministic", "1")
    x, y = R.inputs(shape)
    b = shape[0]
    r = seeded.tensor(f"lpips.r{shape}", (b,)).abs() + 0.5
    xg, yg = x.to(DEV).requires_grad_(True), y.to(DEV).requires_grad_(True)
    K.set_winograd(wino)
    try:
        d, terms = model(xg, yg, retPerLayer=True)
        gx, gy = torch.autograd.grad((d.reshape(-1) * r.to(DEV)).sum(), [xg, yg])
        route = _hip_activations(model, torch.cat([xg.detach(), yg.detach()]))
    finally:
        K.set_winograd("auto")
    assert d.shape == (b, 1, 1, 1) and d.dtype == torch.float32 and len(terms) == 5 and all(t.shape == (b, 1, 1, 1) for t in terms)
    ref, ref_terms = R.lpips(sd64, x.double(), y.double())
    assert_close(d.reshape(-1), ref, 1e-4, f"LPIPS {shape} winograd {wino}")
    for k, (t, rt) in enumerate(zip(terms, ref_terms)):
        assert_close(t.reshape(-1), rt, 1e-4, f"LPIPS term {k} {shape} winograd {wino}")
    xd, yd = x.double().requires_grad_(True), y.double().requires_grad_(True)
    routed, _ = R.lpips(sd64, xd, yd, route=route)
    rx, ry = torch.autograd.grad((routed * r.double()).sum(), [xd, yd])
    assert_grad_close(gx, rx, f"LPIPS gradient to in0 {shape} winograd {wino}")
    assert_grad_close(gy, ry, f"LPIPS gradient to in1 {shape} winograd {wino}")


def test_module_normalize_and_broadcast(model, sd64):
    x, y = R.inputs((2, 3, 33, 47))
    x, y = x.to(DEV), y.to(DEV)
    with torch.no_grad():
        d = model(x, y)
        # normalize=True takes [0, 1] and maps it with 2x - 1 first ((x + 1) / 2 is exact to an ulp, so 1e-6 of the distance)
        assert_close(model((x + 1) / 2, (y + 1) / 2, normalize=True), model(2 * ((x + 1) / 2) - 1, 2 * ((y + 1) / 2) - 1), 0, "normalize")
        assert_close(model((x + 1) / 2, (y + 1) / 2, normalize=True), d, 1e-4, "normalize vs the [-1, 1] call")
    # a batch-1 in1 is broadcast and equals the repeated one.  Its features are computed once, in a merged batch of 3 rows against 4:
    # two fp32 evaluations of one function whose convolutions may pick other tiles, each held to 1e-4 of float64 above -- 2e-4 apart
    # at the most; the gradient to in0 by the default of assert_grad_close.
    xg = x.clone().requires_grad_(True)
    d1 = model(xg, y[:1])
    (g1,) = torch.autograd.grad(d1.sum(), xg)
    d2 = model(xg, y[:1].repeat(2, 1, 1, 1))
    (g2,) = torch.autograd.grad(d2.sum(), xg)
    assert_close(d1, d2, 2e-4, "broadcast in1 vs repeated")
    assert_grad_close(g1, g2, "LPIPS gradient to in0: broadcast in1 vs repeated")
    ref, _ = R.lpips(sd64, x.cpu().double(), y[:1].cpu().double())
    assert_close(d1.reshape(-1), ref, 1e-4, "broadcast in1 vs float64")
    with pytest.raises(RuntimeError, match="broadcast"):
        model(xg, y[:1].clone().requires_grad_(True))
    # in1 alone may take the gradient
    yg = y.clone().requires_grad_(True)
    (gy,) = torch.autograd.grad(model(x, yg).sum(), yg)
    (gy2,) = torch.autograd.grad(model(yg, x).sum(), yg)  # the distance is symmetric
    assert_grad_close(gy, gy2, "LPIPS gradient to in1 alone vs the swapped call")


def test_module_is_exactly_zero_on_equal_images_and_bit_reproducible_in_deterministic_mode(model, w2e_opt):
    w2e_opt("deterministic", "1")
    x, y = R.inputs((2, 3, 33, 47))
    xg, x2 = x.to(DEV).requires_grad_(True), x.to(DEV).clone().requires_grad_(True)
    d = model(xg, x2)
    ga, gb = torch.autograd.grad(d.sum(), [xg, x2])
    assert not d.any() and not ga.any() and not gb.any()
    runs = []
    for _ in range(2):
        xg = x.to(DEV).requires_grad_(True)
        d, terms = model(xg, y.to(DEV), retPerLayer=True)
        (g,) = torch.autograd.grad(d.sum(), xg)
        runs.append([d.detach().clone(), g] + [t.clone() for t in terms])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_forward_and_backward_capture_into_one_graph(model, w2e_opt):
    from where2edit_amd import coach
    w2e_opt("deterministic", "1")
    shape = (2, 3, 32, 32)
    xs = torch.zeros(shape, device=DEV).requires_grad_(True)
    ys = torch.zeros(shape, device=DEV)

    def body():
        d = model(xs, ys)
        (g,) = torch.autograd.grad(d.sum(), xs)
        return d, g

    with torch.no_grad():
        xs.copy_(R.inputs(shape)[0]), ys.copy_(R.inputs(shape)[1])
    graph, (d_static, g_static) = coach.capture_graph(body, "LPIPS forward + backward", torch.device(DEV))
    for salt in (1, 2):
        x = torch.tanh(seeded.tensor("lpips.capture.x", shape, 0.8, salt=salt)).to(DEV)
        y = torch.tanh(seeded.tensor("lpips.capture.y", shape, 0.8, salt=salt)).to(DEV)
        with torch.no_grad():
            xs.copy_(x), ys.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        xe = x.clone().requires_grad_(True)
        de = model(xe, y)
        (ge,) = torch.autograd.grad(de.sum(), xe)
        assert torch.equal(d_static, de.detach()) and torch.equal(g_static, ge), salt


# ---------------------------------------------------------------------------------------------- evaluation
def test_lpips_distance_of_paired_uint8_images(model, w2e_opt):
    from where2edit_amd.evaluation import lpips_distance
    from where2edit_amd.image_io import to_tensor
    w2e_opt("deterministic", "1")  # (two runs of the convolutions are the same bits only without their split-K atomics)
    g = torch.Generator().manual_seed(5)
    a = torch.randint(0, 256, (8, 32, 32, 3), generator=g, dtype=torch.uint8)
    noise = torch.randint(-20, 21, (8, 32, 32, 3), generator=g)
    b = (a.int() + noise).clamp(0, 255).to(torch.uint8)
    out = lpips_distance(a, b, model=model, batch=8)
    with torch.no_grad():
        by_hand = model(to_tensor(a.to(DEV)), to_tensor(b.to(DEV))).reshape(-1)
    assert out["lpips"].shape == (8,) and torch.equal(out["lpips"], by_hand)
    assert abs(out["lpips_mean"] - float(by_hand.double().mean())) <= 1e-6 * float(by_hand.mean())
    # a list of tensors, other batch sizes: the same pairs (the head's result does not depend on the batch; the convolutions' may,
    # within what the forward is held to)
    listed = lpips_distance([a[:3], a[3], a[4:]], [b[:5], b[5:]], model=model, batch=3)
    assert_close(listed["lpips"], by_hand, 2e-4, "lpips_distance in batches of 3")
    with pytest.raises(ValueError, match="8 images, input2 7"):
        lpips_distance(a, b[:7], model=model)
