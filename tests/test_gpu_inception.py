"""The Inception-v3 feature extractor's kernels (include/w2e_inception.h) on the GPU against float64 (tests/inception_ref.py and stock
torch.nn.functional on the CPU): the convolution in all nine geometric forms of the network, the three pools, the input resize, one
block of each kind at reduced size, the whole network, and the metrics on top (calculate_metrics, EditMetrics).

Tolerances: the project's FWD_TOL = 1e-4 under assert_close and per (sample, channel) plane under assert_close_planes, the term scale
being the float64 convolution of |x| and |w| (times |scale|, plus |shift|), as tests/test_gpu_conv_variants.py does.  The max pools are
exact; the average pool and the resize are held to 1e-6."""
import os

import pytest
import torch
import torch.nn.functional as F

import inception_ref as R
from helpers import assert_close, assert_close_planes, rel_err

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-4
CANARY = 12345.0
DEV = "cuda"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _conv_problem(seed, b, cin, n, h, w, k, stride, pad):
    g = _gen(seed)
    kh, kw = k
    x = torch.randn(b, cin, h, w, generator=g)
    wt = torch.randn(n, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    scale = 1 + 0.1 * torch.randn(n, generator=g)
    shift = 0.1 * torch.randn(n, generator=g)
    return x, wt, scale, shift


def _conv_ref(x, wt, scale, shift, stride, pad, relu):
    xd, wd = x.double(), wt.double()
    a = scale.double()[None, :, None, None] if scale is not None else 1.0
    s = shift.double()[None, :, None, None] if shift is not None else 0.0
    y = F.conv2d(xd, wd, stride=stride, padding=pad) * a + s
    absref = F.conv2d(xd.abs(), wd.abs(), stride=stride, padding=pad) * (a.abs() if scale is not None else 1.0) + (s.abs() if shift is not None else 0.0)
    return (F.relu(y) if relu else y), absref


def _run_conv(x, wt, scale, shift, stride, pad, relu, out=None, ch_off=0):
    from where2edit_amd.inception import conv2d_bn_relu
    to = lambda t: None if t is None else t.to(DEV)
    return conv2d_bn_relu(to(x), to(wt), to(scale), to(shift), stride, pad, relu, out, ch_off)


# (form, k, stride, pad): the nine geometric forms of the network
FORMS = {"1x1": ((1, 1), 1, (0, 0)), "3x3p0": ((3, 3), 1, (0, 0)), "3x3p1": ((3, 3), 1, (1, 1)), "3x3s2": ((3, 3), 2, (0, 0)),
         "5x5p2": ((5, 5), 1, (2, 2)), "1x7": ((1, 7), 1, (0, 3)), "7x1": ((7, 1), 1, (3, 0)), "1x3": ((1, 3), 1, (0, 1)), "3x1": ((3, 1), 1, (1, 0))}
# (form, batch, cin, n, h, w, relu): K = 27, 1200, 720, 1120, 4032 among them; every N of {32, 48, 80, 96, 192, 320, 384}
CONV_CASES = [
    ("1x1", 3, 80, 192, 9, 11, True), ("1x1", 1, 448, 320, 8, 8, False), ("1x1", 3, 3, 48, 5, 7, True),
    ("3x3p0", 1, 80, 192, 9, 11, True), ("3x3p0", 3, 48, 80, 5, 7, False),
    ("3x3p1", 1, 448, 384, 8, 8, True), ("3x3p1", 3, 48, 96, 5, 7, False),
    ("3x3s2", 3, 3, 32, 9, 11, True), ("3x3s2", 1, 160, 320, 17, 17, False),
    ("5x5p2", 3, 48, 48, 5, 7, True), ("5x5p2", 1, 48, 80, 17, 17, False),
    ("1x7", 1, 160, 192, 17, 17, True), ("1x7", 3, 160, 80, 5, 7, False),
    ("7x1", 3, 160, 192, 9, 11, True), ("7x1", 1, 80, 32, 17, 17, False),
    ("1x3", 1, 80, 384, 8, 8, True), ("1x3", 3, 448, 96, 5, 7, False),
    ("3x1", 3, 48, 96, 5, 7, False), ("3x1", 1, 160, 320, 8, 8, True),
    # many tiles: the network's first layer at its real size (the 32-channel x 128-position tile) and a 1x1 layer with the 64 x 64 tile
    ("3x3s2", 3, 3, 32, 299, 299, True), ("1x1", 3, 48, 48, 105, 106, False),
    # K = 4680 > 4608: the (k -> offset, tap) table no longer fits beside the tiles and the taps are divided out per load
    ("3x3p1", 1, 520, 32, 5, 7, True),
]


@pytest.mark.parametrize("form,b,cin,n,h,w,relu", CONV_CASES, ids=[f"{c[0]}-b{c[1]}-c{c[2]}-n{c[3]}-{c[4]}x{c[5]}-{'relu' if c[6] else 'id'}" for c in CONV_CASES])
def test_conv_forms_against_float64(form, b, cin, n, h, w, relu):
    k, stride, pad = FORMS[form]
    x, wt, scale, shift = _conv_problem(1000 * cin + 10 * n + b + sum(k), b, cin, n, h, w, k, stride, pad)
    ref, absref = _conv_ref(x, wt, scale, shift, stride, pad, relu)
    y = _run_conv(x, wt, scale, shift, stride, pad, relu)
    if form == "3x3s2" and (h, w) == (9, 11):
        assert tuple(y.shape[2:]) == (4, 5)
    assert y.shape == ref.shape
    what = f"{form} b{b} cin{cin} n{n} {h}x{w}"
    print(f"{what}: rel err {rel_err(y, ref):.2e}")
    assert_close(y, ref, FWD_TOL, what)
    worst = assert_close_planes(y, ref, absref, FWD_TOL, what)
    print(f"{what}: worst plane {worst:.2e}")
    # two runs: equal bits
    assert torch.equal(y, _run_conv(x, wt, scale, shift, stride, pad, relu))
    # a channel slice in the middle of a wider output: the slice holds the same bits, every other byte keeps the canary
    wide = torch.full((b, n + 37, y.shape[2], y.shape[3]), CANARY, device=DEV)
    _run_conv(x, wt, scale, shift, stride, pad, relu, wide, 19)
    assert torch.equal(wide[:, 19:19 + n], y)
    assert bool((wide[:, :19] == CANARY).all()) and bool((wide[:, 19 + n:] == CANARY).all())


@pytest.mark.parametrize("m", [1, 3])
def test_fc_shape_through_the_conv_kernel(m):
    g = _gen(m)
    f = torch.relu(torch.randn(m, 2048, 1, 1, generator=g))
    wt = torch.randn(1008, 2048, 1, 1, generator=g) * 2048 ** -0.5
    bias = 0.1 * torch.randn(1008, generator=g)
    for shift in (None, bias):
        ref, absref = _conv_ref(f, wt, None, shift, 1, (0, 0), False)
        y = _run_conv(f, wt, None, shift, 1, (0, 0), False)
        assert y.shape == (m, 1008, 1, 1)
        assert_close(y, ref, FWD_TOL, f"fc m{m}")
        assert_close_planes(y, ref, absref, FWD_TOL, f"fc m{m}")
        assert torch.equal(y, _run_conv(f, wt, None, shift, 1, (0, 0), False))


def test_conv_refuses_what_it_does_not_cover():
    from where2edit_amd.inception import conv2d_bn_relu
    x = torch.zeros(1, 4, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="1, 3, 5 or 7"):
        conv2d_bn_relu(x, torch.zeros(4, 4, 2, 2, device=DEV), None, None)
    with pytest.raises(RuntimeError, match="stride 3"):
        conv2d_bn_relu(x, torch.zeros(4, 4, 3, 3, device=DEV), None, None, stride=3)
    with pytest.raises(RuntimeError, match="do not lie in an output of 5"):
        conv2d_bn_relu(x, torch.zeros(4, 4, 1, 1, device=DEV), None, None, out=torch.zeros(1, 5, 8, 8, device=DEV), ch_off=2)


# ---------------------------------------------------------------------------------------------- pools
POOL_SIZES = [(3, 3), (4, 4), (5, 7), (8, 8), (17, 17), (35, 35)]


def _pool_ref(x, mode):
    from where2edit_amd import inception as I
    if mode == I.POOL_MAX_S2:
        return F.max_pool2d(x, 3, 2)
    if mode == I.POOL_MAX_S1:
        return F.max_pool2d(x, 3, 1, 1)
    return F.avg_pool2d(x.double(), 3, 1, 1, count_include_pad=False)


@pytest.mark.parametrize("mode_name", ["max_s2", "avg_s1p1", "max_s1p1"])
def test_pool_modes(mode_name):
    from where2edit_amd import inception as I
    mode = {"max_s2": I.POOL_MAX_S2, "avg_s1p1": I.POOL_AVG, "max_s1p1": I.POOL_MAX_S1}[mode_name]
    sizes = POOL_SIZES + ([(1, 1), (2, 3)] if mode == I.POOL_AVG else [])
    for h, w in sizes:
        g = _gen(h * 100 + w)
        x = torch.randn(2, 5, h, w, generator=g)
        x[0, 1] = torch.randint(-2, 3, (h, w), generator=g).float()  # a plane full of ties
        x[1, 2] = -5.0 - torch.rand(h, w, generator=g)               # all negative: a padded zero must never win / be averaged in
        ref = _pool_ref(x, mode)
        y = I.pool3x3(x.to(DEV), mode)
        assert y.shape == ref.shape, (mode_name, h, w)
        if (h, w) == (17, 17) and mode == I.POOL_MAX_S2:
            assert tuple(y.shape[2:]) == (8, 8)
        if (h, w) == (35, 35) and mode == I.POOL_MAX_S2:
            assert tuple(y.shape[2:]) == (17, 17)
        if mode == I.POOL_AVG:
            assert (y.double().cpu() - ref).abs().max() <= 1e-6, (mode_name, h, w)
        else:
            assert torch.equal(y.cpu(), ref), (mode_name, h, w)
        wide = torch.full((2, 5 + 9, y.shape[2], y.shape[3]), CANARY, device=DEV)
        I.pool3x3(x.to(DEV), mode, wide, 3)
        assert torch.equal(wide[:, 3:8], y)
        assert bool((wide[:, :3] == CANARY).all()) and bool((wide[:, 8:] == CANARY).all())


def test_max_pool_propagates_nan_like_torch():
    from where2edit_amd import inception as I
    x = torch.randn(1, 2, 7, 7, generator=_gen(3))
    x[0, 0, 3, 3] = float("nan")
    x[0, 1, 0, 6] = float("nan")
    for mode in (I.POOL_MAX_S2, I.POOL_MAX_S1):
        y, ref = I.pool3x3(x.to(DEV), mode).cpu(), _pool_ref(x, mode)
        assert torch.equal(torch.isnan(y), torch.isnan(ref)) and torch.equal(torch.nan_to_num(y), torch.nan_to_num(ref))


# ---------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (299, 299), (300, 298), (1024, 1024)])
def test_resize_against_the_float64_formula(h, w):
    from where2edit_amd.inception import resize_input
    x = torch.randint(0, 256, (2, h, w, 3), generator=_gen(h + w), dtype=torch.uint8)
    ref = R.resize(x)
    y = resize_input(x.to(DEV))
    assert y.shape == (2, 3, 299, 299) and y.dtype == torch.float32
    err = float((y.double().cpu() - ref).abs().max())
    print(f"resize {h}x{w}: max abs err {err:.2e}")
    assert err <= 1e-6
    if (h, w) == (299, 299):
        assert torch.equal(y.cpu(), ((x.permute(0, 3, 1, 2).float() - 128) / 128))


# ---------------------------------------------------------------------------------------------- blocks and the whole network
@pytest.fixture(scope="module")
def seeded_sd():
    return R.seeded_state_dict()


@pytest.fixture(scope="module")
def net(seeded_sd):
    from where2edit_amd import FeatureExtractorInceptionV3
    m = FeatureExtractorInceptionV3()
    m.load_state_dict(seeded_sd)  # the public loader
    return m.to(DEV)


BLOCK_CASES = [("Mixed_5b", 192, 5, 6), ("Mixed_6c", 768, 5, 6), ("Mixed_6a", 288, 7, 9), ("Mixed_7a", 768, 7, 9), ("Mixed_7b", 1280, 3, 4),
               ("Mixed_7c", 2048, 3, 4)]


@pytest.mark.parametrize("name,cin,h,w", BLOCK_CASES, ids=[c[0] for c in BLOCK_CASES])
def test_blocks_against_float64(net, seeded_sd, name, cin, h, w):
    x = torch.relu(torch.randn(2, cin, h, w, generator=_gen(cin + h)))
    ref = R.block(seeded_sd, name, x.double())
    y = net.block(name, x.to(DEV))
    assert y.shape == ref.shape
    print(f"{name}: rel err {rel_err(y, ref):.2e}")
    assert_close(y, ref, FWD_TOL, name)
    assert torch.equal(y, net.block(name, x.to(DEV)))  # every slice written, by one launch each: two runs give equal bits


@pytest.fixture(scope="module")
def whole_net_cases(seeded_sd):
    g = _gen(11)
    small = torch.randint(0, 256, (2, 64, 48, 3), generator=g, dtype=torch.uint8)
    big = torch.randint(0, 256, (1, 1024, 1024, 3), generator=g, dtype=torch.uint8)
    big[:, 200:700, 100:900] //= 4  # structure that survives the 3.4x down-sampling
    with torch.no_grad():
        return [(small, R.forward(seeded_sd, small)), (big, R.forward(seeded_sd, big))]


def test_whole_network_against_float64(net, whole_net_cases):
    for x, ref in whole_net_cases:
        names = ("768", "2048", "logits_unbiased", "logits")
        outs = net(x.to(DEV), features=names)
        for name, y in zip(names, outs):
            print(f"{tuple(x.shape)} {name}: rel err {rel_err(y, ref[name]):.2e}")
            assert_close(y, ref[name], FWD_TOL, f"{tuple(x.shape)} {name}")
        f, lu = net(x.to(DEV))  # the default features, in their order
        assert torch.equal(f, outs[1]) and torch.equal(lu, outs[2])


# ---------------------------------------------------------------------------------------------- the metrics
def test_calculate_metrics_on_directories_equals_the_tensor_route(net, tmp_path):
    from where2edit_amd import calculate_metrics
    from where2edit_amd.image_io import from_jpeg, save_image
    g = _gen(5)
    decoded = {}
    for d in ("fake", "real"):
        os.makedirs(tmp_path / d)
        base = torch.rand(8, 3, 8, 8, generator=g) * 2 - 1
        imgs = F.interpolate(base, size=64, mode="bilinear", align_corners=False).to(DEV)
        for i in range(8):
            save_image(imgs[i:i + 1], str(tmp_path / d / f"00_{i:05d}.jpg"))
        decoded[d] = [from_jpeg(open(tmp_path / d / f"00_{i:05d}.jpg", "rb").read(), device=DEV) for i in range(8)]
        assert all(tuple(t.shape) == (64, 64, 3) for t in decoded[d])
    by_dir = calculate_metrics(str(tmp_path / "fake"), str(tmp_path / "real"), extractor=net, isc_splits=4)  # eight images: fewer than the default 10 splits
    by_tensor = calculate_metrics(decoded["fake"], torch.stack(decoded["real"]), extractor=net, isc_splits=4)
    with pytest.raises(ValueError, match="N >= splits"):
        calculate_metrics(decoded["fake"], decoded["real"], extractor=net)
    assert set(by_dir) == {"inception_score_mean", "inception_score_std", "frechet_inception_distance"}
    assert by_dir == by_tensor
    assert by_dir["inception_score_mean"] >= 1.0 and by_dir["frechet_inception_distance"] > 0.0
    assert set(calculate_metrics(decoded["fake"], decoded["real"], isc=False, extractor=net, batch=3)) == {"frechet_inception_distance"}


class _ClipStub:
    def preprocess(self, images):
        return F.avg_pool2d(images, 8)

    def encode_image(self, images):
        return images.flatten(1)[:, :32]


def _id_stub(gen, orig):
    return ((gen - orig) ** 2).mean(), 0.0


def test_edit_metrics_equals_the_manual_route(net):
    from where2edit_amd import EditMetrics
    from where2edit_amd.evaluation import fid_from_features, isc_from_logits
    from where2edit_amd.image_io import from_jpeg, to_bytes, to_jpeg
    g = _gen(9)
    metrics = EditMetrics(net, clip_loss=_ClipStub(), id_loss=_id_stub, jpeg=True)
    f_o, f_g, logits, ident, better, count = [], [], [], 0.0, 0, 0
    for step in range(2):
        orig = F.interpolate(torch.rand(6, 3, 8, 8, generator=g) * 2 - 1, size=64, mode="bilinear").to(DEV)
        gen = (orig + 0.2 * F.interpolate(torch.randn(6, 3, 4, 4, generator=g), size=64, mode="bilinear").to(DEV)).clamp(-1, 1)
        text = torch.randn(6, 32, generator=g).to(DEV)
        metrics.update(orig, gen, text)
        route = lambda img: from_jpeg(to_jpeg(to_bytes(img, grid=False)), device=DEV, stack=True)
        f_o.append(net(route(orig), features=("2048",))[0])
        a, b = net(route(gen))
        f_g.append(a), logits.append(b)
        ident += float((1 - _id_stub(gen, orig)[0]) * 6)
        clip = _ClipStub()
        sim = lambda img: torch.cosine_similarity(clip.encode_image(clip.preprocess(img)), text)
        better += int((sim(gen) > sim(orig)).sum())
        count += 6
    inception, fid, ident_got, improve = metrics.compute()
    assert inception == isc_from_logits(torch.cat(logits))[0]
    assert fid == fid_from_features(torch.cat(f_o), torch.cat(f_g))
    assert abs(ident_got - ident / count) <= 1e-6
    assert improve == better / count
    # without the JPEG round trip the features are those of to_bytes' pixels
    plain = EditMetrics(net, jpeg=False)
    plain.update(orig, gen)
    plain.update(gen, orig)
    assert plain.compute()[2:] == (None, None)
    assert torch.equal(plain._f_orig[0], net(to_bytes(orig, grid=False), features=("2048",))[0])
