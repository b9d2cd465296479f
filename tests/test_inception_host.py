"""CPU checks of the FID / Inception Score feature: the float64 reference (tests/inception_ref.py) against independent definitions, the
state-dict schema of where2edit_amd.inception.FeatureExtractorInceptionV3, and the two statistics of where2edit_amd.evaluation against
other formulations (scipy's sqrtm, a numpy loop)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R


# ---------------------------------------------------------------------------------------------- the reference file itself
@pytest.mark.parametrize("h,w", [(1, 1), (7, 5), (299, 299), (300, 298), (40, 611)])
def test_reference_resize_is_the_formula_pixel_by_pixel(h, w):
    g = torch.Generator().manual_seed(h * 1000 + w)
    x = torch.randint(0, 256, (1, h, w, 3), generator=g, dtype=torch.uint8)
    y = R.resize(x)
    assert y.shape == (1, 3, 299, 299) and y.dtype == torch.float64
    xs = x[0].double()
    pts = [(0, 0), (298, 298), (0, 298), (298, 0)] + [tuple(p) for p in torch.randint(0, 299, (200, 2), generator=g).tolist()]
    for oy, ox in pts:
        sy, sx = oy * (h / 299), ox * (w / 299)
        y0, x0 = int(np.floor(sy)), int(np.floor(sx))
        y1, x1 = min(y0 + 1, h - 1), min(x0 + 1, w - 1)
        ty, tx = sy - y0, sx - x0
        for c in range(3):
            top = xs[y0, x0, c] + (xs[y0, x1, c] - xs[y0, x0, c]) * tx
            bot = xs[y1, x0, c] + (xs[y1, x1, c] - xs[y1, x0, c]) * tx
            want = ((top + (bot - top) * ty) - 128) / 128
            assert abs(float(y[0, c, oy, ox]) - float(want)) <= 1e-12, (oy, ox, c)
    if (h, w) == (299, 299):
        assert torch.equal(y, (x.permute(0, 3, 1, 2).double() - 128) / 128)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 7), (17, 17)])
def test_reference_exclusive_average_is_avg_pool2d_without_the_padding(h, w):
    x = torch.randn(2, 3, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(h))
    want = F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
    assert (R.avg_pool_exclusive(x) - want).abs().max() <= 1e-14


def test_reference_folded_bn_is_batch_norm_in_eval_mode():
    sd = R.seeded_state_dict()
    name = "Mixed_5b.branch5x5_2"
    x = torch.randn(2, 64, 4, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = F.batch_norm(x, sd[name + ".bn.running_mean"].double(), sd[name + ".bn.running_var"].double(), sd[name + ".bn.weight"].double(),
                        sd[name + ".bn.bias"].double(), training=False, eps=1e-3)
    scale, shift = R.fold_bn(sd, name)
    assert (x * scale[None, :, None, None] + shift[None, :, None, None] - want).abs().max() <= 1e-13


def test_reference_layer_table_widths_and_sizes():
    table = R.layer_table()
    assert len(table) == 94 and len({t["name"] for t in table}) == 94
    forms = {(t["k"], t["stride"], t["pad"]) for t in table}
    assert forms == {((1, 1), 1, (0, 0)), ((3, 3), 1, (0, 0)), ((3, 3), 1, (1, 1)), ((3, 3), 2, (0, 0)), ((5, 5), 1, (2, 2)), ((1, 7), 1, (0, 3)),
                     ((7, 1), 1, (3, 0)), ((1, 3), 1, (0, 1)), ((3, 1), 1, (1, 0))}
    # shapes through the whole network, on the meta device: no arithmetic
    sd = {k: torch.empty(v.shape, device="meta") for k, v in R.seeded_state_dict().items()}
    trace = []
    x = torch.empty(1, 3, 299, 299, device="meta")
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        x = F.conv2d(x, sd[name + ".conv.weight"], stride=R.TABLE[name]["stride"], padding=R.TABLE[name]["pad"])
        trace.append(x.shape[-1])
    x = R.max_pool_s2(x)
    trace.append(x.shape[-1])
    for name in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
        x = F.conv2d(x, sd[name + ".conv.weight"], stride=R.TABLE[name]["stride"], padding=R.TABLE[name]["pad"])
        trace.append(x.shape[-1])
    x = R.max_pool_s2(x)
    trace.append(x.shape[-1])
    assert trace == [149, 147, 147, 73, 73, 71, 35]
    widths, sizes = [], []
    for name in R.BLOCK_NAMES:
        x = R.block(sd, name, x.to(torch.float32))
        widths.append(x.shape[1]), sizes.append(x.shape[-1])
    assert widths == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    assert sizes == [35, 35, 35, 17, 17, 17, 17, 17, 8, 8, 8]


def test_package_layer_table_is_the_reference_table():
    from where2edit_amd import inception as I
    assert len(I.LAYERS) == 94
    for (name, cin, cout, kh, kw, stride, ph, pw), t in zip(I.LAYERS, R.layer_table()):
        assert (name, cin, cout, (kh, kw), stride, (ph, pw)) == (t["name"], t["cin"], t["cout"], t["k"], t["stride"], t["pad"])
    sd = R.seeded_state_dict()
    scale, shift = I.fold_bn(*(sd["Mixed_7a.branch3x3_2.bn." + k] for k in ("weight", "bias", "running_mean", "running_var")))
    rs, rh = R.fold_bn(sd, "Mixed_7a.branch3x3_2")
    assert torch.equal(scale, rs.float()) and torch.equal(shift, rh.float())


# ---------------------------------------------------------------------------------------------- state-dict schema
def test_state_dict_schema_and_loader():
    from where2edit_amd import FeatureExtractorInceptionV3
    from where2edit_amd.inception import state_dict_shapes
    net = FeatureExtractorInceptionV3()
    ref = R.seeded_state_dict()
    own = net.state_dict()
    assert len(own) == 472 == len(ref) == len(state_dict_shapes())
    assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in ref.items()} == state_dict_shapes()
    assert tuple(own["fc.weight"].shape) == (1008, 2048) and tuple(own["fc.bias"].shape) == (1008,)
    net.load_state_dict(ref)
    assert all(torch.equal(net.state_dict()[k], v) for k, v in ref.items())
    tracked = R.seeded_state_dict(tracked=True)
    assert len(tracked) == 472 + 94
    net2 = FeatureExtractorInceptionV3(seed=3)
    net2.load_state_dict(tracked)
    assert all(torch.equal(net2.state_dict()[k], v) for k, v in ref.items())
    missing = dict(ref)
    del missing["Mixed_6c.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(KeyError, match=r"Mixed_6c\.branch7x7dbl_3\.bn\.running_var"):
        net.load_state_dict(missing)
    bad = dict(ref)
    bad["Mixed_7c.branch3x3_2b.conv.weight"] = torch.zeros(384, 384, 1, 3)
    with pytest.raises(RuntimeError, match=r"Mixed_7c\.branch3x3_2b\.conv\.weight has shape \(384, 384, 1, 3\), expected \(384, 384, 3, 1\)"):
        net.load_state_dict(bad)
    # two constructions with one seed agree; the random initialisation is said to be one
    assert torch.equal(FeatureExtractorInceptionV3().state_dict()["Conv2d_1a_3x3.conv.weight"], FeatureExtractorInceptionV3().state_dict()["Conv2d_1a_3x3.conv.weight"])
    assert "RANDOM" in FeatureExtractorInceptionV3.__doc__


def test_trainable_parameter_and_cpu_input_are_refused():
    from where2edit_amd import FeatureExtractorInceptionV3
    net = FeatureExtractorInceptionV3()
    assert not any(p.requires_grad for p in net.parameters())
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="on the GPU"):  # no CPU path
        net(x)
    with pytest.raises(ValueError, match="unknown feature"):
        net(x, features=("4096",))
    net.Mixed_5b.branch1x1.bn.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="requires grad"):
        net(x)


# ---------------------------------------------------------------------------------------------- the statistics
def _rectified(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5
    return torch.relu(torch.randn(n, d, generator=g, dtype=torch.float64) @ mix + 0.3 * torch.randn(d, generator=g, dtype=torch.float64))


@pytest.mark.parametrize("d,n,tol", [(64, 500, 1e-10), (256, 1000, 1e-10), (64, 40, 1e-6)])
def test_fid_against_the_sqrtm_formulation(d, n, tol):
    """Measured: 6e-15 (D = 64, N = 500) and 1e-15 (D = 256, N = 1000) for full-rank covariances, 9e-9 for the rank-deficient D = 64,
    N = 40 (where sqrtm itself is at its limits)."""
    from where2edit_amd.evaluation import fid_from_features
    f1, f2 = _rectified(n, d, 1), _rectified(n, d, 2) * 1.1 + 0.05
    want = R.fid_sqrtm(f1.numpy(), f2.numpy())
    got = fid_from_features(f1, f2)
    print(f"FID D={d} N={n}: {got:.12g} vs sqrtm {want:.12g}, relative {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) <= tol * abs(want)
    # fp32 inputs are taken to float64, not computed in fp32
    assert fid_from_features(f1.float(), f2.float()) == fid_from_features(f1.float().double(), f2.float().double())


def test_fid_of_a_set_against_itself_is_zero():
    from where2edit_amd.evaluation import feature_statistics, fid_from_features
    for d, n in ((64, 500), (64, 40)):
        f = _rectified(n, d, 5)
        _, s = feature_statistics(f)
        assert torch.allclose(s, torch.from_numpy(np.cov(f.numpy(), rowvar=False)), rtol=1e-12, atol=1e-14)
        assert abs(fid_from_features(f, f)) <= 1e-8 * float(torch.trace(s))


@pytest.mark.parametrize("n,splits", [(100, 10), (57, 10), (23, 1), (31, 3)])
def test_inception_score_against_a_numpy_loop(n, splits):
    from where2edit_amd.evaluation import isc_from_logits
    logits = 2.0 * torch.randn(n, 1008, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    mean, std = isc_from_logits(logits, splits=splits)
    want_mean, want_std = R.isc_loop(logits.numpy(), splits=splits, seed=2020)
    assert abs(mean - want_mean) <= 1e-12 * want_mean and abs(std - want_std) <= 1e-12 * max(want_std, 1.0)
    if splits == 1:
        assert std == 0.0
    else:
        other = R.isc_loop(logits.numpy(), splits=splits, seed=2021)
        assert abs(other[1] - want_std) > 1e-9, "the permutation does not matter for this input: the seed is not tested"
        assert isc_from_logits(logits, splits=splits, rng_seed=2021) == pytest.approx(other, rel=1e-12)
        unshuffled = isc_from_logits(logits, splits=splits, shuffle=False)
        assert unshuffled == pytest.approx(R.isc_loop(logits.numpy(), splits=splits, shuffle=False), rel=1e-12)
    assert isc_from_logits(logits.float(), splits=splits) == isc_from_logits(logits.float().double(), splits=splits)


def test_public_names_are_exported():
    import where2edit_amd as W
    from where2edit_amd import evaluation, inception
    assert W.FeatureExtractorInceptionV3 is inception.FeatureExtractorInceptionV3
    assert W.calculate_metrics is evaluation.calculate_metrics and W.EditMetrics is evaluation.EditMetrics
