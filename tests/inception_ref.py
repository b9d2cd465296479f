"""Float64 restatement of the FID Inception-v3 feature extractor (torch_fidelity's `FeatureExtractorInceptionV3`, the
`pt_inception-2015-12-05` network) from stock torch.nn.functional calls, with its own layer table and seeded weights.  Written
independently of where2edit_amd/inception.py: the tests compare the two.  Test-only; runs on the CPU."""
import torch
import torch.nn.functional as F

EPS = 1e-3
SIZE = 299


def _bc(name, cin, cout, k=(1, 1), stride=1, pad=(0, 0)):
    return dict(name=name, cin=cin, cout=cout, k=k, stride=stride, pad=pad)


def layer_table():
    """The 94 BasicConv2d layers, in network order."""
    t = [_bc("Conv2d_1a_3x3", 3, 32, (3, 3), 2), _bc("Conv2d_2a_3x3", 32, 32, (3, 3)), _bc("Conv2d_2b_3x3", 32, 64, (3, 3), 1, (1, 1)),
         _bc("Conv2d_3b_1x1", 64, 80), _bc("Conv2d_4a_3x3", 80, 192, (3, 3))]
    for n, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        t += [_bc(n + ".branch1x1", cin, 64), _bc(n + ".branch5x5_1", cin, 48), _bc(n + ".branch5x5_2", 48, 64, (5, 5), 1, (2, 2)),
              _bc(n + ".branch3x3dbl_1", cin, 64), _bc(n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
              _bc(n + ".branch3x3dbl_3", 96, 96, (3, 3), 1, (1, 1)), _bc(n + ".branch_pool", cin, pf)]
    n = "Mixed_6a"
    t += [_bc(n + ".branch3x3", 288, 384, (3, 3), 2), _bc(n + ".branch3x3dbl_1", 288, 64), _bc(n + ".branch3x3dbl_2", 64, 96, (3, 3), 1, (1, 1)),
          _bc(n + ".branch3x3dbl_3", 96, 96, (3, 3), 2)]
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        t += [_bc(n + ".branch1x1", 768, 192), _bc(n + ".branch7x7_1", 768, c7), _bc(n + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3)),
              _bc(n + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0)), _bc(n + ".branch7x7dbl_1", 768, c7),
              _bc(n + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)), _bc(n + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)),
              _bc(n + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)), _bc(n + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)),
              _bc(n + ".branch_pool", 768, 192)]
    n = "Mixed_7a"
    t += [_bc(n + ".branch3x3_1", 768, 192), _bc(n + ".branch3x3_2", 192, 320, (3, 3), 2), _bc(n + ".branch7x7x3_1", 768, 192),
          _bc(n + ".branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)), _bc(n + ".branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)),
          _bc(n + ".branch7x7x3_4", 192, 192, (3, 3), 2)]
    for n, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        t += [_bc(n + ".branch1x1", cin, 320), _bc(n + ".branch3x3_1", cin, 384), _bc(n + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)),
              _bc(n + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)), _bc(n + ".branch3x3dbl_1", cin, 448),
              _bc(n + ".branch3x3dbl_2", 448, 384, (3, 3), 1, (1, 1)), _bc(n + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)),
              _bc(n + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)), _bc(n + ".branch_pool", cin, 192)]
    return t


TABLE = {layer["name"]: layer for layer in layer_table()}


def seeded_state_dict(seed=7, tracked=False):
    """The seeded weights (fp32): conv N(0, 2 / (Cin KH KW)); BN weight 1 + 0.1 n, bias 0.1 n, running_mean 0.1 n, running_var
    U(0.5, 1.5); fc weight N(0, 1 / 2048), bias 0.1 n.  tracked: with the `num_batches_tracked` entries of a real checkpoint."""
    g = torch.Generator().manual_seed(seed)
    n = lambda *shape: torch.randn(*shape, generator=g)
    sd = {}
    for layer in layer_table():
        name, cin, cout, (kh, kw) = layer["name"], layer["cin"], layer["cout"], layer["k"]
        sd[name + ".conv.weight"] = n(cout, cin, kh, kw) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[name + ".bn.weight"] = 1 + 0.1 * n(cout)
        sd[name + ".bn.bias"] = 0.1 * n(cout)
        sd[name + ".bn.running_mean"] = 0.1 * n(cout)
        sd[name + ".bn.running_var"] = 0.5 + torch.rand(cout, generator=g)
        if tracked:
            sd[name + ".bn.num_batches_tracked"] = torch.tensor(0, dtype=torch.int64)
    sd["fc.weight"] = n(1008, 2048) * 2048 ** -0.5
    sd["fc.bias"] = 0.1 * n(1008)
    return sd


def resize(x_u8):
    """uint8 [B,H,W,3] -> float64 [B,3,299,299]: the legacy-TensorFlow bilinear resize (src = dst * (in / 299), no half-pixel offset,
    i1 = min(i0 + 1, in - 1)) and (v - 128) / 128."""
    x = x_u8.permute(0, 3, 1, 2).double()
    _, _, h, w = x.shape

    def axis(n):
        src = torch.arange(SIZE, dtype=torch.float64) * (n / SIZE)
        i0 = torch.floor(src).long()
        return i0, torch.clamp(i0 + 1, max=n - 1), src - i0

    y0, y1, ty = axis(h)
    x0, x1, tx = axis(w)
    top = x[:, :, y0][:, :, :, x0] + (x[:, :, y0][:, :, :, x1] - x[:, :, y0][:, :, :, x0]) * tx
    bot = x[:, :, y1][:, :, :, x0] + (x[:, :, y1][:, :, :, x1] - x[:, :, y1][:, :, :, x0]) * tx
    return ((top + (bot - top) * ty[:, None]) - 128.0) / 128.0


def fold_bn(sd, name):
    """Eval-mode BatchNorm as (scale, shift), float64."""
    scale = sd[name + ".bn.weight"].double() / torch.sqrt(sd[name + ".bn.running_var"].double() + EPS)
    return scale, sd[name + ".bn.bias"].double() - sd[name + ".bn.running_mean"].double() * scale


def basic_conv(sd, name, x):
    layer = TABLE[name]
    y = F.conv2d(x, sd[name + ".conv.weight"].to(x.dtype), stride=layer["stride"], padding=layer["pad"])
    scale, shift = fold_bn(sd, name)
    return F.relu(y * scale.to(x.dtype)[None, :, None, None] + shift.to(x.dtype)[None, :, None, None])


def avg_pool_exclusive(x):
    """3x3, stride 1, padding 1, divided by the number of taps inside the image -- written out, not through avg_pool2d."""
    ones = torch.ones_like(x[:1, :1])
    k = torch.ones(1, 1, 3, 3, dtype=x.dtype, device=x.device)
    b, c, h, w = x.shape
    s = F.conv2d(x.reshape(b * c, 1, h, w), k, padding=1).reshape(b, c, h, w)
    return s / F.conv2d(ones, k, padding=1)


def max_pool_s2(x):
    return F.max_pool2d(x, 3, 2)


def max_pool_s1(x):
    return F.max_pool2d(x, 3, 1, 1)


def block(sd, name, x):
    cv = lambda leaf, t: basic_conv(sd, f"{name}.{leaf}", t)
    if name in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        return torch.cat([cv("branch1x1", x), cv("branch5x5_2", cv("branch5x5_1", x)),
                          cv("branch3x3dbl_3", cv("branch3x3dbl_2", cv("branch3x3dbl_1", x))), cv("branch_pool", avg_pool_exclusive(x))], 1)
    if name == "Mixed_6a":
        return torch.cat([cv("branch3x3", x), cv("branch3x3dbl_3", cv("branch3x3dbl_2", cv("branch3x3dbl_1", x))), max_pool_s2(x)], 1)
    if name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        t = cv("branch7x7dbl_1", x)
        for leaf in ("branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"):
            t = cv(leaf, t)
        return torch.cat([cv("branch1x1", x), cv("branch7x7_3", cv("branch7x7_2", cv("branch7x7_1", x))), t,
                          cv("branch_pool", avg_pool_exclusive(x))], 1)
    if name == "Mixed_7a":
        t = cv("branch7x7x3_1", x)
        for leaf in ("branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"):
            t = cv(leaf, t)
        return torch.cat([cv("branch3x3_2", cv("branch3x3_1", x)), t, max_pool_s2(x)], 1)
    assert name in ("Mixed_7b", "Mixed_7c"), name
    a = cv("branch3x3_1", x)
    d = cv("branch3x3dbl_2", cv("branch3x3dbl_1", x))
    pooled = avg_pool_exclusive(x) if name == "Mixed_7b" else max_pool_s1(x)
    return torch.cat([cv("branch1x1", x), cv("branch3x3_2a", a), cv("branch3x3_2b", a), cv("branch3x3dbl_3a", d), cv("branch3x3dbl_3b", d),
                      cv("branch_pool", pooled)], 1)


BLOCK_NAMES = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")


def forward(sd, x_u8, dtype=torch.float64, trace=None):
    """{'768', '2048', 'logits_unbiased', 'logits'} of uint8 [B,H,W,3].  trace: a list that receives (name, shape) after each stage."""
    note = (lambda name, t: trace.append((name, tuple(t.shape)))) if trace is not None else (lambda name, t: None)
    x = resize(x_u8).to(dtype)
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        x = basic_conv(sd, name, x)
        note(name, x)
    x = max_pool_s2(x)
    note("pool1", x)
    for name in ("Conv2d_3b_1x1", "Conv2d_4a_3x3"):
        x = basic_conv(sd, name, x)
        note(name, x)
    x = max_pool_s2(x)
    note("pool2", x)
    out = {}
    for name in BLOCK_NAMES:
        x = block(sd, name, x)
        note(name, x)
        if name == "Mixed_6e":
            out["768"] = x.mean((2, 3))
    f = x.mean((2, 3))
    out["2048"] = f
    out["logits_unbiased"] = f @ sd["fc.weight"].to(dtype).T
    out["logits"] = out["logits_unbiased"] + sd["fc.bias"].to(dtype)
    return out


# ---------------------------------------------------------------------------------------------- the statistics, other formulations
def fid_sqrtm(f1, f2, eps=1e-6):
    """FID through scipy.linalg.sqrtm, as torch_fidelity / pytorch-fid compute it, with their 1e-6 offset and `.real` fallbacks."""
    import numpy as np
    import scipy.linalg
    f1, f2 = np.asarray(f1, dtype=np.float64), np.asarray(f2, dtype=np.float64)
    mu1, mu2 = f1.mean(0), f2.mean(0)
    s1, s2 = np.cov(f1, rowvar=False), np.cov(f2, rowvar=False)
    covmean, _ = scipy.linalg.sqrtm(s1.dot(s2), disp=False)
    if not np.isfinite(covmean).all():
        offset = np.eye(s1.shape[0]) * eps
        covmean = scipy.linalg.sqrtm((s1 + offset).dot(s2 + offset))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2 * np.trace(covmean))


def isc_loop(logits, splits=10, seed=2020, shuffle=True):
    """The Inception Score as a plain numpy loop over splits and rows."""
    import numpy as np
    x = np.asarray(logits, dtype=np.float64)
    n = x.shape[0]
    if shuffle:
        x = x[np.random.RandomState(seed).permutation(n)]
    scores = []
    for k in range(splits):
        rows = x[k * n // splits:(k + 1) * n // splits]
        p = np.stack([np.exp(r - r.max()) / np.exp(r - r.max()).sum() for r in rows])
        marginal = p.mean(0)
        kl = [float((pi * (np.log(pi) - np.log(marginal))).sum()) for pi in p]
        scores.append(np.exp(np.mean(kl)))
    return float(np.mean(scores)), float(np.std(scores))
