"""Float64 restatement of the elementwise / reduction entry points of include/w2e_irse.h (the IR-SE50 / e4e / VGG critics), written
from the header's formulas: the yardstick of tests/test_gpu_irse_kernels.py, itself checked against float64 autograd in
tests/test_irse_ref_host.py.  CPU only, plain torch.  Every function takes tensors of any float dtype and computes in float64; the
`*_scale` twins evaluate the same formula on absolute values -- the size of the terms that were rounded, which is what an error of a
few fp32 roundings is measured against."""
import torch


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().double().cpu()


def _per_channel(v, like, default):
    """[C] -> [1,C,1,1] in float64, or the scalar the header gives a NULL pointer."""
    if v is None:
        return torch.full((1, 1, 1, 1), float(default), dtype=torch.float64)
    v = _d(v)
    assert v.shape == (like.shape[1],), (v.shape, like.shape)
    return v.reshape(1, -1, 1, 1)


def _per_plane(v, like):
    v = _d(v)
    assert v.shape == like.shape[:2], (v.shape, like.shape)
    return v[:, :, None, None]


# ---------------------------------------------------------------------------------------------- the affine pair
def affine_act(x, a=None, b=None, slope=None):
    """w2e_affine_act_fwd: y = prelu(a[c]*x + b[c], slope[c]) over [B,C,H,W]; a / b / slope None = 1 / 0 / identity."""
    x = _d(x)
    pre = _per_channel(a, x, 1) * x + _per_channel(b, x, 0)
    return torch.where(pre > 0, pre, _per_channel(slope, x, 1) * pre)


def affine_act_scale(x, a=None, b=None, slope=None):
    """(|a||x| + |b|) * max(1, |slope|): the terms affine_act rounds."""
    x = _d(x)
    s = _per_channel(slope, x, 1).abs().clamp_min(1.0)
    return (_per_channel(a, x, 1).abs() * x.abs() + _per_channel(b, x, 0).abs()) * s


def affine_act_bwd(gy, y=None, a=None, slope=None):
    """w2e_affine_act_bwd, dense form: gx = a[c] * gy * (y > 0 ? 1 : slope[c]) with y the forward OUTPUT; y None = no mask at all,
    a / slope None = 1 / identity.  (The planar form is this on planar_crop(T).)"""
    gy = _d(gy)
    gx = _per_channel(a, gy, 1) * gy
    if y is not None:
        y = _d(y)
        assert y.shape == gy.shape
        gx = gx * torch.where(y > 0, torch.ones_like(gy), _per_channel(slope, gy, 1).expand_as(gy))
    return gx


def affine_act_bwd_scale(gy, y=None, a=None, slope=None):
    gy = _d(gy)
    return _per_channel(a, gy, 1).abs() * gy.abs() * (_per_channel(slope, gy, 1).abs().clamp_min(1.0) if y is not None else 1.0)


# ---------------------------------------------------------------------------------------------- the SE block around its gate
def channel_sums(x, y=None):
    """w2e_channel_sums: sums[b,c] = sum_p x[b,c,p] * (y ? y[b,c,p] : 1)."""
    x = _d(x)
    return (x if y is None else x * _d(y)).sum((2, 3))


def channel_sums_scale(x, y=None):
    """sum_p |x*y| per plane."""
    x = _d(x)
    return (x if y is None else x * _d(y)).abs().sum((2, 3))


def _strided(shortcut, like, sc_stride):
    """sc_stride 0: a tensor of `like`'s shape; s >= 1: x[b,c,s*y,s*x] of a [B,C,s*H,s*W] tensor (MaxPool2d(1, s))."""
    sc = _d(shortcut)
    b, c, h, w = like.shape
    if sc_stride == 0:
        assert sc.shape == like.shape, (sc.shape, like.shape)
        return sc
    assert sc.shape == (b, c, sc_stride * h, sc_stride * w), (sc.shape, like.shape, sc_stride)
    return sc[:, :, ::sc_stride, ::sc_stride]


def se_apply(t, gate, shortcut, sc_stride=0):
    """w2e_se_apply_fwd: out[b,c,p] = t[b,c,p]*gate[b,c] + shortcut."""
    t = _d(t)
    return t * _per_plane(gate, t) + _strided(shortcut, t, sc_stride)


def se_apply_scale(t, gate, shortcut, sc_stride=0):
    t = _d(t)
    return t.abs() * _per_plane(gate, t).abs() + _strided(shortcut, t, sc_stride).abs()


def se_apply_bwd(gout, gate, gpool):
    """w2e_se_apply_bwd: g_t = gout*gate[b,c] + gpool[b,c]."""
    gout = _d(gout)
    return gout * _per_plane(gate, gout) + _per_plane(gpool, gout)


def se_apply_bwd_scale(gout, gate, gpool):
    gout = _d(gout)
    return gout.abs() * _per_plane(gate, gout).abs() + _per_plane(gpool, gout).abs()


def shortcut_add_bwd(gx, g, stride=1):
    """w2e_shortcut_add_bwd, dense form: a copy of gx [B,C,s*H,s*W] with g [B,C,H,W] added at the strided positions."""
    gx, g = _d(gx).clone(), _d(g)
    b, c, h, w = g.shape
    assert stride >= 1 and gx.shape == (b, c, stride * h, stride * w), (gx.shape, g.shape, stride)
    gx[:, :, ::stride, ::stride] += g
    return gx


# ---------------------------------------------------------------------------------------------- the phase-planar layout of W2E_CONV_UP
def to_planar(dense, fill):
    """[B,C,2h+1,2w+1] -> the UP conv's phase-planar [B,C,2,2,h+1,WP], WP = functional.planar_pitch(w) (W2E_PLANAR_PITCH,
    include/w2e.h): T[Y][X] = planar[Y&1][X&1][Y>>1][X>>1]; every position that holds no element of `dense` = fill.  Keeps the dtype."""
    from where2edit_amd import functional as K
    b, c, ih, iw = dense.shape
    assert ih % 2 == 1 and iw % 2 == 1, dense.shape
    h, w = (ih - 1) // 2, (iw - 1) // 2
    out = torch.full((b, c, 2, 2, h + 1, K.planar_pitch(w)), fill, dtype=dense.dtype)
    for py in range(2):
        for px in range(2):
            sub = dense[:, :, py::2, px::2]
            out[:, :, py, px, :sub.shape[2], :sub.shape[3]] = sub
    return out


def from_planar(planar, ih, iw):
    """The inverse of to_planar: the dense [B,C,ih,iw] (ih = 2h+1, iw = 2w+1) image of a phase-planar tensor."""
    b, c = planar.shape[:2]
    assert planar.shape[2:5] == (2, 2, (ih + 1) // 2) and planar.shape[5] >= (iw + 1) // 2, (planar.shape, ih, iw)
    out = torch.empty((b, c, ih, iw), dtype=planar.dtype)
    for py in range(2):
        for px in range(2):
            sub = out[:, :, py::2, px::2]
            sub.copy_(planar[:, :, py, px, :sub.shape[2], :sub.shape[3]])
    return out


def planar_crop(planar, height, width):
    """The (+1,+1) crop the planar forms read: T[y+1][x+1] for y < height, x < width (both even) -> [B,C,height,width]."""
    assert height % 2 == 0 and width % 2 == 0, (height, width)
    return from_planar(planar, height + 1, width + 1)[:, :, 1:, 1:]


# ---------------------------------------------------------------------------------------------- seeded inputs
KINK_MARGIN = 1e-3  # every pre-activation of kink_free_inputs is at least this far from 0, in float64, from the fp32 inputs


def channel_params(gen, c, slope_zero=False):
    """Seeded fp32 (a, b, slope) of `c` channels, all different between channels: a in +-(0.5, 1.5) with alternating signs (a negative
    BatchNorm scale is legal), b normal, slope in (0.05, 0.55) or all zero (ReLU)."""
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(c)])
    a = (torch.rand(c, generator=gen) + 0.5) * sign
    b = torch.randn(c, generator=gen)
    slope = torch.zeros(c) if slope_zero else torch.rand(c, generator=gen) * 0.5 + 0.05
    return a.float(), b.float(), slope.float()


def kink_free_inputs(gen, shape, a=None, b=None):
    """fp32 x [B,C,H,W] whose pre-activations a*x + b sit at least KINK_MARGIN from 0 BY CONSTRUCTION: the pre-activation is drawn
    first, as sign * (2*KINK_MARGIN + |normal|), and x solved from it in float64; rounding x to fp32 moves a*x + b by |a*x| * 2^-24,
    three orders of magnitude below the margin.  So the branch of the PReLU is the same in fp32 and in float64 for every element."""
    pre = torch.randn(shape, generator=gen, dtype=torch.float64)
    pre = torch.where(pre >= 0, 1.0, -1.0) * (2 * KINK_MARGIN + pre.abs())
    x = ((pre - _per_channel(b, pre, 0)) / _per_channel(a, pre, 1)).float()
    got = _per_channel(a, pre, 1) * x.double() + _per_channel(b, pre, 0)
    assert float(got.abs().min()) >= KINK_MARGIN and bool(((got > 0) == (pre > 0)).all())
    return x
