"""LPIPS-VGG v0.1 (where2edit_amd.lpips) restated on stock torch ops, in the dtype of its inputs (float64 in the tests): the
ScalingLayer, VGG16 configuration D with its five taps, the head in its difference form, and the head's gradient in closed form under
the zero-norm convention of include/w2e_lpips.h.  Own code, written from the published architecture; test-only."""
import torch
import torch.nn.functional as F

CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOLS = (4, 9, 16, 23)
SLICES = (range(0, 4), range(4, 9), range(9, 16), range(16, 23), range(23, 30))
CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10


def unit(f):
    """(u, n): f / (n + eps) and n = sqrt(sum_c f_c^2), over dim 1."""
    n = f.pow(2).sum(1, keepdim=True).sqrt()
    return f / (n + EPS), n


def head(f0, f1, w):
    """d [B] = mean_p sum_c w_c (u0_c - u1_c)^2 of f0 [B,C,h,w] against f1 [B or 1,C,h,w]; differentiable by autograd wherever no
    pixel has n = 0."""
    e = unit(f0)[0] - unit(f1)[0]
    return (w.reshape(1, -1, 1, 1).to(e) * e * e).sum(1).flatten(1).mean(1)


def head_expansion(f0, f1, w):
    """The same number as sum w u0^2 - 2 sum w u0 u1 + sum w u1^2: the form the kernels must NOT use (it cancels)."""
    u0, u1 = unit(f0)[0], unit(f1)[0]
    w = w.reshape(1, -1, 1, 1).to(u0)
    return ((w * u0 * u0).sum(1) - 2 * (w * u0 * u1).sum(1) + (w * u1 * u1).sum(1)).flatten(1).mean(1)


def head_grad(f0, f1, w, gout):
    """(d/df0, d/df1) of sum_b gout[b] d[b], closed form: with a = n + eps, e = u0 - u1, q_c = (gout[b] / pixels) 2 w_c e_c,
        d/df0_j =  q_j / a0 - f0_j (sum_c q_c f0_c) / (n0 a0^2),      d/df1_j = -q_j / a1 + f1_j (sum_c q_c f1_c) / (n1 a1^2),
    the second terms 0 where n = 0.  A batch-1 f1 is broadcast; its gradient is then summed over the batch."""
    b = f0.shape[0]
    f1b = f1.expand(b, -1, -1, -1) if f1.shape[0] != b else f1
    (u0, n0), (u1, n1) = unit(f0), unit(f1b)
    a0, a1 = n0 + EPS, n1 + EPS
    pixels = f0.shape[2] * f0.shape[3]
    q = (gout.reshape(-1, 1, 1, 1).to(f0) / pixels) * 2 * w.reshape(1, -1, 1, 1).to(f0) * (u0 - u1)

    def second(f, n, a):
        s = (q * f).sum(1, keepdim=True)
        return torch.where(n > 0, f * s / (n * a * a).clamp_min(1e-300), torch.zeros_like(f))

    g0 = q / a0 - second(f0, n0, a0)
    g1 = -q / a1 + second(f1b, n1, a1)
    if f1.shape[0] != b:
        g1 = g1.sum(0, keepdim=True)
    return g0, g1


def scaling(x):
    shift = torch.tensor(SHIFT, dtype=x.dtype).reshape(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=x.dtype).reshape(1, 3, 1, 1)
    return (x - shift) / scale


def _slice_of(i):
    return next(k for k, r in enumerate(SLICES) if i in r) + 1


def taps(sd, x, route=None, collect=None):
    """[relu1_2, relu2_2, relu3_3, relu4_3, relu5_3] of scaling(x), from an LPIPS state_dict (`net.slice{k}.{i}.*`).
    `route`: {conv index: a post-ReLU activation of that conv} from another evaluation; the discrete decisions are then taken from it
    (each ReLU's mask from the signs of its activation, each pool's window arg-max from the activation in front of it) while every
    value stays this evaluation's -- as test_perceptual_host.ref_vgg does.  `collect`: a dict that receives every activation."""
    route = route or {}
    h, outs = scaling(x), []
    for k, r in enumerate(SLICES):
        for i in r:
            if i in POOLS:
                if i - 2 in route:
                    _, idx = F.max_pool2d(route[i - 2].to(h), 2, 2, return_indices=True)
                    h = h.flatten(2).gather(2, idx.flatten(2)).reshape(idx.shape)
                else:
                    h = F.max_pool2d(h, 2, 2)
            elif i in CONVS:
                name = f"net.slice{k + 1}.{i}"
                pre = F.conv2d(h, sd[name + ".weight"].to(x), sd[name + ".bias"].to(x), padding=1)
                h = pre * (route[i].to(h) > 0).to(h) if i in route else F.relu(pre)
                if collect is not None:
                    collect[i] = h.detach()
        outs.append(h)
    return outs


def lpips(sd, in0, in1, route=None):
    """(distance [B], [five terms [B]]) of in0 [B,3,H,W] against in1 [B or 1,3,H,W], both in [-1, 1].  `route` covers the merged
    batch [in0; in1], as the module computes it."""
    b0 = in0.shape[0]
    t = taps(sd, torch.cat([in0, in1]), route)
    terms = [head(f[:b0], f[b0:], sd[f"lin{k}.model.1.weight"]) for k, f in enumerate(t)]
    return sum(terms), terms


def inputs(shape):
    """The seeded image pair (in0, in1) of `shape`, in [-1, 1]: the inputs of the whole-module tests, here so that the host test
    can make its statement about exactly them."""
    import seeded
    return (torch.tanh(seeded.tensor(f"lpips.in0{tuple(shape)}", shape, 0.8)), torch.tanh(seeded.tensor(f"lpips.in1{tuple(shape)}", shape, 0.8)))


def zero_norm_pixels(sd, x):
    """Per tap, the number of pixels of scaling(x)'s features whose vector is all zero."""
    return [int((f.abs().sum(1) == 0).sum()) for f in taps(sd, x)]
