"""The projector's arithmetic (include/w2e_projector.h, where2edit_amd/projector.py) restated with the literal torch expressions of
rosinality's projector.py, in the dtype of the inputs (float64 in the tests); autograd gives the gradients.  Beside each formula its
term scale: the same formula on absolute values, which the GPU tests judge every element against.  Own code, test-only."""
import math

import torch


def get_lr(t, initial_lr, rampdown=0.25, rampup=0.05):
    lr_ramp = min(1, (1 - t) / rampdown)
    lr_ramp = 0.5 - 0.5 * math.cos(lr_ramp * math.pi)
    lr_ramp = lr_ramp * min(1, t / rampup)
    return initial_lr * lr_ramp


def latent_std(w):
    """((w - mean)^2).sum() / n) ** 0.5 over n = w.shape[0] samples: one number."""
    mean = w.mean(0)
    return ((w - mean).pow(2).sum() / w.shape[0]) ** 0.5


def noise_strength(t, std, noise=0.05, noise_ramp=0.75):
    return std * noise * max(0, 1 - t / noise_ramp) ** 2


def levels(n):
    """[n, its 2x2 box mean, ...] while the side is above 8: the maps the regulariser looks at."""
    out, size = [n], n.shape[2]
    while size > 8:
        n = n.reshape([-1, 1, size // 2, 2, size // 2, 2]).mean([3, 5])
        size //= 2
        out.append(n)
    return out


def level_means(n):
    """(mean(n * roll(n, 1, dim 3)), mean(n * roll(n, 1, dim 2)))."""
    return (n * torch.roll(n, shifts=1, dims=3)).mean(), (n * torch.roll(n, shifts=1, dims=2)).mean()


def noise_regularize(noises):
    loss = 0
    for noise in noises:
        for n in levels(noise):
            m3, m2 = level_means(n)
            loss = loss + m3.pow(2) + m2.pow(2)
    return loss


def level_grad(n):
    """d/dn of mean(n roll(n,1,3))^2 + mean(n roll(n,1,2))^2 at ONE level, closed form: 2 m / N times the two neighbours of each
    product."""
    m3, m2 = level_means(n)
    N = n.numel()
    return 2 * m3 / N * (torch.roll(n, 1, 3) + torch.roll(n, -1, 3)) + 2 * m2 / N * (torch.roll(n, 1, 2) + torch.roll(n, -1, 2))


def noise_regularize_grad(noise):
    """The gradient of noise_regularize([noise]) in closed form: every level's own gradient plus a quarter of the coarser level's."""
    lv = levels(noise)
    g = None
    for n in reversed(lv):
        own = level_grad(n)
        if g is not None:
            own = own + 0.25 * g.repeat_interleave(2, 2).repeat_interleave(2, 3)
        g = own
    return g


def noise_regularize_scales(noise):
    """(scale of the value, scale of every gradient element) of ONE map: the sums above on absolute values -- the mean of |products| A in
    place of the cancelled mean m, on the pyramid of |n|."""
    a = noise.abs()
    value, g = 0.0, None
    for n in reversed(levels(a)):
        a3, a2 = level_means(n)
        value = value + 2 * (a3 * a3 + a2 * a2)
        N = n.numel()
        own = 2 * a3 / N * (torch.roll(n, 1, 3) + torch.roll(n, -1, 3)) + 2 * a2 / N * (torch.roll(n, 1, 2) + torch.roll(n, -1, 2))
        if g is not None:
            own = own + 0.25 * g.repeat_interleave(2, 2).repeat_interleave(2, 3)
        g = own
    return value, g


def noise_normalize(noise):
    return (noise - noise.mean()) / noise.std()


def front(img, target, f):
    """(small, mse): the f x f box mean and F.mse_loss(small, target)."""
    b, c, h, w = img.shape
    small = img.reshape(b, c, h // f, f, w // f, f).mean([3, 5]) if f > 1 else img
    return small, (small - target).pow(2).mean()


def noise_grad(gpre, noise_w):
    """gpre [planes, pixels] -> noise_w * the plane sum, and its term scale."""
    return noise_w * gpre.sum(0), abs(noise_w) * gpre.abs().sum(0)
