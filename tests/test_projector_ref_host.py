"""tests/projector_ref.py (the float64 restatement the GPU tests of the projector are judged against) held to autograd and to the
package's own host arithmetic, and the host side of where2edit_amd.projector: no GPU needed."""
import os

import pytest
import torch

import projector_ref as R


def _white(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _smooth(shape, seed):
    """A correlated map: white noise box-filtered twice along both axes (wrapping), unit variance."""
    n = _white(shape, seed)
    for _ in range(2):
        n = n + torch.roll(n, 1, 2) + torch.roll(n, 1, 3) + torch.roll(n, (1, 1), (2, 3))
    return n / n.std()


@pytest.mark.parametrize("shape", [(1, 1, 4, 4), (1, 1, 8, 8), (1, 1, 16, 16), (2, 1, 32, 32), (1, 1, 64, 64)], ids=str)
@pytest.mark.parametrize("kind", ["white", "smooth"])
def test_closed_form_gradient_is_autograds(shape, kind):
    n = (_white if kind == "white" else _smooth)(shape, 11).requires_grad_(True)
    (g,) = torch.autograd.grad(R.noise_regularize([n]), n)
    closed = R.noise_regularize_grad(n.detach())
    assert torch.allclose(closed, g, rtol=1e-12, atol=1e-18 + 1e-12 * float(g.abs().max()))
    # one level on its own too
    m = n.detach().clone().requires_grad_(True)
    m3, m2 = R.level_means(m)
    (g1,) = torch.autograd.grad(m3.pow(2) + m2.pow(2), m)
    assert torch.allclose(R.level_grad(m.detach()), g1, rtol=1e-12, atol=1e-12 * float(g1.abs().max()))
    # the term scales bound the values they belong to
    value_scale, grad_scale = R.noise_regularize_scales(n.detach())
    assert float(R.noise_regularize([n.detach()])) <= float(value_scale)
    assert bool((closed.abs() <= grad_scale * (1 + 1e-12)).all())


def test_levels_count():
    assert [len(R.levels(torch.zeros(1, 1, s, s))) for s in (4, 8, 16, 32, 256, 1024)] == [1, 1, 2, 3, 6, 8]


def test_get_lr_is_the_packages():
    from where2edit_amd.run_attention import get_lr
    for steps in (7, 30, 1000):
        for i in range(steps):
            t = i / steps
            assert R.get_lr(t, 0.1, 0.25, 0.05) == get_lr(t, 0.1, 0.25, 0.05)
            assert R.get_lr(t, 0.03, 0.5, 0.1) == get_lr(t, 0.03, 0.5, 0.1)
    assert R.get_lr(0.0, 0.1) == 0.0 and abs(R.get_lr(0.5, 0.1) - 0.1) < 1e-15


def test_white_is_about_zero_and_smooth_is_not():
    white, smooth = _white((1, 1, 256, 256), 3), _smooth((1, 1, 256, 256), 3)
    lw, ls = float(R.noise_regularize([white])), float(R.noise_regularize([smooth]))
    # white: every mean of N products of independent unit normals is ~ N(0, 1/N); six levels, two means each, the coarsest (8^2) dominating
    assert lw < 12 * 3.0 ** 2 / 64
    assert ls > 0.25 and ls > 20 * lw  # neighbours correlated > 0.5 at level 0 alone: (0.5)^2
    assert float(R.noise_strength(0.0, 2.0)) == 2.0 * 0.05 and R.noise_strength(0.75, 2.0) == 0 and R.noise_strength(0.9, 2.0) == 0


def test_latent_std_and_normalize():
    w = _white((1000, 8), 5) * 3 + 1
    assert abs(float(R.latent_std(w)) - float(((w - w.mean(0)) ** 2).sum().div(1000).sqrt())) < 1e-12
    n = R.noise_normalize(_white((2, 1, 16, 16), 6) * 4 - 3)
    assert abs(float(n.mean())) < 1e-12 and abs(float(n.std()) - 1) < 1e-12


def test_front_reference():
    img, target = _white((2, 3, 8, 8), 7), _white((2, 3, 4, 4), 8)
    small, mse = R.front(img, target, 2)
    assert torch.allclose(small, torch.nn.functional.avg_pool2d(img, 2), rtol=1e-13, atol=1e-15)
    assert abs(float(mse) - float(torch.nn.functional.mse_loss(small, target))) < 1e-15
    assert R.front(img, img, 1)[0] is img


def test_save_projection_round_trips(tmp_path):
    from where2edit_amd.projector import Projection, save_projection
    g = torch.Generator().manual_seed(1)
    res = Projection(torch.randn(2, 6, 512, generator=g), [torch.randn(2, 1, 4, 4, generator=g), torch.randn(2, 1, 8, 8, generator=g)],
                     torch.randn(2, 3, 16, 16, generator=g), torch.zeros(3), torch.zeros(3))
    path = os.path.join(tmp_path, "proj.pt")
    out = save_projection(path, res, ["a.png", "b.png"])
    back = torch.load(path)
    assert list(back) == ["a.png", "b.png"] == list(out)
    for i, name in enumerate(back):
        assert set(back[name]) == {"img", "latent", "noise"}
        assert torch.equal(back[name]["img"], res.img[i]) and torch.equal(back[name]["latent"], res.latent[i])
        assert [tuple(n.shape) for n in back[name]["noise"]] == [(1, 1, 4, 4), (1, 1, 8, 8)]
        assert all(torch.equal(n, m[i:i + 1]) for n, m in zip(back[name]["noise"], res.noises))
    shared = Projection(res.latent[:1], [n[:1] for n in res.noises], res.img[:1], res.loss, res.mse)
    one = save_projection(None, shared, ["a.png"])
    assert all(torch.equal(n, m) for n, m in zip(one["a.png"]["noise"], shared.noises))
    with pytest.raises(ValueError):
        save_projection(None, res, ["only one"])
    with pytest.raises(ValueError):
        save_projection(None, res, ["same", "same"])


def test_project_refuses_cpu_tensors_loudly():
    import where2edit_amd
    from where2edit_amd.stylegan2 import Generator
    g = Generator(16, 512, 2).requires_grad_(False).eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        where2edit_amd.project(g, torch.zeros(1, 3, 16, 16), steps=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        where2edit_amd.noise_regularize([torch.zeros(1, 1, 8, 8)])
    with pytest.raises(RuntimeError, match="GPU only"):
        where2edit_amd.noise_normalize_([torch.zeros(1, 1, 8, 8)])
    with pytest.raises(RuntimeError, match="GPU only"):
        where2edit_amd.loss_front(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 8, 8))
    with pytest.raises(TypeError):
        where2edit_amd.project(torch.nn.Linear(2, 2), torch.zeros(1, 3, 16, 16))
