"""tests/mapper_ref.py held to something independent of the kernels it is the reference of (CPU, float64): composed layer by layer its
pieces reproduce oracle/mappers.py's output (1e-12) and float64 autograd's gradient of every weight and bias through the oracle (1e-10)
for LevelsMapper with three levels and with the medium level disabled, SingleMapper, and the two style-space mappers; the layouts are
inverses of each other; every `*_scale` twin is >= |ref|; the slope branch is y > 0."""
import math

import pytest
import torch

import mapper_ref as R
import seeded
from oracle import mappers as OM

OUT_TOL, GRAD_TOL = 1e-12, 1e-10  # float64 against float64: sums of at most 1152 terms of O(1)
LR_MUL = 0.01
N_LATENT = 18
LEVEL_NAMES = {0: "course_mapping.", 4: "medium_mapping.", 8: "fine_mapping."}


def close(a, b, tol, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    a, b = a.detach(), b.detach()
    err = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert err <= tol, f"{what}: {err:.3e}"


def _state(prefixes, dims=None, salt=0):
    """seeded.mapper_state_dict in float64, biases of order 30 (they enter times lr_mul), every tensor a leaf that requires grad."""
    sd = seeded.mapper_state_dict(prefixes, dims, salt=salt)
    return {k: (v.double() * (30.0 if k.endswith("bias") else 1.0)).requires_grad_(True) for k, v in sd.items()}


def _layers(sd, prefix):
    return [sd[f"{prefix}mapping.{i}.weight"] for i in range(1, 5)], [sd[f"{prefix}mapping.{i}.bias"] for i in range(1, 5)]


def _check_grads(sd, prefix, gws, gbs, what):
    for j in range(4):
        close(gws[j], sd[f"{prefix}mapping.{j + 1}.weight"].grad, GRAD_TOL, f"{what} {prefix}mapping.{j + 1}.weight")
        close(gbs[j], sd[f"{prefix}mapping.{j + 1}.bias"].grad, GRAD_TOL, f"{what} {prefix}mapping.{j + 1}.bias")


@pytest.mark.parametrize("kind", ["levels", "no_medium", "single"])
def test_level_mappers_equal_the_oracle_and_autograd(kind):
    batch = 3
    levels = {"levels": ((0, 4), (4, 4), (8, 10)), "no_medium": ((0, 4), (8, 10)), "single": ((0, N_LATENT),)}[kind]
    prefixes = ["mapping."] if kind == "single" else [LEVEL_NAMES[l0] for l0, _ in levels]
    sd = _state(prefixes, salt=1)
    x = seeded.tensor(f"mapper_ref.{kind}.x", (batch, N_LATENT, R.D)).double()
    r = seeded.tensor(f"mapper_ref.{kind}.r", (batch, N_LATENT, R.D)).double()
    want = OM.single_mapper(sd, x) if kind == "single" else OM.levels_mapper(sd, x, no_medium=kind == "no_medium")
    (want * r).sum().backward()

    w_scale = LR_MUL / math.sqrt(R.D)
    h0 = R.split_rows(R.levels_pixelnorm(x, levels), batch, levels)
    gout = R.split_rows(R.gather_rows(r, levels), batch, levels)
    outs = []
    for gi, prefix in enumerate(prefixes):
        ws, bs = _layers(sd, prefix)
        h = R.mapper_forward(h0[gi], ws, bs, w_scale, LR_MUL)
        outs.append(h[-1])
        gws, gbs = R.mapper_backward(h, ws, gout[gi], w_scale, LR_MUL)
        _check_grads(sd, prefix, gws, gbs, kind)
    got = R.scatter_rows(torch.cat(outs, 0), batch, N_LATENT, levels)
    close(got, want, OUT_TOL, f"{kind} output")
    if kind == "no_medium":
        assert not got[:, 4:8].any() and not want[:, 4:8].any()
    # the float32 epsilon the kernels add moves nothing at these magnitudes
    close(R.levels_pixelnorm(x, levels), R.levels_pixelnorm(x, levels, eps=1e-8), OUT_TOL, "EPS")


@pytest.mark.parametrize("kind", ["full", "without_torgb"])
def test_stylespace_mappers_equal_the_oracle_and_autograd(kind):
    batch = 2
    dims = OM.STYLESPACE_DIMENSIONS
    torgb = set(range(1, len(dims), 3)) if kind == "without_torgb" else set()
    idx = [c for c in range(len(dims)) if c not in torgb]
    sd = _state([f"mapper_{c}." for c in idx], [dims[c] for c in idx], salt=2)
    xs = [seeded.tensor(f"mapper_ref.{kind}.x{c}", (batch, 1, d, 1, 1)).double() for c, d in enumerate(dims)]
    rs = [seeded.tensor(f"mapper_ref.{kind}.r{c}", (batch, 1, d, 1, 1)).double() for c, d in enumerate(dims)]
    want = (OM.full_stylespace_mapper if kind == "full" else OM.without_torgb_stylespace_mapper)(sd, xs)
    sum((a * b).sum() for a, b in zip(want, rs) if a.requires_grad).backward()

    mdims = [dims[c] for c in idx]
    h0 = R.ss_unpack(R.ss_pixelnorm([xs[c] for c in idx]), batch, mdims)
    gout = R.ss_unpack(R.ss_pack([rs[c].reshape(batch, -1) for c in idx]), batch, mdims)
    for k, c in enumerate(idx):
        ws, bs = _layers(sd, f"mapper_{c}.")
        w_scale = LR_MUL / math.sqrt(dims[c])
        h = R.mapper_forward(h0[k], ws, bs, w_scale, LR_MUL)
        close(h[-1].view(xs[c].shape), want[c], OUT_TOL, f"{kind} output {c}")
        gws, gbs = R.mapper_backward(h, ws, gout[k], w_scale, LR_MUL)
        _check_grads(sd, f"mapper_{c}.", gws, gbs, kind)
    for c in torgb:
        assert not want[c].any()


def test_layouts_are_inverses_and_name_the_rows_the_header_names():
    batch, levels = 3, ((0, 1), (1, 2), (8, 10))
    t = torch.arange(batch * N_LATENT * 2, dtype=torch.float64).view(batch, N_LATENT, 2)
    rows = R.gather_rows(t, levels)
    r0 = 0
    for l0, ln in levels:
        for b in range(batch):
            for l in range(ln):
                assert torch.equal(rows[r0 + b * ln + l], t[b, l0 + l])
        r0 += batch * ln
    back = R.scatter_rows(rows, batch, N_LATENT, levels)
    covered = R.scatter_rows(torch.ones_like(rows), batch, N_LATENT, levels).bool()
    assert torch.equal(back[covered], t[covered]) and not back[~covered].any()
    dims = (1, 3, 5)
    codes = [torch.randn(batch, d, dtype=torch.float64) for d in dims]
    flat = R.ss_pack(codes)
    off = 0
    for c, d in zip(codes, dims):
        assert torch.equal(flat[off:off + batch * d].view(batch, d), c)
        off += batch * d
    assert all(torch.equal(a, b) for a, b in zip(R.ss_unpack(flat, batch, dims), codes))


def test_the_slope_branch_is_y_greater_than_zero():
    y = torch.tensor([1.0, 0.0, -0.0, -1.0, 1e-45])
    gp = R.gpre(torch.ones(5), y)
    assert torch.equal(gp, torch.tensor([1.0, R.SLOPE, R.SLOPE, R.SLOPE, 1.0], dtype=torch.float64) * R.GAIN)


def test_every_scale_twin_covers_its_reference():
    g = torch.Generator().manual_seed(7)
    a, w, bias = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((5, 33), (33, 33), (33,)))
    gy, y = torch.randn(5, 33, generator=g, dtype=torch.float64), torch.randn(5, 33, generator=g, dtype=torch.float64)
    gp = R.gpre(gy, y)

    def covers(scale, ref):
        assert scale.shape == ref.shape and bool((scale >= ref.abs() * (1 - 1e-12)).all())

    for b in (bias, None):
        covers(R.linear_fwd_scale(a, w, b, 0.3, 0.01, 41), R.linear_fwd(a, w, b, 0.3, 0.01))
    covers(R.linear_bwd_scale(gp, w, 0.3), R.linear_bwd(gp, w, 0.3))
    for s, r in zip(R.wgrad_scale(gp, a, 0.3, 0.01), R.wgrad(gp, a, 0.3, 0.01)):
        covers(s, r)
    assert R.EPS == float(torch.tensor(1e-8, dtype=torch.float32)) and R.EPS != 1e-8
