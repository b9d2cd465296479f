"""The style branch of the region-attention net on HIP (csrc/region_style.hip, region_style_hip.py).

(a) Every entry point on its own, through the C ABI, element by element against tests/region_style_ref.py (float64, CPU):
    |got - ref| <= (K + 8) * 2^-24 * sum|terms|, K the contraction length of that product (k0 + k1 forward, n for the input gradient, B
    for the weight gradient, d for the norm; 1 for the element-wise finish).  Outputs are pre-filled with NaN between sentinels that
    must survive.  Inputs: heavy-tailed operands (normal^3), layer outputs of both signs with one in eight exactly 0, biases of order 1;
    a group's first source sits inside wider rows (the codes are read in place out of [B, 1, E + d] rows).  CASES are the smallest
    shapes at which the tiling can go wrong.  `-s` prints the worst ratio of every check.
(b) The node against the float64 composition (outputs 1e-4, gradients 1e-3: helpers), bit-identical runs in both library modes.
(c) The zero-diff code.  (d) The launch census.  (e) `applies` on the GPU, and W2E_RSTYLE_STOCK."""
import ctypes

import pytest
import torch

import region_style_ref as R
import seeded
from helpers import assert_close, assert_grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENTINEL = 64, 1e30
T = 512
TINY_E = 32  # make_golden.CLIP_TINY's embed_dim (asserted below)

# name -> (batch, code widths, E)
CASES = {
    "b1_narrow": (1, [32], 512),                       # one row, the narrowest code, k = 32 + 512
    "b3_mixed": (3, [512, 256, 128, 64, 32], 512),     # mixed widths in one launch
    "b2_tiny_clip": (2, [512, 32], TINY_E),            # ragged text hidden width: H = 272
    "b2_odd": (2, [32, 64], 30),                       # E = 30: H = 271, sources 8-byte aligned only -- the one-float-per-lane kernels
    "b16_two": (16, [512, 64], 512),                   # the maximum batch
    "b1_all26": (1, R.WIDTHS_1024, 512),               # every code of a 1024^2 generator (attention_layer = 26)
}


def _specs(name):
    """Per case the branch's three forward launches as lists of groups (k0, k1, n, act, pad0, shared): pad0 = floats in front of source
    0 in its rows (x_c and x_text live inside [B, E + d] rows), shared = every group with the same key reads ONE tensor."""
    if name == "b5_shared":  # a shared source and a two-source group in one launch, each once
        return 5, {"mixed": [(48, 0, 40, 1, 8, "s"), (48, 0, 24, 0, 8, "s"), (40, 24, 36, 1, 0, None)]}
    batch, dims, e = CASES[name]
    h = (e + 512) // 2
    first = [(d, 0, d, 0, e, None) for d in dims] + [(e, 0, h, 1, 0, "text") for _ in dims]
    return batch, {"mapper+text0": first[:32], "text1": [(h, 0, T, 1, 0, None) for _ in dims], "all": [(d, T, d, 0, 0, None) for d in dims]}


LAUNCHES = [(n, ln) for n in list(CASES) + ["b5_shared"] for ln in _specs(n)[1]]


def _guarded(shape, fill=float("nan")):
    n = int(torch.Size(shape).numel())
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.float32)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return buf, view


def _intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def _worst(got, ref, terms, k, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: an output element was not written"
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = ((got - ref).abs() / (R.gamma(k) * terms).clamp_min(1e-300)).max().item()
    print(f"{what}: worst |err| / ((K + 8) 2^-24 sum|terms|) = {ratio:.4f}  (K = {k})")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} x the bound"


def _pa(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ia(v):
    return (ctypes.c_int * len(v))(*v)


def _fa(v):
    return (ctypes.c_float * len(v))(*v)


@pytest.fixture(scope="module")
def launches():
    """Per (case, launch): CPU operands, device copies and float64 references -- made once, read-only."""
    made = {}

    def make(name, launch):
        if (name, launch) in made:
            return made[name, launch]
        batch, by_launch = _specs(name)
        specs = by_launch[launch]
        key = f"rsk.{name}.{launch}"
        shared, groups = {}, []
        for i, (k0, k1, n, on, pad0, sh) in enumerate(specs):
            if sh is None or sh not in shared:
                rows = R.heavy(f"{key}.a{i}", (batch, pad0 + k0))
                if sh is not None:
                    shared[sh] = rows
            else:
                rows = shared[sh]
            g = dict(k0=k0, k1=k1, n=n, act=on, pad0=pad0, rows0=rows, src0=rows[:, pad0:],
                     src1=R.heavy(f"{key}.a1_{i}", (batch, k1)) if k1 else None,
                     w=R.heavy(f"{key}.w{i}", (n, k0 + k1)), bias=seeded.tensor(f"{key}.b{i}", (n,), 0.5, 1.0),
                     gy=R.heavy(f"{key}.gy{i}", (batch, n)), y=R.layer_output(f"{key}.y{i}", (batch, n)), w_scale=1.0 / (k0 + k1) ** 0.5)
            srcs = [g["src0"]] + ([g["src1"]] if k1 else [])
            g["fwd"] = R.linear_fwd(srcs, g["w"], g["bias"], g["w_scale"], 1.0, on)
            gp = R.gpre(g["gy"], g["y"], on)
            g["dgrad"] = R.linear_dgrad(gp, g["w"], g["w_scale"])
            g["wgrad"] = R.linear_wgrad(gp, srcs, g["w_scale"], 0.5)
            groups.append(g)
        dev = {}
        for i, g in enumerate(groups):
            for f in ("rows0", "src1", "w", "bias", "gy", "y"):
                t = g[f]
                if t is not None:
                    if id(t) not in dev:
                        dev[id(t)] = t.to(DEV)
                    g["d_" + f] = dev[id(t)]
                else:
                    g["d_" + f] = None
        made[name, launch] = (batch, groups)
        return made[name, launch]

    return make


def _src_args(groups):
    src0 = (ctypes.c_void_p * len(groups))(*[g["d_rows0"].data_ptr() + 4 * g["pad0"] for g in groups])
    return (src0, _pa([g["d_src1"] for g in groups]), _ia([g["k0"] for g in groups]), _ia([g["k1"] for g in groups]),
            _ia([g["pad0"] + g["k0"] for g in groups]), _ia([g["k1"] for g in groups]))


def test_clip_tiny_embed_dim():
    from make_golden import CLIP_TINY
    assert CLIP_TINY["embed_dim"] == TINY_E


@pytest.mark.parametrize("name,launch", LAUNCHES)
def test_linear_forward_matches_float64(launches, name, launch):
    from where2edit_amd._lib import call, stream_ptr
    batch, groups = launches(name, launch)
    outs = [_guarded((batch, g["n"])) for g in groups]
    src0, src1, k0, k1, ld0, ld1 = _src_args(groups)
    call("w2e_rstyle_linear_fwd", len(groups), batch, src0, src1, k0, k1, ld0, ld1, _pa([g["d_w"] for g in groups]),
         _pa([g["d_bias"] for g in groups]), _pa([o[1] for o in outs]), _ia([g["n"] for g in groups]), _fa([g["w_scale"] for g in groups]), 1.0,
         _ia([g["act"] for g in groups]), stream_ptr())
    torch.cuda.synchronize()
    for i, (g, (buf, out)) in enumerate(zip(groups, outs)):
        assert _intact(buf), f"group {i}: wrote outside its output"
        _worst(out, *g["fwd"], g["k0"] + g["k1"], f"{name}/{launch} forward, group {i} ({g['k0']}+{g['k1']} -> {g['n']})")


@pytest.mark.parametrize("name,launch", LAUNCHES)
def test_linear_input_gradient_matches_float64(launches, name, launch):
    from where2edit_amd._lib import call, stream_ptr
    batch, groups = launches(name, launch)
    # a two-source group of the shared-source case asks for its second source only (a gradient nobody needs is not computed)
    skip0 = [name == "b5_shared" and g["k1"] > 0 for g in groups]
    gx0 = [None if s else _guarded((batch, g["k0"])) for g, s in zip(groups, skip0)]
    gx1 = [_guarded((batch, g["k1"])) if g["k1"] else None for g in groups]
    call("w2e_rstyle_linear_dgrad", len(groups), batch, _pa([g["d_gy"] for g in groups]), _pa([g["d_y"] for g in groups]),
         _pa([g["d_w"] for g in groups]), _pa([None if o is None else o[1] for o in gx0]), _pa([None if o is None else o[1] for o in gx1]),
         _ia([g["k0"] for g in groups]), _ia([g["k1"] for g in groups]), _ia([g["n"] for g in groups]), _fa([g["w_scale"] for g in groups]),
         _ia([g["act"] for g in groups]), stream_ptr())
    torch.cuda.synchronize()
    for i, g in enumerate(groups):
        ref, terms = g["dgrad"]
        for o, lo, hi, which in ((gx0[i], 0, g["k0"], "source 0"), (gx1[i], g["k0"], g["k0"] + g["k1"], "source 1")):
            if o is None:
                continue
            assert _intact(o[0]), f"group {i} {which}: wrote outside its output"
            _worst(o[1], ref[:, lo:hi], terms[:, lo:hi], g["n"], f"{name}/{launch} input gradient, group {i} {which}")


@pytest.mark.parametrize("name,launch", LAUNCHES)
def test_linear_weight_gradient_matches_float64(launches, name, launch):
    from where2edit_amd._lib import call, stream_ptr
    batch, groups = launches(name, launch)
    gw = [_guarded((g["n"], g["k0"] + g["k1"])) for g in groups]
    gb = [_guarded((g["n"],)) for g in groups]
    src0, src1, k0, k1, ld0, ld1 = _src_args(groups)
    call("w2e_rstyle_linear_wgrad", len(groups), batch, _pa([g["d_gy"] for g in groups]), _pa([g["d_y"] for g in groups]), src0, src1, k0, k1,
         ld0, ld1, _pa([o[1] for o in gw]), _pa([o[1] for o in gb]), _ia([g["n"] for g in groups]), _fa([g["w_scale"] for g in groups]), 0.5,
         _ia([g["act"] for g in groups]), stream_ptr())
    torch.cuda.synchronize()
    for i, g in enumerate(groups):
        rw, tw, rb, tb = g["wgrad"]
        assert _intact(gw[i][0]) and _intact(gb[i][0]), f"group {i}: wrote outside its output"
        _worst(gw[i][1], rw, tw, batch, f"{name}/{launch} weight gradient, group {i}")
        _worst(gb[i][1], rb, tb, batch, f"{name}/{launch} bias gradient, group {i}")


@pytest.mark.parametrize("name", list(CASES))
def test_finish_matches_float64(name):
    from where2edit_amd._lib import call, ptr, stream_ptr
    batch, dims, e = CASES[name]
    g, layers, alpha = len(dims), len(dims) + 2, 0.1
    rows = [R.heavy(f"rsk.{name}.fin.x{c}", (batch, e + d)) for c, d in enumerate(dims)]
    xs = [r[:, e:] for r in rows]
    ys = [R.layer_output(f"rsk.{name}.fin.y{c}", (batch, d)) for c, d in enumerate(dims)]
    ys[-1][0] = xs[-1][0]  # a row whose code comes back unchanged: norm 0
    fin = R.finish_fwd(xs, ys, alpha, layers)
    d_rows, d_y = [r.to(DEV) for r in rows], [y.to(DEV) for y in ys]
    xp = (ctypes.c_void_p * g)(*[r.data_ptr() + 4 * e for r in d_rows])
    ldx = _ia([e + d for d in dims])
    outs = [_guarded((batch, d)) for d in dims]
    nbuf, norms = _guarded((g, batch))
    lbuf, loss = _guarded((1,))
    call("w2e_rstyle_finish_fwd", g, batch, xp, ldx, _pa(d_y), _pa([o[1] for o in outs]), _ia(dims), alpha, layers, ptr(norms), ptr(loss), stream_ptr())
    torch.cuda.synchronize()
    assert _intact(nbuf) and _intact(lbuf) and all(_intact(o[0]) for o in outs)
    for c in range(g):
        _worst(outs[c][1], fin["x_new"][c], fin["x_new_terms"][c], 1, f"{name} x_new {c}")
        _worst(norms[c], fin["norms"][c], fin["norms"][c].clamp_min(1e-300), dims[c], f"{name} norms {c}")
    assert float(norms[-1, 0]) == 0.0
    _worst(loss, fin["loss"].reshape(1), fin["loss"].reshape(1), max(dims) + g * batch, f"{name} loss_delta")
    # backward, on the kernel's own norms
    g_out = [R.heavy(f"rsk.{name}.fin.go{c}", (batch, d)) for c, d in enumerate(dims)]
    g_out[0] = None  # a code nobody uses downstream
    g_loss = torch.tensor([0.7], device=DEV)
    ref, terms = R.finish_bwd(xs, ys, g_out, [norms[c].cpu() for c in range(g)], 0.7, alpha, layers)
    gys = [_guarded((batch, d)) for d in dims]
    d_go = [None if t is None else t.to(DEV) for t in g_out]
    call("w2e_rstyle_finish_bwd", g, batch, xp, ldx, _pa(d_y), _pa(d_go), ptr(norms), ptr(g_loss), _pa([o[1] for o in gys]), _ia(dims), alpha,
         layers, stream_ptr())
    torch.cuda.synchronize()
    for c in range(g):
        assert _intact(gys[c][0])
        _worst(gys[c][1], ref[c], terms[c].clamp_min(1e-300), 1, f"{name} finish backward {c}")


# ---- (b) the node ------------------------------------------------------------------------------------------------------------------
def _node_case(name, zero_diff=False):
    batch, dims, e = CASES[name] if not zero_diff else (1, [64, 32], TINY_E)
    params = R.make_params("rsnode." + name, dims, e)
    x = R.make_inputs("rsnode." + name, batch, dims, e, extra=1)
    if zero_diff:  # mapper_all_0: zero weight, bias = the code
        w, _ = params["all"][0]
        params["all"][0] = (torch.zeros_like(w), x[0][0, 0, e:].clone())
    layers = len(dims)
    net = R.style_net(params, dims, e, layers, DEV)
    return params, x, net, dims, e, layers


def _run(net, x, e, alpha=0.1):
    net.zero_grad(set_to_none=True)
    xd = [t.to(DEV) for t in x]
    out, loss = net.new_styles(xd, xd[0][:, 0, :e], alpha)
    probes = R.probe([o[..., 0, 0] for o in out[:len(out) - 1]])
    (sum((o[..., 0, 0] * p.to(DEV)).sum() for o, p in zip(out, probes)) + 0.7 * loss).backward()
    torch.cuda.synchronize()
    return out, loss


def _families(net, g):
    return {"mapper": [getattr(net, f"mapper_{c}") for c in range(g)], "text0": [getattr(net, f"mapper_text_{c}")[0] for c in range(g)],
            "text1": [getattr(net, f"mapper_text_{c}")[1] for c in range(g)], "all": [getattr(net, f"mapper_all_{c}") for c in range(g)]}


@pytest.fixture
def w2e_calls(monkeypatch):
    """The names of the entry points that go through _lib.call."""
    from where2edit_amd import _lib
    seen, real = [], _lib.call

    def logging(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", logging)
    return seen


@pytest.mark.parametrize("name", ["b3_mixed", "b2_tiny_clip"])
def test_node_matches_the_float64_composition(w2e_calls, w2e_opt, name):
    params, x, net, dims, e, layers = _node_case(name)
    ref_out, ref_loss, ref_grads = R.branch(params, x, 0.1, layers, e)
    out, loss = _run(net, x, e)
    assert any(n.startswith("w2e_rstyle_") for n in w2e_calls), "the node was not taken"
    assert len(out) == len(dims) + 1 and torch.equal(out[-1][..., 0, 0].cpu(), x[-1][:, :, e:])
    for c, d in enumerate(dims):
        assert tuple(out[c].shape) == (x[0].shape[0], 1, d, 1, 1)
        assert_close(out[c][..., 0, 0], ref_out[c], 1e-4, f"{name} new code {c}")
    assert loss.dim() == 0
    assert_close(loss, ref_loss, 1e-4, f"{name} loss_delta")
    fams = _families(net, len(dims))
    for f in R.FAMILIES:
        for c, m in enumerate(fams[f]):
            assert_grad_close(m.weight.grad, ref_grads[f][c][0], f"region style {name}: {f} weight {c}")
            assert_grad_close(m.bias.grad, ref_grads[f][c][1], f"region style {name}: {f} bias {c}")
    assert all(p.grad is None for n, p in net.named_parameters() if "textca" in n)
    # two runs, bit for bit, in both library modes
    for det in ("0", "1"):
        w2e_opt("deterministic", det)
        runs = []
        for _ in range(2):
            o, l = _run(net, x, e)
            runs.append([t.detach().clone() for t in o] + [l.detach().clone()] + [p.grad.clone() for p in net.parameters() if p.grad is not None])
        assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs)), f"deterministic = {det}: two runs differ"


def test_forward_alone_runs_without_grad_and_in_eval():
    params, x, net, dims, e, layers = _node_case("b2_tiny_clip")
    ref_out, ref_loss, _ = R.branch(params, x, 0.25, layers, e)
    net.eval()
    with torch.no_grad():
        xd = [t.to(DEV) for t in x]
        out, loss = net.new_styles(xd, xd[0][:, 0, :e], 0.25)
    assert not loss.requires_grad and not out[0].requires_grad
    for c in range(len(dims)):
        assert_close(out[c][..., 0, 0], ref_out[c], 1e-4, f"new code {c} (no_grad, eval, alpha 0.25)")
    assert_close(loss, ref_loss, 1e-4, "loss_delta (no_grad, eval)")


# ---- (c) the zero-diff code --------------------------------------------------------------------------------------------------------
def test_zero_diff_code_gives_finite_gradients_equal_to_the_stock_compositions():
    params, x, net, dims, e, layers = _node_case("zero", zero_diff=True)
    _, ref_loss, ref_grads = R.stock_composition(params, x[:len(dims)], 0.1, layers, e)
    out, loss = _run(net, x, e)
    assert torch.equal(out[0][..., 0, 0].cpu(), x[0][:, :, e:]), "code 0 must come back unchanged"
    assert_close(loss, ref_loss, 1e-4, "loss_delta")
    fams = _families(net, len(dims))
    for f in R.FAMILIES:
        for c, m in enumerate(fams[f]):
            for got, ref, what in ((m.weight.grad, ref_grads[f][c][0], "weight"), (m.bias.grad, ref_grads[f][c][1], "bias")):
                assert torch.isfinite(got).all(), f"{f} {what} {c}: the gradient is not finite"
                if ref.abs().max() == 0:  # (mapper_0 sits behind mapper_all_0's zero weight: exactly 0, which has no direction to compare)
                    assert torch.equal(got.cpu(), torch.zeros_like(got.cpu())), f"{f} {what} {c}: expected exactly 0"
                else:
                    assert_grad_close(got, ref, f"region style zero-diff: {f} {what} {c}")


# ---- (d) the launch census ---------------------------------------------------------------------------------------------------------
def test_one_forward_and_backward_is_at_most_13_calls_and_no_gemm(w2e_calls):
    from torch.profiler import ProfilerActivity, profile
    params, x, net, dims, e, layers = _node_case("b3_mixed")
    _run(net, x, e)  # (library load, first-use work)
    del w2e_calls[:]
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        _run(net, x, e)
    print("w2e calls of one forward + backward:", w2e_calls)
    assert 0 < len(w2e_calls) <= 13 and all(n.startswith("w2e_rstyle_") for n in w2e_calls)
    assert sum(n in ("w2e_rstyle_linear_fwd", "w2e_rstyle_finish_fwd") for n in w2e_calls) <= 5
    assert sum(n in ("w2e_rstyle_linear_dgrad", "w2e_rstyle_linear_wgrad", "w2e_rstyle_finish_bwd") for n in w2e_calls) <= 8
    gemm = {"aten::mm", "aten::addmm", "aten::bmm", "aten::baddbmm", "aten::matmul", "aten::linear"}
    ran = {ev.key for ev in prof.key_averages()}
    assert not (ran & gemm), f"stock GEMMs ran: {sorted(ran & gemm)}"


# ---- (e) applies on the GPU, the stock switch ---------------------------------------------------------------------------------------
def test_applies_on_the_gpu_and_the_stock_fallback(w2e_calls, monkeypatch):
    from where2edit_amd import region_style_hip as RS
    params, x, net, dims, e, layers = _node_case("b2_tiny_clip")
    xd = [t.to(DEV) for t in x]
    xt = xd[0][:, 0, :e]
    assert RS.applies(net, xd, xt) is not None
    assert RS.applies(net, x, x[0][:, 0, :e]) is None, "CPU tensors"
    assert RS.applies(net, [t.repeat(9, 1, 1)[:17].contiguous() for t in xd], xt.repeat(9, 1)[:17]) is None, "B = 17"
    d33 = [32] * 33
    n33 = R.style_net(R.make_params("rsnode.33", d33, e), d33, e, 33, DEV)
    x33 = [t.to(DEV) for t in R.make_inputs("rsnode.33", 1, d33, e)]
    assert RS.applies(n33, x33, x33[0][:, 0, :e]) is None, "33 codes"
    assert RS.applies(n33, x33[:32], x33[0][:, 0, :e]) is not None, "32 codes are taken (mapper_layer counts only the codes passed)"
    assert RS.applies(net, [t.clone().requires_grad_() for t in xd], xt) is None, "an input that requires grad"
    assert RS.applies(net, [t.double() for t in xd], xt.double()) is None, "float64"
    assert RS.applies(net, [torch.cat([t, t], -1)[:, :, :t.shape[-1]] for t in xd], xt) is None, "non-contiguous codes"
    foreign = R.style_net(params, dims, e, layers, DEV)
    foreign.mapper_all_1.activation = "fused_lrelu"
    assert RS.applies(foreign, xd, xt) is None, "a module with a foreign structure"
    # the stock composition on the GPU: through the switch (no style kernel is called), equal to the node's result
    out, loss = _run(net, x, e)
    grads = [p.grad.clone() for p in net.parameters() if p.grad is not None]
    del w2e_calls[:]
    monkeypatch.setenv("W2E_RSTYLE_STOCK", "1")
    out_s, loss_s = _run(net, x, e)
    assert not any(n.startswith("w2e_rstyle_") for n in w2e_calls), "W2E_RSTYLE_STOCK=1 was not honoured"
    for c, (a, b) in enumerate(zip(out, out_s)):
        assert a.shape == b.shape
        assert_close(a, b, 1e-5, f"node vs stock: new code {c}")
    assert loss.shape == loss_s.shape
    assert_close(loss, loss_s, 1e-5, "node vs stock: loss_delta")
    for a, b in zip(grads, [p.grad for p in net.parameters() if p.grad is not None]):
        assert_grad_close(a, b, "region style: node vs stock gradient")
