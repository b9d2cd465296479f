"""The opt-in trainable mask branch on the GPU (run_attention.train_mask_branch): w2e_cluster_pool_bwd and w2e_attention_logits_bwd
against float64 restatements (1e-4 in rel_err, the figure the forward tests of this branch use: the fp32 oracle's own mask gradients
sit at most 7.9e-7 from float64 on the seeded problem), the opted-in net against the reference's gradients
(tests/golden/attention_grad.npz) and the float64 oracle, the trainer's `train_mask_from` schedule, reproducibility, graph capture
and cache invalidation.  Every comparison prints its measured error."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import make_golden_attention as M
import mask_train_common as C
import seeded
from helpers import assert_close, assert_grad_close, golden, rel_err
from mask_ref import logits_ref as _logits_ref, nearest_index, pool_ref as _pool_ref
from oracle import attention_net as OA

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
CFG = dict(attention_layer=M.ATT_LAYER, cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS)


def _close(a, b, what):
    e = rel_err(a, b)
    print(f"  {what}: rel err {e:.3e}")
    assert e <= TOL, f"{what}: rel err {e:.3e} > {TOL:.0e}"


# ---------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("size,cs,clusters,batch", [(16, 16, 6, 2), (20, 8, 5, 3), (64, 64, 20, 2), (7, 3, 4, 1), (22, 26, 7, 2), (46, 14, 5, 1),
                                                    (128, 64, 32, 1)])
def test_cluster_pool_bwd_vs_float64(size, cs, clusters, batch):
    """An empty cluster (id clusters-1 is never assigned), out-of-range ids (-1 and K), the reflect borders (r is dense up to the
    edge; size 7 folds every tap), `size` not a multiple of the cluster resolution (20 / 8, 7 / 3), means on both sides of 0.7 and
    0.8; 26 -> 22 and 14 -> 46, where torch's nearest resize (the reference's gather, mask_ref.nearest_index) and floor(dst * in / out)
    read different pixels; size 128, the 128 KB LDS opt-in."""
    from where2edit_amd.run_attention import _ClusterPoolTrain
    rs = np.random.RandomState(size * 100 + cs)
    assign = torch.from_numpy(rs.randint(0, clusters - 1, size=(batch, cs, cs)).astype(np.int32))
    assign[0, 0, 0], assign[-1, cs - 1, cs - 2] = -1, clusters
    level = torch.tensor([0.75, 0.55, 0.85, 0.65, 0.95])[assign.long().clamp(0, clusters - 1) % 5]
    idx = nearest_index(cs, size)
    each = (level[:, idx][:, :, idx] + 0.04 * seeded.tensor(f"pool.each{size}", (batch, size, size))).clamp(0.01, 0.99)
    r = seeded.tensor(f"pool.r{size}", (batch, 1, size, size))
    e64 = each.double().requires_grad_(True)
    final_o, reg_o, tv_o, same_o = _pool_ref(e64, assign, size, clusters)
    (g_o,) = torch.autograd.grad((final_o * r.double()).sum() + 2.0 * reg_o.sum() + 5.0 * tv_o, e64)
    choice = assign.long()[:, idx][:, :, idx]
    means = [float(same_o.detach()[b][choice[b] == k].mean()) for b in range(batch) for k in range(clusters - 1) if (choice[b] == k).any()]
    assert min(means) < 0.7 < max(means) and min(abs(m - 0.7) for m in means) > 1e-3
    eg = each.to(DEV).requires_grad_(True)
    final, reg, tv, same, _, counts, _ = _ClusterPoolTrain.apply(eg, assign.to(DEV), size, clusters)
    assert (counts[:, clusters - 1] == 0).all()  # the empty cluster
    print(f"cluster_pool_bwd size {size} cs {cs} K {clusters} B {batch}")
    _close(final, final_o, "final"), _close(same, same_o, "same"), _close(reg, reg_o, "loss_reg"), _close(tv.reshape(1), tv_o.reshape(1), "loss_tv")
    (g,) = torch.autograd.grad((final * r.to(DEV)).sum() + 2.0 * reg.sum() + 5.0 * tv, eg)
    _close(g, g_o, "g_each (all three terms)")
    for name, terms in (("final only", (1.0, 0.0, 0.0)), ("loss_reg only", (0.0, 1.0, 0.0)), ("loss_tv only", (0.0, 0.0, 1.0))):
        e64 = each.double().requires_grad_(True)
        fo, ro, to_, _ = _pool_ref(e64, assign, size, clusters)
        (g_o,) = torch.autograd.grad(terms[0] * (fo * r.double()).sum() + terms[1] * ro.sum() + terms[2] * to_, e64)
        eg = each.to(DEV).requires_grad_(True)
        f_, r_, t_ = _ClusterPoolTrain.apply(eg, assign.to(DEV), size, clusters)[:3]
        (g,) = torch.autograd.grad(terms[0] * (f_ * r.to(DEV)).sum() + terms[1] * r_.sum() + terms[2] * t_, eg)
        _close(g, g_o, "g_each, " + name)


@pytest.mark.parametrize("size,batch,shapes", [(16, 2, ((512, 4), (256, 32), (32, 16), (32, 64))), (12, 3, ((40, 5), (256, 48))),
                                               (22, 3, ((40, 26), (8, 5)))])
def test_attention_logits_bwd_vs_float64(size, batch, shapes):
    """Every output of w2e_attention_logits_bwd: channel counts 512 / 256 / 32 (and 40: not a multiple of the 32-channel chunk), source
    resolutions below, at and above `size` (and 5 -> 12: a non-integer ratio; 26 -> 22: a ratio at which torch's nearest resize and
    floor(dst * in / out) read different pixels), explicit non-zero noise and noise strengths."""
    from where2edit_amd.run_attention import _MaskLogitsTrain
    n, eps = len(shapes), 1e-8
    t = lambda name, shape, scale=1.0, shift=0.0: seeded.tensor(f"logits{size}.{name}", shape, scale, shift)  # noqa: E731
    feats = [t(f"f{j}", (batch, c, r, r)) for j, (c, r) in enumerate(shapes)]
    per = []
    for j, (c, r) in enumerate(shapes):
        per += [t(f"w{j}", (c, 32), 1.0 / c ** 0.5), t(f"s{j}", (batch, c), 0.5, 1.0), t(f"b{j}", (32,), 0.3), t(f"nw{j}", (1,), 0.2, 0.3)]
    small = [t("wl", (32 * n,), 1.0 / (32 * n) ** 0.5), t("sl", (batch, 32 * n), 0.5, 1.0), t("bl", (1,), 0.2), t("nwl", (1,), 0.2, 0.4),
             t("ib", (1,), 0.1, 0.6)]
    noises = [t(f"noise{j}", (batch, size * size)) for j in range(n + 1)]
    r = t("r", (batch, size, size))
    leaves = [x.double().requires_grad_(True) for x in small + per]
    each_o = _logits_ref([f.double() for f in feats], leaves[5:], *leaves[:5], [z.double() for z in noises], size, eps)
    grads_o = torch.autograd.grad((each_o * r.double()).sum(), leaves)
    gl = [x.to(DEV).requires_grad_(True) for x in small + per]
    each = _MaskLogitsTrain.apply([f.to(DEV) for f in feats], [z.to(DEV) for z in noises], size, eps, eps, *gl)
    print(f"attention_logits_bwd size {size} B {batch} sources {shapes}")
    _close(each, each_o, "each")
    grads = torch.autograd.grad((each * r.to(DEV)).sum(), gl)
    names = ["g_wlast", "g_s_last", "g_bias_last", "g_nw_last", "g_initial_bias"]
    for j in range(n):
        names += [f"g_wscaled_{j}", f"g_style_{j}", f"g_bias_{j}", f"g_noise_w_{j}"]
    for name, g, go in zip(names, grads, grads_o):
        assert g.shape == go.shape, name
        _close(g, go, name)


# ---------------------------------------------------------------------------------------------------- net level
def _opted_in_net(initial_bias=None):
    from where2edit_amd.run_attention import train_mask_branch
    net, sd = C.seeded_state_dict(initial_bias)
    net.load_state_dict(sd, strict=True)
    return train_mask_branch(net.to(DEV).train()), sd


def _seeded_inputs():
    x, att_text, _ = M.inputs()
    return x, att_text, M.feature_maps()


def _zero_noises(n, batch, size):
    return [torch.zeros(batch, size * size, device=DEV) for _ in range(n + 1)]


def _net_mask_grads(net, x, att_text, feats, size, noises=None):
    out, final, losses = net([t.to(DEV) for t in x], [f.to(DEV) for f in feats], size, attention_text=att_text.to(DEV), _mask_noises=noises)
    params = {n: p for n, p in net.named_parameters() if C.is_mask_param(n)}
    grads = torch.autograd.grad(C.fixture_scalar(final, losses), list(params.values()), allow_unused=True)
    return dict(zip(params, grads)), final, losses


def test_opted_in_net_matches_the_references_mask_gradients():
    g = golden("attention_grad")
    net, _ = _opted_in_net()
    x, att_text, feats = _seeded_inputs()
    grads, final, _ = _net_mask_grads(net, x, att_text, feats, M.SIZE)
    assert_close(final, golden("attention_net")["final_map"], 1e-4, "blurred map of the opted-in net")
    assert sorted(n for n, v in grads.items() if v is None) == sorted(str(n) for n in g["unused"])  # conv.modulation.*: .grad stays None
    for key, name, rows in C.fixture_entries(g):
        got = grads[name] if rows is None else grads[name][:rows]
        assert_grad_close(got, g["grad." + key], "mask grad vs reference fixture: " + key)
        print(f"  {key}: rel err {rel_err(got, g['grad.' + key]):.3e}")


def _compare_every_mask_param(grads, grads_o, unused_o, what):
    compared = 0
    for n, go in grads_o.items():
        if n.endswith("noise.weight"):  # the oracle adds a constant zero noise: gradient 0; with zero noise pinned the kernels write exactly 0
            assert not go.any() and grads[n] is not None and not grads[n].any(), n
            continue
        assert_grad_close(grads[n], go, f"{what}: {n}")
        print(f"  {n}: rel err {rel_err(grads[n], go):.3e}")
        compared += 1
    assert compared == sum(1 for n in grads if ".conv.modulation." not in n and not n.endswith("noise.weight"))  # every other mask parameter
    for n in unused_o:
        assert ".conv.modulation." in n and grads[n] is None, n


def test_relu_kink_of_loss_reg_is_exercised_on_both_sides():
    """On the committed seeded problem (initial_bias 1.35) every non-empty cluster mean is above 0.7 (lowest 0.7385).  initial_bias 1.0
    (chosen on the CPU, float64 oracle) puts one cluster below: means 0.6674 ... 0.8371, the nearest 1.5e-2 from 0.7."""
    for bias, below in ((1.35, 0), (1.0, 1)):
        net, sd = _opted_in_net(bias)
        x, att_text, feats = _seeded_inputs()
        grads_o, unused_o, extra = C.oracle_mask_grads(sd, x, feats, M.SIZE, att_text, **CFG)
        means = [m for _, _, m in C.cluster_means(extra, M.CLUSTERS)]
        assert all(abs(m - 0.7) >= 1e-3 for m in means), means
        assert sum(m < 0.7 for m in means) >= below and any(m > 0.7 for m in means), means
        print(f"initial_bias {bias}: {sum(m < 0.7 for m in means)} of {len(means)} non-empty cluster means below 0.7")
        n_src = len(net._sources(len(x)))
        grads, _, _ = _net_mask_grads(net, x, att_text, feats, M.SIZE, _zero_noises(n_src, M.BATCH, M.SIZE))
        _compare_every_mask_param(grads, grads_o, unused_o, f"initial_bias {bias}")


def test_opted_in_net_at_ffhq1024_shapes_vs_float64_oracle():
    """The shipped setting of test_attention_map_at_ffhq1024_shapes_vs_oracle (18 sources, resolutions 4..1024, channels 512..32, size
    64, K = 20, batch 2): every mask parameter's gradient against the float64 oracle.  Measured on an MI355X: every parameter <= 5e-5
    except source 21 (64 channels at 512^2: conv.weight 9.4e-4, its two style tensors 5.2e-4, cosine 0.9999998) -- the size of one
    LeakyReLU pre-activation within fp32 rounding of 0 taking the other slope, as helpers.assert_grad_close describes."""
    from where2edit_amd.run_attention import FullSpaceMapperFEATClusterLinStyle_Net, train_mask_branch
    layers, att, k, size, b = 18, 13, 20, 64, 2
    res = [4, 4] + [r for r in (8, 16, 32, 64, 128, 256, 512, 1024) for _ in range(3)]
    ch = [512, 3] + [c for c in (512, 512, 512, 512, 256, 128, 64, 32) for c in (c, c, 3)]
    feats = [seeded.tensor(f"att1024.f{i}", (b, c, r, r)) for i, (r, c) in enumerate(zip(res, ch))]
    protos = seeded.tensor("att1024.protos", (k, 512), 1.0)
    lab = torch.from_numpy(np.random.RandomState(5).randint(0, k - 2, size=(b, 8, 8))).repeat_interleave(8, 1).repeat_interleave(8, 2)
    feats[att - 1] = (protos[lab].permute(0, 3, 1, 2) + 0.25 * seeded.tensor("att1024.noise", (b, 512, 64, 64))).contiguous()
    feats.append(seeded.tensor("att1024.const", (1, 512, 4, 4)).repeat(b, 1, 1, 1))
    net = FullSpaceMapperFEATClusterLinStyle_Net(layers, 1024, 512, attention_layer=att, channel_multiplier=2, cluster_layer=att,
                                                 clusters=k, cluster_dim=576)
    sd = M.net_state_dict(net)
    sd["initial_state"] = torch.cat([protos, 0.05 * seeded.tensor("att1024.cpos", (k, 64))], 1)
    net.load_state_dict(sd, strict=True)
    net = train_mask_branch(net.to(DEV).train())
    text = seeded.tensor("att1024.text", (b, 512), 0.3)
    att_text = seeded.tensor("att1024.att_text", (1, 512), 0.3).repeat(b, 1)
    dims = OA.dims(2)
    x = [torch.cat([text.unsqueeze(1), seeded.tensor(f"att1024.s{c}", (b, 1, dims[c]), 0.5, 1.0)], -1) for c in range(26)]
    grads, final, losses = _net_mask_grads(net, x, att_text, feats, size, _zero_noises(18, b, size))
    grads = {n: (None if v is None else v.cpu()) for n, v in grads.items()}
    final, losses = final.detach().cpu(), [v.detach().cpu() for v in losses]
    torch.cuda.synchronize()
    grads_o, unused_o, extra = C.oracle_mask_grads(sd, x, feats, size, att_text, attention_layer=att, cluster_layer=att, clusters=k)
    assert torch.equal(net.last["assign"].cpu().long(), extra["choice"])
    _close(net.last["each"], extra["each"], "each_attention_map")
    assert len(grads_o) == 19 * 5 + 1  # 19 convs: conv.weight, activate.bias, noise.weight, textca weight + bias; initial_bias
    _compare_every_mask_param(grads, grads_o, unused_o, "FFHQ-1024 shapes")


# ---------------------------------------------------------------------------------------------------- trainer
def _trainer(size=256, **kw):
    import types
    from make_golden import CLIP_TINY as c
    from where2edit_amd.attention_model import Generator
    from where2edit_amd.clip_loss import CLIPLoss
    from where2edit_amd.clip_vit import CLIP
    from where2edit_amd.run_attention import FullSpaceMapperFEATClusterLinStyle_Net, RegionAttentionTrainer
    gsd = seeded.generator_state_dict(size)
    g = Generator(size, 512, 8)
    g.load_state_dict(gsd, strict=True)
    clip = CLIP(embed_dim=c["embed_dim"], vision_layers=c["vision_layers"], vision_width=c["vision_width"],
                context_length=c["context_length"], vocab_size=c["vocab_size"], transformer_width=c["text_width"],
                transformer_heads=1, transformer_layers=c["text_layers"])
    csd = seeded.clip_state_dict(**c)
    clip.load_state_dict(csd, strict=True)
    net = FullSpaceMapperFEATClusterLinStyle_Net(M.LAYERS, c["embed_dim"] + 512, c["embed_dim"], attention_layer=M.ATT_LAYER,
                                                 channel_multiplier=2, cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS, cluster_dim=576)
    msd = M.net_state_dict(net)
    net.load_state_dict(msd, strict=True)
    tr = RegionAttentionTrainer(g, CLIPLoss(types.SimpleNamespace(stylegan_size=size), model=clip), net, attention_layer=M.ATT_LAYER,
                                lr=0.01, steps=100, device=DEV, **kw)
    return tr, gsd, csd, msd, c["embed_dim"]


def test_trainer_step_with_a_trainable_mask_branch_matches_oracle():
    """test_region_attention_trainer_step_matches_oracle with train_mask_from=0.0: the mask parameters require grad in the oracle too.
    Loss terms, the gradients of the mask and of the mapper parameters, and Adam moves both groups.  (The noise strengths are 0 and
    the oracle adds zero noise: their gradients -- sum g_pre * randn here -- have no oracle counterpart and are not compared.)"""
    from oracle import clip_model as OC
    from oracle import ops as OO
    from oracle import stylegan2 as OG
    size, b = 256, 2
    tr, gsd, csd, msd, edim = _trainer(size, train_mask_from=0.0)
    tr.global_step = 30  # t = 0.3: both ramps are past their start (:1415)
    w1 = seeded.wplus_latents(b, OG.n_latent(size), salt=51)
    w2 = seeded.wplus_latents(b, OG.n_latent(size), salt=52)
    att_text = seeded.tensor("trainer.att_text", (b, edim), 0.3)
    names = [n for n, p in tr.mapper.named_parameters() if p.requires_grad]
    assert any(C.is_mask_param(n) for n in names) and any(n.startswith("mapper_") for n in names)
    osd = {k: v.clone() for k, v in msd.items()}
    for n in names:
        osd[n].requires_grad_(True)
    with torch.no_grad():
        img1, _, _, _ = OG.generator_forward(gsd, [w1], size=size, input_is_latent=True, randomize_noise=False, return_features=True)
        cfo = OC.encode_image(csd, OO.clip_preprocess(img1, size))
        img2, _, codes2, feats2 = OG.generator_forward(gsd, [w2], size=size, input_is_latent=True, randomize_noise=False, return_features=True)
        feats2 = list(feats2) + [gsd["input.input"].repeat(b, 1, 1, 1)]
        first_feats = [f[:1].repeat(b, 1, 1, 1) for f in feats2]
        first_codes = [s[:1].repeat(b, 1, 1, 1, 1) for s in codes2]
    x = [torch.cat([cfo.unsqueeze(1), s[:, :, :, 0, 0]], -1) for s in first_codes]
    first_text = att_text[:1].repeat(b, 1)
    new_codes, amap, dl, _ = OA.forward(osd, x, first_feats, M.SIZE, attention_text=first_text, attention_layer=M.ATT_LAYER,
                                        cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS, latent_dim=edim)
    img_gen, _ = OG.generator_forward(gsd, [new_codes], size=size, input_is_stylespace=True, randomize_noise=False,
                                      attention_layer=M.ATT_LAYER, attention_map=amap, feature_map=first_feats)
    feat_gen = OC.encode_image(csd, OO.clip_preprocess(img_gen, size))
    l_consist = OA.info_nce(feat_gen, cfo)
    total_o = l_consist + 1.0 * (0.03 * dl[2] + 0.01 * dl[1].squeeze()) + 0.03 * dl[0]
    grads_o = torch.autograd.grad(total_o, [osd[n] for n in names], allow_unused=True)
    before = {n: p.detach().clone() for n, p in tr.mapper.named_parameters()}
    d = tr.train_step(w1.to(DEV), w2.to(DEV), att_text.to(DEV))
    for key, ref in (("loss_consist", l_consist), ("loss_delta", dl[0]), ("loss_secphase", dl[1]), ("loss_essence", dl[2]), ("loss", total_o)):
        assert abs(float(d[key]) - float(ref.detach())) <= 2e-4 * max(abs(float(ref.detach())), 1e-3), (key, float(d[key]), float(ref.detach()))
    params = dict(tr.mapper.named_parameters())
    used = [(n, g) for n, g in zip(names, grads_o) if g is not None and not n.endswith("noise.weight")]
    for group, pick in (("trainable mask parameters", C.is_mask_param), ("trainable mapper parameters", lambda n: n.startswith("mapper_"))):
        sel = [(n, g) for n, g in used if pick(n)]
        assert sel
        assert_grad_close(torch.cat([params[n].grad.reshape(-1).cpu() for n, _ in sel]), torch.cat([g.reshape(-1) for _, g in sel]), group)
    for n, g in zip(names, grads_o):
        if g is None:
            assert params[n].grad is None, n
    moved = [n for n, p in params.items() if not torch.equal(p.detach(), before[n])]
    assert any(C.is_mask_param(n) for n in moved) and any(n.startswith("mapper_") for n in moved)
    assert all(not torch.equal(params[n].detach(), before[n]) for n, _ in used if n in ("initial_bias", "attention_first.conv.weight"))


def test_a_schedule_that_never_unfreezes_is_bit_identical_to_none():
    """Deterministic mode, three steps: train_mask_from=2.0 (never reached) leaves every parameter bit-identical to train_mask_from=None,
    and no attention* / initial* parameter moves in either."""
    import where2edit_amd
    lat = lambda salt: seeded.wplus_latents(1, 14, salt=salt).to(DEV)  # noqa: E731
    runs = []
    where2edit_amd.set_deterministic(True)
    try:
        for t_from in (None, 2.0):
            tr, _, _, msd, edim = _trainer(train_mask_from=t_from)
            text = seeded.tensor("amp.att", (1, edim), 0.3).to(DEV)
            for i in range(3):
                tr.train_step(lat(200 + i), lat(300 + i), text)
            runs.append(tr)
    finally:
        where2edit_amd.set_deterministic(False)
    a, b = runs
    moved = 0
    for (n, pa), (_, pb) in zip(a.mapper.named_parameters(), b.mapper.named_parameters()):
        assert torch.equal(pa, pb), n
        if C.is_mask_param(n):
            assert torch.equal(pa.detach().cpu(), msd[n]) and torch.equal(pb.detach().cpu(), msd[n]), n
        else:
            moved += int(not torch.equal(pa.detach().cpu(), msd[n]))
    assert moved


def test_frozen_phase_moves_only_mapper_parameters_then_the_mask_joins():
    """steps = 100, T = 0.3, starting at step 28 (both loss ramps are past their end): steps 28 and 29 are frozen, step 30 trains the mask."""
    tr, _, _, msd, edim = _trainer(train_mask_from=0.3)
    lat = lambda salt: seeded.wplus_latents(1, 14, salt=salt).to(DEV)  # noqa: E731
    text = seeded.tensor("amp.att", (1, edim), 0.3).to(DEV)
    tr.global_step = 28
    for step in range(3):
        tr.train_step(lat(400 + step), lat(500 + step), text)
        moved = [n for n, p in tr.mapper.named_parameters() if not torch.equal(p.detach().cpu(), msd[n])]
        assert any(n.startswith("mapper_") for n in moved)
        assert any(C.is_mask_param(n) for n in moved) is (step == 2), (step, [n for n in moved if C.is_mask_param(n)][:4])


# ---------------------------------------------------------------------------------------------------- reproducibility, capture, caches
def test_two_opted_in_backwards_are_bit_identical_without_deterministic_mode():
    import where2edit_amd
    from where2edit_amd import _lib
    assert _lib.get_option("deterministic") == 0
    x, att_text, feats = _seeded_inputs()
    torch.manual_seed(3)
    noises = [torch.randn(M.BATCH, M.SIZE * M.SIZE, device=DEV) for _ in range(15)]
    runs = []
    for _ in range(2):
        net, _ = _opted_in_net()
        with torch.no_grad():
            for n, p in net.named_parameters():
                if n.endswith("noise.weight"):
                    p.fill_(0.25)
        n_src = len(net._sources(len(x)))
        grads, final, _ = _net_mask_grads(net, x, att_text, feats, M.SIZE, noises[:n_src + 1])
        runs.append((grads, final))
    for n, ga in runs[0][0].items():
        gb = runs[1][0][n]
        assert (ga is None and gb is None) or torch.equal(ga, gb), n
    assert torch.equal(runs[0][1], runs[1][1])
    assert any(g is not None and g.abs().max() > 0 for n, g in runs[0][0].items() if n.endswith("noise.weight"))


def test_opted_in_losses_and_backward_capture_into_a_graph():
    """The opted-in net's forward + backward (final, loss_reg, loss_tv -> every mask parameter) as one hipGraph: the replay writes the
    same gradients as the eager run (no memset / memcpy node, no host synchronisation in the new path)."""
    x, att_text, feats = _seeded_inputs()
    net, _ = _opted_in_net()
    xg, fg, tg = [t.to(DEV) for t in x], [f.to(DEV) for f in feats], att_text.to(DEV)
    n_src = len(net._sources(len(x)))
    torch.manual_seed(5)
    noises = [torch.randn(M.BATCH, M.SIZE * M.SIZE, device=DEV) for _ in range(n_src + 1)]
    params = [p for n, p in net.named_parameters() if C.is_mask_param(n) and ".conv.modulation." not in n]
    r = seeded.tensor("attgrad.r", (M.BATCH, 1, M.SIZE, M.SIZE)).to(DEV)

    def step():
        _, final, losses = net(xg, fg, M.SIZE, attention_text=tg, _mask_noises=noises)
        return torch.autograd.grad(C.fixture_scalar(final, losses, r), params)

    eager = [g.clone() for g in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for g in captured:
        g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for p, a, b in zip(params, eager, captured):
        assert torch.equal(a, b)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, captured))


def test_graph_safety_tool_finds_no_memset_or_memcpy_in_the_new_kernels():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("graph_safety", os.path.join(root, "tools", "graph_safety.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ops = tool.mask_branch_memops(batch=2)
    print("memset / memcpy operations of the mask-branch Functions:", dict(ops))
    assert not ops, dict(ops)


def test_optimizer_step_invalidates_the_weight_caches():
    """_wsc_t / _text_pack / _noise_off are keyed on the parameters' versions: after an optimizer step the frozen (cached) forward and the
    opted-in forward both use the new weights, and agree with a freshly loaded net."""
    from where2edit_amd.run_attention import freeze_mask_branch, train_mask_branch
    x, att_text, feats = _seeded_inputs()
    xg, fg, tg = [t.to(DEV) for t in x], [f.to(DEV) for f in feats], att_text.to(DEV)
    net, sd = _opted_in_net()
    freeze_mask_branch(net)
    with torch.no_grad():
        _, final0, _ = net(xg, fg, M.SIZE, attention_text=tg)  # fills the caches
    assert net.__dict__.get("_wsc_t") and net.__dict__.get("_text_pack")
    train_mask_branch(net)
    opt = torch.optim.SGD([p for n, p in net.named_parameters() if C.is_mask_param(n)], lr=0.5)
    zeros = _zero_noises(len(net._sources(len(x))), M.BATCH, M.SIZE)
    _, final, losses = net(xg, fg, M.SIZE, attention_text=tg, _mask_noises=zeros)
    assert_close(final, final0, 1e-5, "opted-in forward vs the cached forward (same kernels; the style GEMMs differ in rounding)")
    C.fixture_scalar(final, losses).backward()
    opt.step()
    with torch.no_grad():
        _, final_trained, _ = net(xg, fg, M.SIZE, attention_text=tg)                      # opted in, no grad: the cached path
    _, final_grad, _ = net(xg, fg, M.SIZE, attention_text=tg, _mask_noises=zeros)         # the differentiable path
    freeze_mask_branch(net)
    _, final_frozen, _ = net(xg, fg, M.SIZE, attention_text=tg)
    assert rel_err(final_trained, final0) > 1e-3, "the step did not change the map: the test shows nothing"
    fresh, _ = C.seeded_state_dict()
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh = fresh.to(DEV).requires_grad_(False)
    _, final_fresh, _ = fresh(xg, fg, M.SIZE, attention_text=tg)
    assert torch.equal(final_trained, final_fresh) and torch.equal(final_frozen, final_fresh)  # stale caches would show here
    assert_close(final_grad, final_fresh, 1e-5, "differentiable path after the step")
