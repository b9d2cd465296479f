"""The CLIP text tower on the HIP kernels (csrc/text.hip + the block kernels of vit2.hip / vit3.hip, vit_hip.text_forward): the causal
attention, embedding and pooling kernels against float64 torch, the whole tower against the CPU oracle, the dispatch rule of
CLIP.encode_text, graph capture, and the region-attention trainer fed with token ids."""
import pytest
import torch

import seeded
from helpers import assert_close, rel_err
from oracle import clip_model as OC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _call(name, *args):
    from where2edit_amd._lib import call, stream_ptr
    call(name, *args, stream_ptr())


def _p(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------- causal attention
def _attn_ref(qkv_sum, b, l, heads):
    q, k, v = qkv_sum.double().view(b, l, 3, heads, 64).permute(2, 0, 3, 1, 4)
    att = q @ k.transpose(-1, -2) / 8 + torch.full((l, l), float("-inf"), dtype=torch.float64, device=qkv_sum.device).triu(1)
    return (att.softmax(-1) @ v).transpose(1, 2).reshape(b * l, heads * 64)


def _attn_run(slabs, bias, b, l, heads, packed):
    from where2edit_amd.vit_hip import _pad, ptr
    m, dim = b * l, heads * 64
    if packed:
        mpad = _pad(m, 32) + 32  # at least 32 padded rows, which must come back untouched
        out = torch.full((dim // 4, mpad, 4), 777.0, device=DEV)
    else:
        mpad = 0
        out = torch.empty((m, dim), device=DEV)
    _call("w2e_attn_causal_fwd", ptr(slabs), slabs.shape[0], m * 3 * dim, ptr(bias), ptr(out), b, l, heads, mpad)
    return out, mpad


@pytest.mark.parametrize("l", [1, 2, 31, 32, 33, 64, 77, 96])
@pytest.mark.parametrize("heads", [8, 12])
def test_causal_attention_vs_float64(l, heads):
    dim = 3 * heads * 64
    for b in (1, 3):
        for nsplit in (1, 3):
            g = torch.Generator().manual_seed(1000 * l + 10 * heads + b + nsplit)
            slabs = (torch.randn(nsplit, b * l, dim, generator=g) * (1.5 / nsplit)).to(DEV)
            bias = (torch.randn(dim, generator=g) * 0.3).to(DEV)
            ref = _attn_ref(slabs.sum(0) + bias, b, l, heads)  # (the fp32 slab sum is an exact restatement only up to rounding: 1e-5 covers it)
            for packed in (False, True):
                out, mpad = _attn_run(slabs, bias, b, l, heads, packed)
                if packed:
                    full = out.permute(1, 0, 2).reshape(mpad, heads * 64)
                    assert torch.all(full[b * l:] == 777.0), "a padded row of the packed output was written"
                    got = full[: b * l]
                else:
                    got = out
                e = rel_err(got, ref)
                assert e <= 1e-5, (l, heads, b, nsplit, packed, e)
                again, _ = _attn_run(slabs, bias, b, l, heads, packed)
                assert torch.equal(again, out), "rerun is not bit-identical"


# ---------------------------------------------------------------------------------------------- embedding and pooling
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dim", [512, 768])
def test_text_embed_is_exact_and_bad_ids_are_nan(dtype, dim):
    from where2edit_amd.vit_hip import ptr
    vocab, ctx, b, l = 1000, 96, 3, 77
    g = torch.Generator().manual_seed(dim)
    table = torch.randn(vocab, dim, generator=g).to(DEV)
    pos = torch.randn(ctx, dim, generator=g).to(DEV)
    tokens = torch.randint(0, vocab, (b, l), generator=g).to(dtype)
    tokens[0, 0], tokens[2, 76] = 0, vocab - 1  # both ends of the table
    ref = table.cpu()[tokens.long()] + pos.cpu()[:l]
    out = torch.empty(b * l, dim, device=DEV)
    tg = tokens.to(DEV)
    _call("w2e_text_embed", _p(tg), tg.element_size(), ptr(table), vocab, ptr(pos), ptr(out), b, l, dim)
    assert torch.equal(out.cpu().view(b, l, dim), ref)
    bad = tokens.clone()
    bad[1, 5], bad[2, 0] = vocab, -1
    bg = bad.to(DEV)
    _call("w2e_text_embed", _p(bg), bg.element_size(), ptr(table), vocab, ptr(pos), ptr(out), b, l, dim)
    o = out.cpu().view(b, l, dim)
    assert torch.isnan(o[1, 5]).all() and torch.isnan(o[2, 0]).all()
    keep = torch.ones(b, l, dtype=torch.bool)
    keep[1, 5] = keep[2, 0] = False
    assert torch.equal(o[keep], ref[keep])


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dim", [512, 1024])
def test_text_pool_vs_float64_layer_norm(dtype, dim):
    from where2edit_amd.vit_hip import ptr
    b, l, nsplit = 4, 77, 3
    g = torch.Generator().manual_seed(7 + dim)
    tokens = torch.randint(1, 500, (b, l), generator=g)
    tokens[0, 9] = 900
    tokens[1, 4], tokens[1, 30] = 950, 950      # the maximum twice: the first occurrence wins (torch.argmax)
    tokens[2, 76] = 999                           # EOT at the last position
    tokens[3, 0] = 999                            # ... and at the first
    tokens = tokens.to(dtype)
    part = torch.randn(nsplit, b * l, dim, generator=g).to(DEV)
    bias = torch.randn(dim, generator=g).to(DEV)
    res = torch.randn(b * l, dim, generator=g).to(DEV)
    gamma = (1 + 0.1 * torch.randn(dim, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(dim, generator=g)).to(DEV)
    out = torch.empty(b, dim, device=DEV)
    tg = tokens.to(DEV)
    _call("w2e_text_pool", ptr(part), nsplit, b * l * dim, ptr(bias), ptr(res), _p(tg), tg.element_size(), b, l, ptr(gamma), ptr(beta),
          1e-5, ptr(out), dim)
    idx = tokens.long().argmax(-1)
    assert idx.tolist() == [9, 4, 76, 0]
    rows = torch.arange(b) * l + idx
    x = part.double().cpu().sum(0)[rows] + bias.double().cpu() + res.double().cpu()[rows]
    ref = torch.nn.functional.layer_norm(x, (dim,), gamma.double().cpu(), beta.double().cpu(), 1e-5)
    assert_close(out, ref, 1e-5, "pool")


# ---------------------------------------------------------------------------------------------- the whole tower
def _clip(width=512, heads=8, layers=12, ctx=77, vocab=49408, embed=512):
    from where2edit_amd.clip_vit import CLIP
    cfg = dict(embed_dim=embed, image_resolution=32, vision_layers=1, vision_width=64, vision_patch=32, context_length=ctx,
               vocab_size=vocab, text_width=width, text_layers=layers)
    m = CLIP(embed_dim=embed, image_resolution=32, vision_layers=1, vision_width=64, vision_patch_size=32, context_length=ctx,
             vocab_size=vocab, transformer_width=width, transformer_heads=heads, transformer_layers=layers)
    sd = seeded.clip_state_dict(**cfg)
    m.load_state_dict(sd, strict=True)
    m.requires_grad_(False)
    return m.to(DEV).eval(), sd


def _tokens(b, ctx=77, vocab=49408, seed=0):
    """clip.tokenize-shaped ids: SOT, words, EOT (the largest id), zero padding; EOT positions spread over 1 .. ctx-1 (row 0 is the
    empty prompt [SOT, EOT], the last row has no padding)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(b, ctx, dtype=torch.int64)
    for i in range(b):
        n = ctx - 1 if b == 1 else 1 + (i * (ctx - 2)) // (b - 1)
        t[i, 0] = vocab - 2
        t[i, 1:n] = torch.randint(1, vocab - 2, (n - 1,), generator=g)
        t[i, n] = vocab - 1
    return t


@pytest.mark.parametrize("b", [1, 5, 24])
def test_vit_b32_text_tower_vs_oracle(b):
    from where2edit_amd import vit_hip
    m, sd = _clip()
    tokens = _tokens(b, seed=b)
    assert vit_hip.text_hip_ok(m, tokens.to(DEV))
    out = m.encode_text(tokens.to(DEV))
    ref = OC.encode_text(sd, tokens)
    ref64 = OC.encode_text({k: v.double() for k, v in sd.items()}, tokens)
    e, e64, eo = rel_err(out, ref), rel_err(out, ref64), rel_err(ref, ref64)
    print(f"text tower b={b}: vs fp32 oracle {e:.2e}, vs float64 oracle {e64:.2e} (fp32 oracle vs float64 {eo:.2e})")
    assert e <= 1e-4 and e64 <= 1e-4
    assert torch.equal(m.encode_text(tokens.int().to(DEV)), out), "int32 and int64 tokens differ"


def test_text_tower_768_wide_vs_oracle():
    m, sd = _clip(width=768, heads=12, layers=2, embed=512)
    tokens = _tokens(5, seed=11)
    out = m.encode_text(tokens.to(DEV))
    ref = OC.encode_text(sd, tokens)
    e = rel_err(out, ref)
    print(f"text tower 768 wide: vs fp32 oracle {e:.2e}")
    assert e <= 1e-4


# ---------------------------------------------------------------------------------------------- dispatch
def _kernel_names(fn):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = set()
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            names.add(e.name)
        names.update(k.name for k in (e.kernels or []))
    return out, names


def _is_blas(name):
    n = name.lower()
    return "cijk" in n or "rocblas" in n or "hipblaslt" in n


def test_dispatch(monkeypatch):
    m, sd = _clip(layers=2)
    tokens = _tokens(3, seed=5)
    td = tokens.to(DEV)
    ref = OC.encode_text(sd, tokens)
    with torch.no_grad():
        out, names = _kernel_names(lambda: m.encode_text(td))
    for k in ("text_embed_kernel", "attn_causal_fwd_kernel", "text_pool_kernel", "gemm_pk_kernel"):
        assert any(k in n for n in names), (k, sorted(names))
    assert not [n for n in names if _is_blas(n)], sorted(names)
    assert_close(out, ref, 1e-4, "HIP")
    # W2E_TEXT_STOCK=1: the stock composition
    monkeypatch.setenv("W2E_TEXT_STOCK", "1")
    stock, names = _kernel_names(lambda: m.encode_text(td))
    assert not any("attn_causal" in n for n in names)
    assert_close(stock, ref, 1e-4, "W2E_TEXT_STOCK")
    assert torch.equal(stock, m._encode_text_stock(td))
    monkeypatch.delenv("W2E_TEXT_STOCK")
    # a text parameter that needs a gradient under grad mode: stock (CLIP text fine-tuning keeps its autograd graph)
    m.ln_final.weight.requires_grad_(True)
    ft, names = _kernel_names(lambda: m.encode_text(td))
    assert ft.requires_grad and not any("attn_causal" in n for n in names)
    assert_close(ft.detach(), ref, 1e-4, "requires_grad")
    with torch.no_grad():  # ... but not under no_grad
        _, names = _kernel_names(lambda: m.encode_text(td))
    assert any("attn_causal" in n for n in names)
    m.ln_final.weight.requires_grad_(False)
    # a 64-wide tower (the tests' tiny CLIP): stock
    tiny, tsd = _clip(width=64, heads=1, layers=2, ctx=16, vocab=100, embed=32)
    tt = _tokens(2, ctx=16, vocab=100)
    small, names = _kernel_names(lambda: tiny.encode_text(tt.to(DEV)))
    assert not any("attn_causal" in n for n in names)
    assert_close(small, OC.encode_text(tsd, tt), 1e-4, "64 wide")


def test_weight_update_refreshes_the_packs():
    m, sd = _clip(layers=2)
    tokens = _tokens(2, seed=3).to(DEV)
    first = m.encode_text(tokens)
    sd2 = seeded.clip_state_dict(embed_dim=512, image_resolution=32, vision_layers=1, vision_width=64, vision_patch=32, context_length=77,
                                 vocab_size=49408, text_width=512, text_layers=2, salt=9)
    m.load_state_dict(sd2, strict=True)
    second = m.encode_text(tokens)
    assert_close(second, OC.encode_text(sd2, tokens.cpu()), 1e-4, "after load_state_dict")
    assert not torch.allclose(first, second)


# ---------------------------------------------------------------------------------------------- capture
def test_encode_text_captures_and_replays_on_new_tokens():
    from where2edit_amd.coach import capture_graph
    m, _ = _clip(layers=2)
    static = _tokens(8, seed=21).to(DEV)
    graph, out = capture_graph(lambda: m.encode_text(static), "encode_text", torch.device(DEV))  # (passes memset_guard inside)
    new = _tokens(8, seed=22).to(DEV)
    static.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    eager = m.encode_text(new)
    assert_close(out, eager, 1e-6, "replay on overwritten tokens")


# ---------------------------------------------------------------------------------------------- the trainer with token ids
def _trainer():
    import types
    import make_golden_attention as M
    from make_golden import CLIP_TINY as c
    from where2edit_amd.attention_model import Generator
    from where2edit_amd.clip_loss import CLIPLoss
    from where2edit_amd.clip_vit import CLIP
    from where2edit_amd.run_attention import FullSpaceMapperFEATClusterLinStyle_Net, RegionAttentionTrainer
    size = 256
    g = Generator(size, 512, 8)
    g.load_state_dict(seeded.generator_state_dict(size), strict=True)
    cfg = dict(c, context_length=77, vocab_size=1000, text_width=512, text_layers=2)
    clip = CLIP(embed_dim=cfg["embed_dim"], vision_layers=cfg["vision_layers"], vision_width=cfg["vision_width"],
                context_length=77, vocab_size=1000, transformer_width=512, transformer_heads=8, transformer_layers=2)
    clip.load_state_dict(seeded.clip_state_dict(**cfg), strict=True)
    net = FullSpaceMapperFEATClusterLinStyle_Net(M.LAYERS, cfg["embed_dim"] + 512, cfg["embed_dim"], attention_layer=M.ATT_LAYER,
                                                 channel_multiplier=2, cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS, cluster_dim=576)
    net.load_state_dict(M.net_state_dict(net), strict=True)
    tr = RegionAttentionTrainer(g, CLIPLoss(types.SimpleNamespace(stylegan_size=size), model=clip), net, attention_layer=M.ATT_LAYER,
                                lr=0.01, steps=100, device=DEV)
    tr.global_step = 30
    return tr


def test_trainer_takes_token_ids():
    import where2edit_amd
    from oracle import stylegan2 as OG
    b = 2
    w1 = seeded.wplus_latents(b, OG.n_latent(256), salt=61).to(DEV)
    w2 = seeded.wplus_latents(b, OG.n_latent(256), salt=62).to(DEV)
    tokens = _tokens(b, vocab=1000, seed=63).to(DEV)
    where2edit_amd.set_deterministic(True)
    try:
        runs = []
        for use_tokens in (True, False):
            tr = _trainer()
            if use_tokens:
                text = tokens
            else:
                with torch.no_grad():
                    text = tr.clip_loss.model.encode_text(tokens[:1])
            d = tr.train_step(w1, w2, text)
            grads = [p.grad.detach().clone() if p.grad is not None else None for p in tr.params]
            runs.append((d, grads))
    finally:
        where2edit_amd.set_deterministic(False)
    (d_t, g_t), (d_f, g_f) = runs
    assert d_t.keys() == d_f.keys()
    for k in d_t:
        assert torch.equal(d_t[k], d_f[k]), k
    assert any(g is not None for g in g_t)
    for a, c in zip(g_t, g_f):
        assert (a is None and c is None) or torch.equal(a, c)
