"""CPU-side checks of the CLIP text-tower entry points (include/w2e_vit.h, csrc/text.hip) and of CLIP.encode_text's dispatch rule:
every bad argument is refused with a message before any HIP call (so no GPU is needed), and CPU tokens keep the stock composition."""
import ctypes

import pytest
import torch

P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
D = P(4096)  # a non-null, aligned dummy address: never dereferenced, every call below is refused first


@pytest.fixture(scope="module")
def lib():
    from where2edit_amd import build
    lib = ctypes.CDLL(build.build(verbose=False))
    from where2edit_amd import _lib
    for name in ("w2e_text_embed", "w2e_attn_causal_fwd", "w2e_text_pool"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._PROTOS[name]
    lib.w2e_last_error.restype = ctypes.c_char_p
    return lib


def _refused(lib, rc, *words):
    msg = lib.w2e_last_error()
    assert rc == 1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def _embed(lib, tokens=D, token_bytes=8, table=D, vocab=49408, pos=D, out=D, batch=2, seq=77, dim=512):
    return lib.w2e_text_embed(tokens, token_bytes, table, vocab, pos, out, batch, seq, dim, None)


def _attn(lib, qkv=D, nsplit=1, slab=0, bias=D, out=D, batch=2, seq=77, heads=8, packed=0):
    return lib.w2e_attn_causal_fwd(qkv, nsplit, slab, bias, out, batch, seq, heads, packed, None)


def _pool(lib, part=D, nsplit=1, slab=0, bias=D, res=D, tokens=D, token_bytes=8, batch=2, seq=77, gamma=D, beta=D, out=D, dim=512):
    return lib.w2e_text_pool(part, nsplit, slab, bias, res, tokens, token_bytes, batch, seq, gamma, beta, 1e-5, out, dim, None)


@pytest.mark.parametrize("kw", [dict(tokens=None), dict(table=None), dict(pos=None), dict(out=None)])
def test_text_embed_refuses_null_pointers(lib, kw):
    _refused(lib, _embed(lib, **kw), "text_embed", "null")


def test_text_embed_refuses_bad_arguments(lib):
    _refused(lib, _embed(lib, seq=97), "text_embed", "seq 97")
    _refused(lib, _embed(lib, seq=0), "text_embed", "seq 0")
    _refused(lib, _embed(lib, dim=640), "text_embed", "dim 640")
    _refused(lib, _embed(lib, dim=64), "text_embed", "dim 64")
    for tb in (0, 2, 16):
        _refused(lib, _embed(lib, token_bytes=tb), "text_embed", f"token_bytes {tb}")
    _refused(lib, _embed(lib, vocab=0), "text_embed", "vocab")


@pytest.mark.parametrize("kw", [dict(qkv=None), dict(out=None), dict(nsplit=0)])
def test_attn_causal_refuses_null_pointers(lib, kw):
    _refused(lib, _attn(lib, **kw), "attn_causal_fwd")


def test_attn_causal_refuses_bad_arguments(lib):
    _refused(lib, _attn(lib, seq=97), "attn_causal_fwd", "seq 97")
    _refused(lib, _attn(lib, seq=0), "attn_causal_fwd", "seq 0")
    _refused(lib, _attn(lib, heads=1), "attn_causal_fwd", "64 unsupported")   # width = heads * 64 must be 512 / 768 / 1024
    _refused(lib, _attn(lib, heads=10), "attn_causal_fwd", "640 unsupported")
    _refused(lib, _attn(lib, packed=2 * 77 - 1), "attn_causal_fwd", "out_packed_rows 153 for 154 rows")
    assert _attn(lib, batch=0, packed=0) == 0  # nothing to do: accepted without a launch


@pytest.mark.parametrize("kw", [dict(part=None), dict(tokens=None), dict(gamma=None), dict(beta=None), dict(out=None), dict(nsplit=0)])
def test_text_pool_refuses_null_pointers(lib, kw):
    _refused(lib, _pool(lib, **kw), "text_pool")


def test_text_pool_refuses_bad_arguments(lib):
    _refused(lib, _pool(lib, seq=97), "text_pool", "seq 97")
    _refused(lib, _pool(lib, dim=256), "text_pool", "dim 256")
    _refused(lib, _pool(lib, token_bytes=2), "text_pool", "token_bytes 2")
    assert _pool(lib, batch=0) == 0


def _clip(width=512, heads=8, layers=1, ctx=77):
    from where2edit_amd.clip_vit import CLIP
    torch.manual_seed(0)
    m = CLIP(embed_dim=64, image_resolution=32, vision_layers=1, vision_width=64, vision_patch_size=32, context_length=ctx, vocab_size=100,
             transformer_width=width, transformer_heads=heads, transformer_layers=layers)
    return m.requires_grad_(False).eval()


def test_dispatch_refuses_the_hip_path_for_cpu_tokens(monkeypatch):
    from where2edit_amd import vit_hip
    m = _clip()
    tokens = torch.randint(0, 100, (2, 77))
    assert not vit_hip.text_hip_ok(m, tokens)
    assert not vit_hip.text_hip_ok(m, tokens.int())

    def boom(*a, **k):
        raise AssertionError("the HIP text tower ran on CPU tokens")

    monkeypatch.setattr(vit_hip, "text_forward", boom)
    out = m.encode_text(tokens)  # the stock composition, unchanged
    assert out.shape == (2, 64)
    assert torch.equal(out, m._encode_text_stock(tokens))
