"""Image I/O on the GPU (where2edit_amd/image_io.py, csrc/image.hip) against the numpy restatement of tests/imageio_ref.py, which
tests/test_image_io_host.py holds against Pillow and the torch CPU op sequence: byte for byte / bit for bit, no tolerance anywhere.

SHAPES (B, C, in_h, in_w, out_h, out_w) and what each exercises:
    (1,3,5,5,1,1)            one output pixel whose window is the whole image
    (2,1,2,3,5,4)            up-scaling both axes, windows clipped at both borders
    (1,3,9,7,16,16)          up-scaling, non-square
    (2,3,37,53,16,16)        non-integer scales, 159-byte rows
    (1,3,16,16,16,8)         vertical pass skipped
    (1,1,16,24,4,24)         horizontal pass skipped
    (1,3,64,64,64,64)        identity, both passes skipped
    (1,1,100,75,32,33)       non-integer scales, single channel
    (1,3,200,520,50,130)     several tiles in both axes, ragged last tiles
    (1,3,300,200,7,11)       the two-launch form
    (2,1,512,512,64,64)      the label shape
    (2,3,1024,1024,256,256)  the image shape
"""
import functools
import types

import numpy as np
import pytest
import torch

import imageio_ref as R
import seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILTERS = ("bilinear", "nearest")


@functools.lru_cache(maxsize=None)
def _input(index, name):
    x = R.pattern(name, R.SHAPES[index], index)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(index, name, filter):
    """The restatement's resize of a pattern: computed once, shared by the tests below, read-only."""
    s = R.SHAPES[index]
    y = R.resize(_input(index, name), s[4], s[5], filter)
    y.setflags(write=False)
    return y


def _gpu(x):
    return torch.from_numpy(np.array(x)).to(DEV)  # (a copy: the cached inputs are read-only)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("index", range(len(R.SHAPES)))
def test_resize_u8_equals_the_reference_byte_for_byte(index, filter):
    from where2edit_amd.image_io import label_ids, resize_plan, resize_u8
    s = R.SHAPES[index]
    assert resize_plan(*s)["form"] == (1 if s == (1, 3, 300, 200, 7, 11) else 0)
    for name in R.PATTERNS:
        x = _input(index, name)
        got = resize_u8(_gpu(x), (s[4], s[5]), filter)
        want = _ref(index, name, filter)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_contiguous()
        bad = int((got.cpu().numpy() != want).sum())
        assert bad == 0, f"{s} {filter} {name}: {bad} of {want.size} bytes differ"
        if s[1] == 1:  # the [B,H,W] layout, as labels come
            got3 = label_ids(_gpu(x[..., 0]), (s[4], s[5]), filter)
            assert tuple(got3.shape) == want.shape[:3] and np.array_equal(got3.cpu().numpy(), want[..., 0])


@pytest.mark.parametrize("index", range(len(R.SHAPES)))
def test_to_tensor_is_the_table_applied_to_those_bytes_bit_for_bit(index):
    from where2edit_amd.image_io import to_tensor
    s = R.SHAPES[index]
    c = s[1]
    x = _gpu(_input(index, "random"))
    stats = [(0.5, 0.5), ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)) if c == 3 else ((0.3,), (0.7,))]
    for mean, std in stats:
        got = to_tensor(x, (s[4], s[5]), mean=mean, std=std)
        want = R.to_tensor(_ref(index, "random", "bilinear"), mean, std)
        assert got.dtype == torch.float32 and tuple(got.shape) == (s[0], c, s[4], s[5]) and got.is_contiguous()
        assert np.array_equal(_bits(got).numpy(), want.view(np.int32)), (s, mean)
    if s[2] == s[4] and s[3] == s[5]:  # size=None: no resize, the table alone
        assert torch.equal(_bits(to_tensor(x)), _bits(to_tensor(x, (s[4], s[5]))))


@pytest.mark.parametrize("index", [3, 6, 8, 9, 11])
def test_a_source_one_byte_past_an_aligned_address_gives_the_same_bytes(index):
    """The staging loop reads 16-byte chunks at their absolute alignment and bytes at the two ragged ends of the buffer: every row of
    such a view starts at another address modulo 16 than in the aligned tensor."""
    from where2edit_amd.image_io import resize_u8, to_tensor
    s = R.SHAPES[index]
    x = _input(index, "random")
    flat = torch.zeros(x.size + 32, dtype=torch.uint8, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:1 + x.size].view(x.shape)
    view.copy_(_gpu(x))
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    for filter in FILTERS:
        assert np.array_equal(resize_u8(view, (s[4], s[5]), filter).cpu().numpy(), _ref(index, "random", filter)), (s, filter)
    assert torch.equal(_bits(to_tensor(view, (s[4], s[5]))), _bits(to_tensor(_gpu(x), (s[4], s[5]))))


def test_tables_are_cached_per_device_and_an_empty_batch_is_empty():
    from where2edit_amd import image_io as I
    I.clear_caches()
    x = _gpu(_input(3, "random"))
    a = I.to_tensor(x, 16)
    keys = set(I._DEVICE_TABLES), set(I._NORM_TABLES)
    held = [t.data_ptr() for pair in I._DEVICE_TABLES.values() for t in pair]
    b = I.to_tensor(x, 16)
    assert (set(I._DEVICE_TABLES), set(I._NORM_TABLES)) == keys and len(keys[0]) == 2 and len(keys[1]) == 1
    assert held == [t.data_ptr() for pair in I._DEVICE_TABLES.values() for t in pair] and torch.equal(a, b)
    assert tuple(I.resize_u8(x[:0], 16).shape) == (0, 16, 16, 3)
    assert tuple(I.to_bytes(torch.zeros(0, 3, 4, 4, device=DEV), grid=False).shape) == (0, 4, 4, 3)


@pytest.mark.parametrize("lo,hi", [(-1, 1), (0, 1)])
def test_to_bytes_equals_the_reference_on_the_boundary_set(lo, hi):
    """Every rounding boundary of the quantiser with three fp32 neighbours on either side, the range's ends, +-5, +-inf, NaN and
    100 000 seeded values a little wider than the range -- laid out as one 3-channel image (zero-filled to a rectangle)."""
    from where2edit_amd.image_io import to_bytes
    vals = R.boundary_set(lo, hi)
    h, w = 184, 185
    assert 3 * h * w >= vals.size
    x = np.zeros(3 * h * w, np.float32)
    x[:vals.size] = vals
    x = x.reshape(1, 3, h, w)
    for grid in (False, True):
        got = to_bytes(_gpu(x), value_range=(lo, hi), grid=grid).cpu().numpy()
        want = R.to_bytes(x, lo, hi, grid=grid)
        assert got.shape == want.shape and got.dtype == np.uint8
        bad = np.flatnonzero(got.ravel() != want.ravel())
        assert bad.size == 0, f"range ({lo}, {hi}) grid={grid}: {bad.size} bytes differ, first at {bad[:5]}"
    y = x.reshape(3, 1, h, w)  # the same values as three 1-channel images
    assert np.array_equal(to_bytes(_gpu(y), value_range=(lo, hi), grid=False).cpu().numpy(), R.to_bytes(y, lo, hi, grid=False))


@pytest.mark.parametrize("h,w", [(6, 10), (64, 64)])
def test_grids_are_exact(h, w):
    from where2edit_amd.image_io import to_bytes
    rng = np.random.RandomState(h)
    cases = [dict(b=1, c=3),                         # a batch of one: unpadded
             dict(b=2, c=3),                         # the couple_outputs pair
             dict(b=3, c=3, nrow=2),                 # an empty cell = pad
             dict(b=3, c=1, nrow=2),                 # one channel replicated
             dict(b=1, c=1),
             dict(b=2, c=3, pad_value=1.0),
             dict(b=5, c=3, nrow=3, padding=1, pad_value=0.25),
             dict(b=9, c=1, nrow=8, padding=0),
             dict(b=2, c=3, grid=False), dict(b=2, c=1, grid=False)]
    for case in cases:
        kw = dict(case)
        b, c = kw.pop("b"), kw.pop("c")
        x = rng.uniform(-1.2, 1.2, size=(b, c, h, w)).astype(np.float32)
        got = to_bytes(_gpu(x), **kw).cpu().numpy()
        want = R.to_bytes(x, **kw)
        assert got.shape == want.shape and np.array_equal(got, want), case


@pytest.fixture(scope="module")
def config5():
    """The seeded modules of tests/test_gpu_irse.py's config-5 test, at its size (1024^2 generator, tiny CLIP, 20 clusters at layer
    13), with deterministic kernels: two runs on the same input must agree bit for bit for the comparisons below to mean anything
    (the direct convolutions otherwise join their K splits with fp32 atomics)."""
    import make_golden_attention as MA
    import make_golden_e4e as ME
    import where2edit_amd
    from make_golden import CLIP_TINY as c
    from where2edit_amd.attention_model import Generator
    from where2edit_amd.clip_loss import CLIPLoss
    from where2edit_amd.clip_vit import CLIP
    from where2edit_amd.psp_encoders import Encoder4Editing
    from where2edit_amd.run_attention import FullSpaceMapperFEATClusterLinStyle_Net
    size, k, att = 1024, 20, 13
    opts = types.SimpleNamespace(stylegan_size=size)
    e4e = Encoder4Editing(50, "ir_se", opts).eval()
    e4e.load_state_dict(ME.encoder_state_dict(e4e.state_dict()), strict=True)
    g = Generator(size, 512, 8)
    g.load_state_dict(seeded.generator_state_dict(size), strict=True)
    clip = CLIP(embed_dim=c["embed_dim"], vision_layers=c["vision_layers"], vision_width=c["vision_width"], context_length=c["context_length"],
                vocab_size=c["vocab_size"], transformer_width=c["text_width"], transformer_heads=1, transformer_layers=c["text_layers"])
    clip.load_state_dict(seeded.clip_state_dict(**c), strict=True)
    edim = c["embed_dim"]
    net = FullSpaceMapperFEATClusterLinStyle_Net(18, edim + 512, edim, attention_layer=att, channel_multiplier=2, cluster_layer=att, clusters=k,
                                                 cluster_dim=576)
    msd = MA.net_state_dict(net)
    msd["initial_bias"] = torch.tensor([0.9])
    msd["initial_state"] = seeded.tensor("io.centres", (k, 576), 1.0)  # (that test takes them from the oracle's features; any 20 do here)
    net.load_state_dict(msd, strict=True)
    mods = (e4e.to(DEV).requires_grad_(False), g.to(DEV).requires_grad_(False), CLIPLoss(opts, model=clip).to(DEV), net.to(DEV).requires_grad_(False))
    where2edit_amd.set_deterministic(True)
    yield mods, edim, att
    where2edit_amd.set_deterministic(False)


FLOAT_KEYS = ("img_orig", "img_gen", "mask", "latents", "features_orig", "features_gen")


def _same(a, b, keys):
    for key in keys:
        x, y = a[key], b[key]
        assert x.dtype == y.dtype and x.shape == y.shape, key
        assert torch.equal(_bits(x), _bits(y)) if x.dtype == torch.float32 else torch.equal(x.cpu(), y.cpu()), key
    for x, y in zip(a["new_codes"], b["new_codes"]):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("bsz", [1, 2])
def test_invert_and_edit_on_bytes_equals_the_float_pipeline(config5, bsz):
    from where2edit_amd.demo_pipeline import capture_invert_and_edit, invert_and_edit
    from where2edit_amd.image_io import to_bytes, to_tensor
    (e4e, g, clip_loss, net), edim, att = config5
    rng = np.random.RandomState(40 + bsz)
    u8 = _gpu(rng.randint(0, 256, size=(bsz, 37, 53, 3)).astype(np.uint8))
    text, att_text = seeded.tensor("io.text", (bsz, edim), 0.3).to(DEV), seeded.tensor("io.att", (bsz, edim), 0.3).to(DEV)
    want = invert_and_edit(to_tensor(u8, 256), e4e, g, clip_loss, net, text, att_text, attention_layer=att)
    assert set(want) == set(FLOAT_KEYS) | {"new_codes"}  # float in, defaults: what it returned before
    got = invert_and_edit(u8, e4e, g, clip_loss, net, text, att_text, attention_layer=att, as_bytes=True)
    _same(got, want, FLOAT_KEYS)
    assert tuple(got["img_gen_u8"].shape) == (bsz, 1024, 1024, 3) and tuple(got["mask_u8"].shape) == (bsz, 64, 64, 1)
    for key in ("img_orig", "img_gen"):
        assert torch.equal(got[key + "_u8"], to_bytes(want[key], (-1, 1), grid=False)), key
    assert torch.equal(got["mask_u8"], to_bytes(want["mask"], (0, 1), grid=False))
    assert float(got["img_gen_u8"].float().std()) > 1 and float((want["img_gen"] - want["img_orig"]).abs().max()) > 0
    if bsz == 2:  # one captured replay with fresh bytes in the static buffers equals the eager call
        run = capture_invert_and_edit(torch.zeros_like(u8), e4e, g, clip_loss, net, torch.zeros_like(text), torch.zeros_like(att_text),
                                      attention_layer=att, as_bytes=True)
        rep = run(u8, text, att_text)
        torch.cuda.synchronize()
        _same(rep, got, FLOAT_KEYS + ("img_orig_u8", "img_gen_u8", "mask_u8"))


def test_calculate_iou_resizes_bytes_as_the_pieces_called_by_hand():
    """uint8 labels at 4x the mask's size with label_resize = "bilinear" / "nearest" against calculate_iou on label_ids(...) called by
    hand; then uint8 images of another size against calculate_iou on to_tensor(..., 256).  G(256) + the seeded net of
    tests/test_gpu_attention.py (mask at layer 7 = 16 x 16), deterministic kernels."""
    import make_golden_attention as M
    import make_golden_e4e as ME
    import test_gpu_attention as TA
    import where2edit_amd
    from where2edit_amd import calculate_iou
    from where2edit_amd.attention_model import Generator
    from where2edit_amd.image_io import label_ids, to_tensor
    from where2edit_amd.psp_encoders import Encoder4Editing
    g = Generator(256, 512, 8)
    g.load_state_dict(seeded.generator_state_dict(256), strict=True)
    g = g.to(DEV).eval().requires_grad_(False)
    net, _ = TA._net()
    net = net.requires_grad_(False)
    where2edit_amd.set_deterministic(True)
    try:
        w = seeded.wplus_latents(2, g.n_latent, salt=61).to(DEV)
        text = seeded.tensor("iou.text8", (8, 512), 0.3).to(DEV)
        big = R.block_label(np.random.RandomState(9).randint(0, 19, size=(2 * 8, 8)).astype(np.uint8), 8).reshape(2, 64, 64)
        lab = torch.from_numpy(big)
        kw = dict(attention_layer=M.ATT_LAYER)
        results = {}
        for filter in ("bilinear", "nearest"):
            hand = label_ids(lab.to(DEV), M.SIZE, filter)
            assert tuple(hand.shape) == (2, M.SIZE, M.SIZE)
            results[filter] = calculate_iou([(w, hand)], g, net, text, **kw)
            assert calculate_iou([(w, lab)], g, net, text, label_resize=filter, **kw) == results[filter]
            assert calculate_iou([(w, lab.unsqueeze(1))], g, net, text, label_resize=filter, **kw) == results[filter]
        assert not torch.equal(label_ids(lab.to(DEV), M.SIZE, "bilinear"), label_ids(lab.to(DEV), M.SIZE, "nearest"))
        with pytest.raises(RuntimeError, match=r"resize the labels to 16 x 16 \(nearest\)"):  # None: as before
            calculate_iou([(w, lab)], g, net, text, **kw)
        with pytest.raises(ValueError, match="label_resize"):
            calculate_iou([(w, lab)], g, net, text, label_resize="bicubic", **kw)
        # decoded images in
        e4e = Encoder4Editing(50, "ir_se", types.SimpleNamespace(stylegan_size=256)).eval()
        e4e.load_state_dict(ME.encoder_state_dict(e4e.state_dict()), strict=True)
        e4e = e4e.to(DEV).requires_grad_(False)
        img = torch.from_numpy(np.random.RandomState(10).randint(0, 256, size=(2, 300, 280, 3)).astype(np.uint8))
        a = calculate_iou([(img, lab)], g, net, text, e4e=e4e, label_resize="bilinear", **kw)
        b = calculate_iou([(to_tensor(img.to(DEV), 256), label_ids(lab.to(DEV), M.SIZE))], g, net, text, e4e=e4e, **kw)
        assert a == b and len(a[0]) == 8
        with pytest.raises(RuntimeError, match="pass e4e"):
            calculate_iou([(img, lab)], g, net, text, label_resize="bilinear", **kw)
    finally:
        where2edit_amd.set_deterministic(False)
