"""The mask IoU evaluation on the GPU (where2edit_amd.evaluation, csrc/evaluate.hip): the counting kernel against the integer
yardstick of tests/iou_ref.py -- exactly, count for count -- on every path it has (vector / scalar, T <= 8 / T <= 16, aligned or
not), the mask-only entry of the net against its forward, and calculate_iou against the same pieces called by hand."""
import numpy as np
import pytest
import torch

import iou_ref as R
import make_golden_attention as M
import seeded

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS = list(range(20)) + [255]  # every CelebAMask-HQ id, one past the list, and the largest byte


def _mapping(classes):
    """The CelebAMask-HQ table at T = 8 (None: MaskIoU's default); for other T every id 1..18 and 255 lands in some region 1..T."""
    if classes == 8:
        return None
    m = {raw: 1 + (raw - 1) % classes for raw in range(1, 19)}
    m[255] = classes
    return m


def _problem(b, t, s, seed):
    """masks ~ U(0.6, 1) around the threshold, labels drawn from IDS with the first min(21, n) pixels walking through all of IDS."""
    rng = np.random.RandomState(seed)
    masks = rng.uniform(0.6, 1.0, size=(b, t, s, s)).astype(np.float32)
    ids = rng.choice(IDS, size=b * s * s).astype(np.uint8)
    n = min(len(IDS), ids.size)
    ids[:n] = IDS[:n]
    return masks, ids.reshape(b, s, s)


def _metric(t, **kw):
    from where2edit_amd import MaskIoU
    return MaskIoU(classes=t, mapping=_mapping(t), device=DEV, **kw)


@pytest.mark.parametrize("b,t,s", [(3, 8, 6),     # S*S = 36: the scalar path, less than one wave per image
                                   (2, 8, 64),    # the evaluation's shape: the vector path, more than one workgroup
                                   (1, 1, 1),
                                   (2, 16, 10)])  # the largest T; S*S a multiple of 4 but not of 64
def test_counts_equal_the_integer_reference(b, t, s):
    masks, ids = _problem(b, t, s, seed=100 * t + s)
    m = _metric(t)
    m.update(torch.from_numpy(masks).to(DEV), torch.from_numpy(ids).to(DEV))
    want = R.confusion_counts(masks, ids, t, mapping=_mapping(t))
    got = m.counts()
    assert got.dtype == torch.int64 and got.numpy().tolist() == want.tolist()
    if b * s * s >= len(IDS):
        assert want[:, 2].all() and (want[:, 1] > want[:, 0]).all(), "a region without a real or a wrongly predicted pixel checks less"
    per, mean = m.compute()
    ref_per, ref_mean = R.jaccard(want)
    assert per == [float(p) for p in ref_per] and abs(mean - float(ref_mean)) <= 1e-15


def test_unaligned_views_fall_back_to_the_scalar_path():
    """S*S = 64 would take the 16-byte loads, but the mask starts 4 bytes (and then the labels 1 byte) past an aligned address."""
    from where2edit_amd.evaluation import celebamask_mapping, mask_iou_counts, region_lut
    b, t, s = 2, 8, 8
    masks, ids = _problem(b, t, s, seed=7)
    want = R.confusion_counts(masks, ids, t)
    lut = region_lut(celebamask_mapping(), t).to(DEV)
    flat = torch.zeros(masks.size + 1, device=DEV)
    flat[1:] = torch.from_numpy(masks).to(DEV).reshape(-1)
    view = flat[1:].view(b, t, s, s)
    lab = torch.from_numpy(ids).to(DEV)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and lab.data_ptr() % 4 == 0
    counts = torch.zeros((t, 3), dtype=torch.int64, device=DEV)
    mask_iou_counts(view, lab, lut, 0.8, counts)
    assert counts.cpu().numpy().tolist() == want.tolist()
    lflat = torch.zeros(ids.size + 1, dtype=torch.uint8, device=DEV)
    lflat[1:] = lab.reshape(-1)
    lview = lflat[1:].view(b, s, s)
    assert lview.data_ptr() % 4 == 1 and flat[4:].data_ptr() % 16 == 0
    aligned = torch.from_numpy(masks).to(DEV)
    assert aligned.data_ptr() % 16 == 0
    counts.zero_()
    mask_iou_counts(aligned, lview, lut, 0.8, counts)
    assert counts.cpu().numpy().tolist() == want.tolist()


@pytest.mark.parametrize("s", [8, 5])  # the vector and the scalar path
def test_threshold_edge_values(s):
    """float32(0.8) itself is predicted (the reference's two writes amount to m >= 0.8f), its lower neighbour is not, NaN is not,
    +inf is, -inf is not."""
    f = np.float32(0.8)
    special = np.array([f, np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(1)), 0.75, np.nan, np.inf, -np.inf, 1.0], dtype=np.float32)
    predicted = [1, 0, 1, 0, 0, 1, 0, 1]
    b, t = 2, 8
    n = b * s * s
    planes = np.repeat(special[None, :, None], n // b, 2).reshape(1, t, s, s).repeat(b, 0)  # plane k holds special[k] everywhere
    rolled = np.stack([np.roll(special, k)[np.arange(n) % 8] for k in range(t)], 0).reshape(t, b, s, s).transpose(1, 0, 2, 3).copy()
    _, ids = _problem(b, t, s, seed=3)
    for masks in (planes, rolled):
        m = _metric(t)
        m.update(torch.from_numpy(masks).to(DEV), torch.from_numpy(ids).to(DEV))
        got = m.counts().numpy()
        assert got.tolist() == R.confusion_counts(masks, ids, t).tolist()
        if masks is planes:
            assert got[:, 1].tolist() == [n * p for p in predicted]


def test_two_updates_equal_one_update_on_the_concatenation_and_labels_in_either_form():
    b, t, s = 4, 8, 10
    masks, ids = _problem(b, t, s, seed=21)
    mk, lab = torch.from_numpy(masks).to(DEV), torch.from_numpy(ids).to(DEV)
    one, two = _metric(t), _metric(t)
    one.update(mk, lab)
    two.update(mk[:1], lab[:1].unsqueeze(1))                          # [B,1,S,S]
    two.update(mk[1:], lab[1:].to(torch.float32).div(255))            # what ToTensor makes of the label image
    assert torch.equal(one.counts(), two.counts())
    assert one.counts().numpy().tolist() == R.confusion_counts(masks, ids, t).tolist()
    two.reset()
    assert not two.counts().any()
    two.update(mk, lab.long())
    assert torch.equal(one.counts(), two.counts())


def test_the_accumulator_is_64_bit():
    b, t, s = 2, 8, 8
    masks, ids = _problem(b, t, s, seed=5)
    m = _metric(t)
    m.update(torch.from_numpy(masks).to(DEV), torch.from_numpy(ids).to(DEV))
    batch = m.counts()
    m._counts.fill_(2 ** 33 + 5)
    m.update(torch.from_numpy(masks).to(DEV), torch.from_numpy(ids).to(DEV))
    assert torch.equal(m.counts(), batch + (2 ** 33 + 5))


def test_counts_are_bit_identical_from_run_to_run_also_when_deterministic():
    import where2edit_amd
    b, t, s = 6, 8, 64  # 24 workgroups adding into the same 24 counters
    masks, ids = _problem(b, t, s, seed=9)
    mk, lab = torch.from_numpy(masks).to(DEV), torch.from_numpy(ids).to(DEV)
    runs = []
    try:
        for det in (False, False, True, True):
            where2edit_amd.set_deterministic(det)
            m = _metric(t)
            m.update(mk, lab)
            runs.append(m.counts())
    finally:
        where2edit_amd.set_deterministic(False)
    assert all(torch.equal(runs[0], r) for r in runs[1:])
    assert runs[0].numpy().tolist() == R.confusion_counts(masks, ids, t).tolist()


# ---- the mask-only entry of the net and the driver -------------------------------------------------------------------------

def test_net_mask_is_the_second_output_of_forward_bit_for_bit():
    import test_gpu_attention as TA
    from where2edit_amd import attention_with_text, binarise
    net, _ = TA._net()
    x, att_text, _ = M.inputs()
    x, att_text = [t.to(DEV) for t in x], att_text.to(DEV)
    feats = [f.to(DEV) for f in M.feature_maps()]
    _, final, _ = net(x, feats, M.SIZE, attention_text=att_text)
    mask = net.mask(feats, M.SIZE, att_text, len(x))
    assert mask.shape == (M.BATCH, 1, M.SIZE, M.SIZE) and not mask.requires_grad and torch.equal(mask, final)
    assert 0 < int((mask >= 0.8).sum()) < mask.numel(), "a constant mask would make the next comparison empty"
    # attention_with_text: the binarised mask, from S-space codes (a list) or from a W+ tensor of the matching depth
    want = binarise(mask)
    assert set(want.unique().tolist()) == {0.0, 1.0}
    codes = [c[:, :, 512:].unsqueeze(3).unsqueeze(3) for c in x]
    assert torch.equal(attention_with_text(net, att_text, codes, feats, M.ATT_LAYER), want)
    assert torch.equal(attention_with_text(net, att_text[:1], torch.zeros(M.BATCH, M.LAYERS, 512, device=DEV), feats, M.ATT_LAYER), want)


@pytest.fixture(scope="module")
def pair():
    """G(256) + the seeded net of tests/test_gpu_attention.py (14 latents, 20 codes, mask at layer 7 = 16 x 16), deterministic
    kernels: a mask pixel within rounding of the threshold must not flip between two runs of the same generator pass."""
    import test_gpu_attention as TA
    import where2edit_amd
    from where2edit_amd.attention_model import Generator
    g = Generator(256, 512, 8)
    g.load_state_dict(seeded.generator_state_dict(256), strict=True)
    g = g.to(DEV).eval().requires_grad_(False)
    net, _ = TA._net()
    where2edit_amd.set_deterministic(True)
    yield g, net.requires_grad_(False)
    where2edit_amd.set_deterministic(False)


def _hand_masks(g, net, w, text):
    """[B,T,S,S] soft masks from the pieces other tests pin: style codes, G with features (+ const input), net.mask per prompt."""
    with torch.no_grad():
        _, styles = g.style_codes([w], input_is_latent=True)
        _, _, _, feats = g([styles], input_is_latent=True, randomize_noise=False, return_features=True, input_is_stylespace=True)
        feats = list(feats) + [g.input.input.repeat(w.shape[0], 1, 1, 1)]
        return torch.cat([net.mask(feats, M.SIZE, text[j:j + 1].repeat(w.shape[0], 1), len(styles)) for j in range(text.shape[0])], 1)


def test_calculate_iou_on_latents_equals_the_pieces_called_by_hand(pair):
    from where2edit_amd import calculate_iou
    g, net = pair
    t = 3
    mapping = {1: 1, 2: 2, 4: 3, 5: 3, 13: 2}
    w = seeded.wplus_latents(2, g.n_latent, salt=61).to(DEV)
    text = seeded.tensor("iou.text", (t, 512), 0.3).to(DEV)
    ids = np.random.RandomState(4).choice([0, 1, 2, 4, 5, 13, 17], size=(2, M.SIZE, M.SIZE)).astype(np.uint8)
    lab = torch.from_numpy(ids).to(torch.float32).div(255).unsqueeze(1)  # [B,1,S,S] floats on the CPU, as a loader yields them
    hand = torch.cat([_hand_masks(g, net, w[i:i + 1], text) for i in range(2)]).cpu().numpy()
    assert hand.max() > hand.min()
    thr = (float(hand.min()) + float(hand.max())) / 2  # splits these masks, whatever the seeded net makes of the seeded generator
    share = float((hand >= np.float32(thr)).mean())
    print(f"calculate_iou test: masks in [{hand.min():.3f}, {hand.max():.3f}], threshold {thr:.3f}, predicted share {share:.3f}")
    assert 0 < share < 1
    kw = dict(attention_layer=M.ATT_LAYER, threshold=thr, mapping=mapping)
    samples = [(w[i:i + 1].cpu(), lab[i:i + 1]) for i in range(2)]
    per, mean = calculate_iou(samples, g, net, text, **kw)
    ref_per, ref_mean = R.jaccard(R.confusion_counts(hand, ids, t, threshold=thr, mapping=mapping))
    assert per == [float(p) for p in ref_per] and abs(mean - float(ref_mean)) <= 1e-15
    # it stops at max_images: between batches, and inside one
    first = R.jaccard(R.confusion_counts(hand[:1], ids[:1], t, threshold=thr, mapping=mapping))
    seen = []

    def counted():
        for s in samples:
            seen.append(1)
            yield s

    per1, mean1 = calculate_iou(counted(), g, net, text, max_images=1, **kw)
    assert per1 == [float(p) for p in first[0]] and len(seen) <= 2
    per1b, _ = calculate_iou([(w.cpu(), lab)], g, net, text, max_images=1, **kw)
    assert per1b == per1
    assert per1 != per, "the second image changed nothing: the stop would go unnoticed"


def test_calculate_iou_image_path_equals_the_latent_path_fed_with_the_encoders_output(pair):
    """256^2 images through a seeded e4e (IR-SE50, 14 styles for the 256^2 generator) with the latent-average hook of
    load_e4e_standalone, against calculate_iou on the W+ latents that encoder returns."""
    import types
    import make_golden_e4e as ME
    from where2edit_amd import calculate_iou
    from where2edit_amd.psp_encoders import Encoder4Editing
    g, net = pair
    e4e = Encoder4Editing(50, "ir_se", types.SimpleNamespace(stylegan_size=256)).eval()
    e4e.load_state_dict(ME.encoder_state_dict(e4e.state_dict()), strict=True)
    e4e = e4e.to(DEV).requires_grad_(False)
    avg = seeded.tensor("iou.latent_avg", (g.n_latent, 512), 0.2).to(DEV)
    e4e.register_forward_hook(lambda model, inputs, outputs: outputs + avg.repeat(outputs.shape[0], 1, 1))
    img = seeded.tensor("iou.img", (2, 3, 256, 256), 0.5)
    text = seeded.tensor("iou.text8", (8, 512), 0.3).to(DEV)
    ids = np.random.RandomState(6).choice(IDS, size=(2, M.SIZE, M.SIZE)).astype(np.uint8)
    lab = torch.from_numpy(ids)
    with torch.no_grad():
        w = e4e(img.to(DEV))
    assert w.shape == (2, g.n_latent, 512)
    a = calculate_iou([(img, lab)], g, net, text, attention_layer=M.ATT_LAYER, e4e=e4e)
    b = calculate_iou([(w, lab)], g, net, text, attention_layer=M.ATT_LAYER)
    assert a == b and len(a[0]) == 8
    with pytest.raises(RuntimeError, match="pass e4e"):
        calculate_iou([(img, lab)], g, net, text, attention_layer=M.ATT_LAYER)
