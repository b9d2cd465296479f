"""The region mask's IoU against CelebAMask-HQ parsing labels: `calculate_IOU` / `attention_with_text` of the reference
(utils.py:639-726) on this package's kernels.

For eight fixed prompts the reference predicts one mask per test image, binarises it (`m[m < 0.8] = 0; m[m > 0.7] = 1`), remaps the
parsing label to eight regions, moves everything to the host as a [N*S*S, 8] one-hot matrix and calls scikit-learn's `jaccard_score`.
Here the expensive stages (e4e, G with features, the mask branch) are the kernels the training loop already runs, the mask branch
runs alone (`net.mask`: the reference runs the whole Mapper per prompt and drops the styles), and the confusion counts are one
streaming kernel (`w2e_mask_iou_counts`: binarisation, label remap and the three counts per region in one pass, accumulated in a
[T,3] int64 table on the device).  Nothing moves to the host before `MaskIoU.compute()`, which copies 3*T integers.

Callers bring the dataset: `(image or W+ latent, parsing label already resized to the mask's S x S)` pairs, and the CLIP text
features of the prompts (there is no tokeniser in this package).  Decoded bytes are welcome too: uint8 [B,H,W,3] images and, with
`calculate_iou(label_resize=...)`, uint8 labels of any size are resized on the device with Pillow's own arithmetic (image_io.py).

Second half: the quality metrics of edits, `cal_evaluation` / `generate_imgs` (utils.py:434-551) -- Inception Score, FID, identity
similarity and the share of edits whose CLIP score improves: `calculate_metrics`, `EditMetrics`, `fid_from_features`,
`isc_from_logits`, on inception.FeatureExtractorInceptionV3."""
import ctypes

import torch

from ._lib import call, ptr, stream_ptr

# CelebAMask-HQ's parsing ids, in the order the dataset's label list gives them (id = index).
CELEBAMASK_LABELS = ("background", "skin", "nose", "eye_g", "l_eye", "r_eye", "l_brow", "r_brow", "l_ear", "r_ear", "mouth", "u_lip",
                     "l_lip", "hair", "hat", "ear_r", "neck_l", "neck", "cloth")

# (region name, the prompt evaluated against it, the parsing labels it is made of); region ids are 1-based in this order, 0 = none
# (utils.py:677 for the prompts, :702-715 for the remap).
CELEBAMASK_REGIONS = (
    ("skin", "rosy cheeks", ("skin",)),
    ("nose", "big nose", ("nose",)),
    ("eyes", "brown eyes", ("l_eye", "r_eye")),
    ("eyebrows", "bushy eyebrows", ("l_brow", "r_brow")),
    ("ears", "large ears", ("l_ear", "r_ear")),
    ("mouth", "mouths are slightly open", ("mouth",)),
    ("lips", "pink lipsticks", ("u_lip", "l_lip")),
    ("hair", "blonde hair", ("hair",)),
)


def celebamask_mapping():
    """{raw parsing id: region id in 1..8} of CELEBAMASK_REGIONS; every id that is not listed belongs to no region."""
    return {CELEBAMASK_LABELS.index(name): r + 1 for r, (_, _, parts) in enumerate(CELEBAMASK_REGIONS) for name in parts}


def region_lut(mapping, classes):
    """The 256-entry table `w2e_mask_iou_counts` reads: uint8 [256] on the CPU, lut[raw id] = region in 0..classes (0 = none).
    `mapping`: {raw id: region}.  A raw id outside 0..255 or a region outside 0..classes is refused here -- the kernel does not
    look at the table's values again."""
    if not 1 <= int(classes) <= 16:
        raise ValueError(f"region_lut: 1 <= classes <= 16 (got {classes})")
    lut = torch.zeros(256, dtype=torch.uint8)
    for raw, region in mapping.items():
        if not (isinstance(raw, int) and 0 <= raw <= 255):
            raise ValueError(f"region_lut: raw parsing id {raw!r} is not an integer in 0..255")
        if not (isinstance(region, int) and 0 <= region <= classes):
            raise ValueError(f"region_lut: raw id {raw} maps to region {region!r}, but there are {classes} regions: regions are "
                             f"1..{classes} (0 = none); pass classes >= {region!r} or drop the entry")
        lut[raw] = region
    return lut


def _f32(x):
    """x rounded to fp32, as a Python float: comparing an fp32 tensor against it gives the fp32 comparison whatever precision the
    comparison itself is carried out in."""
    return ctypes.c_float(float(x)).value


def binarise(mask, threshold=0.8):
    """The reference's `m[m < 0.8] = 0; m[m > 0.7] = 1` (utils.py:649-650) as one expression: 1 where mask >= float32(threshold), else
    0 (a NaN, which the two writes would leave in place, becomes 0).  Same shape and dtype as `mask`."""
    return (mask >= _f32(threshold)).to(mask.dtype)


def labels_to_ids(labels):
    """Parsing labels as uint8 ids.  Float labels are taken to be ToTensor's id / 255 and converted as the reference does
    (utils.py:702: (label * 255).type(torch.int)), which is exact for all 256 ids in fp32; integer labels are ids already."""
    if labels.is_floating_point():
        return (labels * 255).to(torch.int).to(torch.uint8)
    return labels.to(torch.uint8)


def mask_iou_counts(masks, labels, lut, threshold, counts):
    """counts [T,3] int64 += the confusion counts of masks [B,T,S,S] (fp32, contiguous) against labels uint8 [B,S,S] through lut
    uint8 [256] (w2e_mask_iou_counts); everything on the current GPU.  No copies are made of the arguments."""
    b, t, s, s2 = masks.shape
    for what, x, dt, shape in (("labels", labels, torch.uint8, (b, s, s)), ("lut", lut, torch.uint8, (256,)), ("counts", counts, torch.int64, (t, 3))):
        if not (x.is_cuda and x.device == masks.device and x.dtype == dt and tuple(x.shape) == shape and x.is_contiguous()):
            raise RuntimeError(f"mask_iou_counts: {what} must be a contiguous {dt} tensor of shape {shape} on {masks.device} "
                               f"(got {x.dtype} {tuple(x.shape)} on {x.device})")
    if s != s2:
        raise RuntimeError(f"mask_iou_counts: masks are [B,T,S,S] (got {tuple(masks.shape)})")
    call("w2e_mask_iou_counts", ptr(masks), ctypes.c_void_p(labels.data_ptr() if b else 16), ctypes.c_void_p(lut.data_ptr()),
         _f32(threshold), b, t, s, ctypes.c_void_p(counts.data_ptr()), stream_ptr())
    return counts


class MaskIoU:
    """Streaming Jaccard scores of T predicted masks against T label regions: `update` adds a batch's confusion counts to a [T,3]
    int64 table on the device (one kernel, no host synchronisation), `compute` copies the table and returns what
    `sklearn.metrics.jaccard_score(real, pred, average=None / 'macro')` returns on the one-hot matrices of utils.py:716-724.
    `mapping`: {raw parsing id: region 1..T}; the CelebAMask-HQ table by default (then `classes` must be at least 8)."""

    def __init__(self, classes=8, threshold=0.8, mapping=None, device="cuda"):
        self.classes, self.threshold = int(classes), float(threshold)
        if self.threshold != self.threshold:
            raise ValueError("MaskIoU: the threshold is NaN")
        lut = region_lut(celebamask_mapping() if mapping is None else mapping, self.classes)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"MaskIoU runs on the GPU only (got device='{self.device}'): pass device='cuda'")
        self._lut_host, self._lut, self._counts = lut, None, None  # (the device tensors are made by the first update)

    def _table(self):
        if self._counts is None:
            self._lut = self._lut_host.to(self.device)
            self._counts = torch.zeros((self.classes, 3), dtype=torch.int64, device=self.device)
        return self._counts

    def reset(self):
        if self._counts is not None:
            self._counts.zero_()

    def update(self, masks, labels):
        """masks [B,T,S,S] (soft or binary; a pixel is predicted where mask >= threshold); labels [B,S,S] or [B,1,S,S], uint8 /
        integer ids or float id / 255, already at S x S."""
        if masks.ndim != 4 or masks.shape[1] != self.classes or masks.shape[2] != masks.shape[3]:
            raise RuntimeError(f"MaskIoU.update: masks must be [B, {self.classes}, S, S], one mask per region (got {tuple(masks.shape)})")
        b, _, s, _ = masks.shape
        if labels.ndim == 4 and labels.shape[1] == 1:
            labels = labels[:, 0]
        if tuple(labels.shape) != (b, s, s):
            raise RuntimeError(f"MaskIoU.update: labels are {tuple(labels.shape)} but the masks are {s} x {s} for a batch of {b}: resize "
                               f"the labels to {s} x {s} (nearest) before calling update -- labels must be [B,S,S] or [B,1,S,S]")
        if not (masks.is_cuda and labels.is_cuda):
            raise RuntimeError("MaskIoU.update: masks and labels must be on the GPU (got "
                               f"{masks.device} and {labels.device}): move them with .to('{self.device}') first")
        with torch.cuda.device(masks.device):
            counts = self._table()
            mask_iou_counts(masks.detach().float().contiguous(), labels_to_ids(labels).contiguous(), self._lut, self.threshold, counts)

    def counts(self):
        """The raw table as an int64 [T,3] CPU tensor: per region (intersection, predicted, real) pixel counts.  Synchronises."""
        return self._table().cpu()

    def compute(self):
        """(per-region IoU: T floats, their plain mean).  IoU = inter / (pred + real - inter), 0 where that union is empty --
        what jaccard_score returns there (with a warning); the mean is over all T regions, empty ones included."""
        per = []
        for inter, pred, real in self.counts().tolist():
            union = pred + real - inter
            per.append(inter / union if union else 0.0)
        return per, sum(per) / len(per)


def n_style_codes(n_latent):
    """S-space codes of a generator with `n_latent` W+ rows: one per conv layer and ToRGB (18 -> 26)."""
    return n_latent + (n_latent - 2) // 2


def _codes_dims(codes):
    """(batch, n_codes) of S-space codes (a list of [B,1,C,1,1]) or of a W+ tensor [B,n_latent,512]."""
    if torch.is_tensor(codes):
        return codes.shape[0], n_style_codes(codes.shape[1])
    return codes[0].shape[0], len(codes)


@torch.no_grad()
def attention_with_text(net, text_features, codes, feature_map, attention_layer):
    """utils.py:639-651: the binary mask [B,1,S,S] (S = the resolution of feature_map[attention_layer - 1]) of `net` for the prompt
    with CLIP features `text_features` ([B,512] or [1,512]).  `codes` -- the S-space codes (a list) or the W+ tensor -- only tells the
    number of codes and the batch: the mask branch does not read the styles.  (Argument order: the net first, no work_in_stylespace
    flag -- the type of `codes` says it.)"""
    batch, n_codes = _codes_dims(codes)
    size = feature_map[attention_layer - 1].shape[-1]
    if text_features.shape[0] != batch:
        text_features = text_features[:1].repeat(batch, 1)
    return binarise(net.mask(feature_map, size, text_features, n_codes)).view(batch, 1, size, size)


@torch.no_grad()
def calculate_iou(samples, g_ema, mapper, text_features, *, attention_layer=13, e4e=None, max_images=90, threshold=0.8,
                  work_in_stylespace=True, mapping=None, label_resize=None):
    """utils.py:654-726.  `samples` yields (x, label): x = [B,3,256,256] images or uint8 [B,H,W,3] decoded images of any size (they go
    through image_io.to_tensor(x, 256) = transform_img(256, ...); for both `e4e`, e.g. psp_encoders.load_e4e_standalone's, is
    required) or, with e4e=None, W+ latents [B,n_latent,512]; label = the parsing label at the mask's resolution (MaskIoU.update).
    label_resize: None -- labels come at the mask's S x S (a mismatch is MaskIoU.update's error); "bilinear" / "nearest" -- labels are
    uint8 ids [B,H,W] or [B,1,H,W] of any size and are resized to S x S by image_io.label_ids.  "bilinear" is the REFERENCE-EXACT
    choice: transform_label resizes the mode-L label PNG with Pillow's antialiased bilinear filter, so ids blend at region borders
    (a pixel between skin = 1 and hair = 13 gets some id in between, e.g. 7 = r_brow) and `label == k` keeps only the exact hits;
    use it to reproduce the reference's numbers.  "nearest" is the sensible choice: every pixel keeps an id that was there.
    text_features [T,512]: the CLIP text features of the T prompts (CELEBAMASK_REGIONS lists the reference's eight), one region each;
    `mapping` as for MaskIoU (a T other than 8 needs its own).  Stops after `max_images` images (the reference: 90 batches of 1).
    Returns (per-region IoU, mean IoU).  One generator pass with features per batch, one mask-branch pass per prompt over the same
    feature maps; the host first waits for the device in the final `compute()`."""
    if not text_features.is_floating_point():
        raise RuntimeError("calculate_iou: text_features are the CLIP text features [T,512] of the prompts; encode token ids with the "
                           "CLIP model's encode_text first")
    if label_resize not in (None, "bilinear", "nearest"):
        raise ValueError(f"calculate_iou: label_resize is None, 'bilinear' or 'nearest' (got {label_resize!r})")
    dev = text_features.device
    n_prompts = text_features.shape[0]
    metric = MaskIoU(classes=n_prompts, threshold=threshold, mapping=mapping, device=dev)
    text_features = text_features.float()
    seen = 0
    for x, label in samples:
        if seen >= max_images:
            break
        x, label = x[:max_images - seen].to(dev, non_blocking=True), label[:max_images - seen].to(dev, non_blocking=True)
        batch = x.shape[0]
        if x.dtype == torch.uint8:
            if e4e is None:
                raise RuntimeError(f"calculate_iou: uint8 samples of shape {tuple(x.shape)} are decoded images [B,H,W,3]: pass e4e=...")
            from .image_io import to_tensor
            x = to_tensor(x, 256)
        if e4e is not None:
            w = e4e(x)
        elif x.ndim == 3:
            w = x
        else:
            raise RuntimeError(f"calculate_iou: samples of shape {tuple(x.shape)} are images: pass e4e=...; without it x is W+ [B,n_latent,512]")
        if hasattr(g_ema, "style_codes"):  # the codes alone: the reference runs the whole generator here and drops the image
            latents, styles = g_ema.style_codes([w], input_is_latent=True)
        else:
            _, latents, styles = g_ema([w], input_is_latent=True, return_latents=True, randomize_noise=False)
        codes = styles if work_in_stylespace else latents
        _, _, _, feats = g_ema([codes], input_is_latent=True, randomize_noise=False, return_features=True, input_is_stylespace=work_in_stylespace)
        feats = list(feats) + [g_ema.input.input.repeat(batch, 1, 1, 1)]
        size = feats[attention_layer - 1].shape[-1]
        n_codes = _codes_dims(codes)[1]
        masks = torch.cat([mapper.mask(feats, size, text_features[j:j + 1].repeat(batch, 1), n_codes) for j in range(n_prompts)], 1)
        if label_resize is not None:
            from .image_io import label_ids
            if label.ndim == 4 and label.shape[1] == 1:
                label = label[:, 0]
            label = label_ids(label.contiguous(), size, label_resize)
        metric.update(masks, label)  # (binarisation happens inside the counting kernel)
        seen += batch
    return metric.compute()


def celebamask_samples(img_dir, label_dir, batch=8, device=None):
    """The samples of `calculate_iou` from CelebAMask-HQ as the reference lays it out (utils.py:570-587): image i is
    `img_dir/{i}.jpg`, its parsing label `label_dir/{i}.png`, i = 0 .. (number of files in img_dir) - 1.  A generator of
    (uint8 [B,H,W,3] images, uint8 [B,H,W] label ids), both decoded on the GPU (image_io.from_jpeg / from_png(mode="raw")), `batch`
    files at a time.  With calculate_iou(..., e4e=..., label_resize="bilinear") the evaluation runs from the files to the IoU without
    Pillow."""
    import os

    from .image_io import from_jpeg, from_png
    if not (isinstance(batch, int) and batch >= 1):
        raise ValueError(f"celebamask_samples: batch is a positive integer (got {batch!r})")
    count = len([name for name in os.listdir(img_dir) if os.path.isfile(os.path.join(img_dir, name))])

    def read(path):
        with open(path, "rb") as f:
            return f.read()

    for first in range(0, count, batch):
        ids = range(first, min(first + batch, count))
        images = from_jpeg([read(os.path.join(img_dir, f"{i}.jpg")) for i in ids], device=device, stack=True)
        labels = from_png([read(os.path.join(label_dir, f"{i}.png")) for i in ids], mode="raw", device=device, stack=True)
        if labels.ndim != 3:
            raise ValueError(f"celebamask_samples: the labels {first}.png .. are no grey or palette files (decoded shape {tuple(labels.shape)})")
        yield images, labels


# ---------------------------------------------------------------------------------------------- FID / Inception Score
# utils.py:434-551 (cal_evaluation / generate_imgs): the reference writes the original and the edited images as quality-75 JPEG files
# and hands the two directories to torch_fidelity.calculate_metrics(isc=True, fid=True).  The feature extractor is
# inception.FeatureExtractorInceptionV3 on its HIP kernels; the two statistics below are float64 torch compositions over [N,2048] /
# [N,1008] matrices -- plumbing, computed on the host (no dependence on the ROCm build's eigh).
def _feature_matrix(f, what):
    f = torch.as_tensor(f).detach().to("cpu", torch.float64)
    if f.dim() != 2 or f.shape[0] < 2:
        raise ValueError(f"{what}: features are [N,D] with N >= 2 (got {tuple(f.shape)})")
    return f


def feature_statistics(f):
    """(mean [D], covariance [D,D] with N - 1) of features [N,D], float64."""
    f = _feature_matrix(f, "feature_statistics")
    mu = f.mean(0)
    d = f - mu
    return mu, d.T @ d / (f.shape[0] - 1)


def fid_from_statistics(mu1, s1, mu2, s2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^1/2.  The trace comes from eigenvalues, without a matrix square root of the
    unsymmetric product: with R = S1^1/2 (eigh, eigenvalues clamped at 0) the matrices S1 S2 and R S2 R share their spectrum and the
    latter is symmetric positive semi-definite, so tr (S1 S2)^1/2 = sum sqrt(eigvalsh(R S2 R)), clamped at 0.
    R S2 R is formed in S1's eigenbasis, on the eigenvectors above S1's numerical rank tolerance (D eps lambda_max, matrix_rank's)
    only: the rest contribute exactly 0 to R, but as rows and columns of rounding noise of size eps they would each add sqrt(eps) to
    the trace -- with fewer samples than dimensions that is most of them, and a set's distance to itself would not be 0."""
    mu1, s1, mu2, s2 = (torch.as_tensor(t).to("cpu", torch.float64) for t in (mu1, s1, mu2, s2))
    lam, q = torch.linalg.eigh(s1)
    keep = lam > lam.max().clamp_min(0) * lam.numel() * torch.finfo(torch.float64).eps
    h = q[:, keep] * lam[keep].sqrt()  # R = h q_keep^T, so R S2 R = q_keep (h^T S2 h) q_keep^T: the same non-zero spectrum
    m = h.T @ s2 @ h
    tr = torch.linalg.eigvalsh((m + m.T) / 2).clamp_min(0).sqrt().sum()
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(s1) + torch.trace(s2) - 2 * tr)


def fid_from_features(f1, f2):
    """The Frechet distance of two feature sets [N1,D], [N2,D] (torch_fidelity's frechet_inception_distance on the '2048' features)."""
    return fid_from_statistics(*feature_statistics(f1), *feature_statistics(f2))


def isc_from_logits(logits, splits=10, shuffle=True, rng_seed=2020):
    """torch_fidelity's Inception Score of the UNBIASED logits [N,1008]: (mean, population standard deviation) over `splits` of
    exp(mean_i sum_c p_ic (log p_ic - log mean_i p_ic)); the rows are first permuted by numpy.random.RandomState(rng_seed), split k
    holds rows [k N // splits, (k + 1) N // splits).  float64."""
    import numpy as np
    x = torch.as_tensor(logits).detach().to("cpu", torch.float64)
    if x.dim() != 2 or not 1 <= splits <= x.shape[0]:
        raise ValueError(f"isc_from_logits: logits are [N,C] with N >= splits >= 1 (got {tuple(x.shape)}, splits {splits})")
    n = x.shape[0]
    if shuffle:
        x = x[torch.from_numpy(np.random.RandomState(rng_seed).permutation(n))]
    logp = torch.log_softmax(x, dim=1)
    scores = []
    for k in range(splits):
        lp = logp[k * n // splits:(k + 1) * n // splits]
        p = lp.exp()
        log_marginal = p.mean(0, keepdim=True).log()
        scores.append((p * (lp - log_marginal)).sum(1).mean().exp())
    scores = torch.stack(scores)
    return float(scores.mean()), float(scores.std(unbiased=False))


_IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png")


def _image_batches(source, batch, device):
    """uint8 [b,H,W,3] batches on the GPU of one `calculate_metrics` input: a uint8 tensor [N,H,W,3] (or [H,W,3]), a list of such
    tensors, or a directory of .jpg / .png files (sorted by name, decoded by image_io.read_image, grouped by size)."""
    import os
    if isinstance(source, (str, os.PathLike)):
        from .image_io import read_image
        names = sorted(n for n in os.listdir(source) if os.path.splitext(n)[1].lower() in _IMAGE_SUFFIXES)
        if not names:
            raise ValueError(f"calculate_metrics: no .jpg / .png file in {os.fspath(source)!r}")
        source = [read_image(os.path.join(source, n), device=device) for n in names]
    if torch.is_tensor(source):
        source = [source]
    groups = {}
    for t in source:
        if not (torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() in (3, 4) and t.shape[-1] == 3):
            raise ValueError("calculate_metrics: an input is a uint8 tensor [N,H,W,3], a list of uint8 [H,W,3] / [N,H,W,3] tensors, or a directory "
                             f"(got {type(t).__name__}{'' if not torch.is_tensor(t) else f' {t.dtype} {tuple(t.shape)}'})")
        t = t[None] if t.dim() == 3 else t
        groups.setdefault(tuple(t.shape[1:3]), []).append(t)
    for members in groups.values():
        images = members[0] if len(members) == 1 else torch.cat(members)
        for first in range(0, images.shape[0], batch):
            yield images[first:first + batch].to(device)


def inception_features(source, extractor, batch=32, features=("2048", "logits_unbiased")):
    """The named features of every image of `source` (see `_image_batches`), each [N,D] on the extractor's device."""
    device = next(extractor.parameters()).device
    chunks = [[] for _ in features]
    with torch.cuda.device(device):
        for images in _image_batches(source, batch, device):
            for acc, f in zip(chunks, extractor(images, features=features)):
                acc.append(f)
    return tuple(torch.cat(c) for c in chunks)


def calculate_metrics(input1, input2, isc=True, fid=True, batch=32, extractor=None, isc_splits=10):
    """torch_fidelity.calculate_metrics(input1, input2, isc=, fid=) (utils.py:545-550): the Inception Score of input1 and the Frechet
    Inception Distance between the two inputs, under torch_fidelity's keys.  Each input: a uint8 [N,H,W,3] tensor, a list of uint8
    tensors, or a directory of .jpg / .png files (read on the GPU, grouped by size into batches of at most `batch`).  extractor: a
    FeatureExtractorInceptionV3 on the GPU with the pretrained weights loaded; None builds one with its seeded random weights, whose
    numbers are comparable only with each other.  isc_splits: torch_fidelity's keyword of that name (input1 needs that many images)."""
    if extractor is None:
        from .inception import FeatureExtractorInceptionV3
        extractor = FeatureExtractorInceptionV3().to("cuda")
    if not (isinstance(batch, int) and batch >= 1):
        raise ValueError(f"calculate_metrics: batch is a positive integer (got {batch!r})")
    out = {}
    f1, l1 = inception_features(input1, extractor, batch)
    if isc:
        out["inception_score_mean"], out["inception_score_std"] = isc_from_logits(l1, splits=isc_splits)
    if fid:
        (f2,) = inception_features(input2, extractor, batch, features=("2048",))
        out["frechet_inception_distance"] = fid_from_features(f1, f2)
    return out


def _images_in_order(source, device, what):
    """The images of one `lpips_distance` input as a list of uint8 [H,W,3] tensors, in order: a uint8 tensor [N,H,W,3] (or [H,W,3]),
    a list of such tensors, or a directory of .jpg / .png files (sorted by name, decoded by image_io.read_image on `device`)."""
    import os
    if isinstance(source, (str, os.PathLike)):
        from .image_io import read_image
        names = sorted(n for n in os.listdir(source) if os.path.splitext(n)[1].lower() in _IMAGE_SUFFIXES)
        if not names:
            raise ValueError(f"lpips_distance: no .jpg / .png file in {os.fspath(source)!r}")
        source = [read_image(os.path.join(source, n), device=device) for n in names]
    if torch.is_tensor(source):
        source = [source]
    images = []
    for t in source:
        if not (torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() in (3, 4) and t.shape[-1] == 3):
            raise ValueError(f"lpips_distance: {what} is a uint8 tensor [N,H,W,3], a list of uint8 [H,W,3] / [N,H,W,3] tensors, or a directory "
                             f"(got {type(t).__name__}{'' if not torch.is_tensor(t) else f' {t.dtype} {tuple(t.shape)}'})")
        images += [t] if t.dim() == 3 else list(t.unbind(0))
    return images


@torch.no_grad()
def lpips_distance(input1, input2, model=None, batch=32):
    """LPIPS of paired images -- original against edit: how much changed.  input1 / input2: what `calculate_metrics` takes (a uint8
    [N,H,W,3] tensor, a list of uint8 tensors, or a directory of .jpg / .png files read on the GPU); image i of input1 is paired with
    image i of input2, so the counts must agree and so must the two sizes of every pair.  The bytes become [-1, 1] tensors through
    image_io.to_tensor (no resize) and go through `model` in batches of at most `batch` consecutive pairs of one size.
    Returns {"lpips_mean": float, "lpips": fp32 tensor [N] on the model's device}; the float is the one host synchronisation.
    model: an lpips.LPIPS on the GPU with the published weights loaded.  None builds one with its SEEDED RANDOM weights: such numbers
    rank edits of one run against each other and are no LPIPS of the literature (lpips.py says what to load)."""
    if not (isinstance(batch, int) and batch >= 1):
        raise ValueError(f"lpips_distance: batch is a positive integer (got {batch!r})")
    device = torch.device("cuda") if model is None or not hasattr(model, "parameters") else next(model.parameters()).device
    first, second = _images_in_order(input1, device, "input1"), _images_in_order(input2, device, "input2")
    if len(first) != len(second):
        raise ValueError(f"lpips_distance: input1 holds {len(first)} images, input2 {len(second)}: pairs are by order, the counts must agree")
    for i, (a, b) in enumerate(zip(first, second)):
        if a.shape != b.shape:
            raise ValueError(f"lpips_distance: pair {i} has sizes {tuple(a.shape[:2])} and {tuple(b.shape[:2])}: resize one side first")
    if not first:
        raise ValueError("lpips_distance: no images")
    if model is None:
        from .lpips import LPIPS
        model = LPIPS().to(device)
    from .image_io import to_tensor
    out, i = [], 0
    with torch.cuda.device(device):
        while i < len(first):
            j = i + 1
            while j < len(first) and j - i < batch and first[j].shape == first[i].shape:
                j += 1
            x0 = to_tensor(torch.stack(first[i:j]).to(device))
            x1 = to_tensor(torch.stack(second[i:j]).to(device))
            out.append(model(x0, x1).reshape(-1))
            i = j
    d = torch.cat(out)
    return {"lpips_mean": float(d.mean()), "lpips": d}


class EditMetrics:
    """`generate_imgs` + `cal_evaluation` (utils.py:434-551) over tensors.  `update(img_orig, img_gen, text_features)` takes the
    generator's fp32 images [B,3,H,W] in [-1, 1]; `compute()` returns (IS of the edited images, FID original vs edited, mean identity
    similarity, share of edits whose CLIP score against the text improved), as cal_evaluation does.
    jpeg=True: each image goes through to_bytes(grid=False) -> to_jpeg -> from_jpeg first -- the reference's metric reads the
    quality-75 JPEG files save_image wrote; this is that round trip without the disk.  jpeg=False feeds to_bytes' pixels directly.
    id_loss(img_gen, img_orig) -> (loss, ...) as criteria/id_loss.py: (1 - loss) * B is accumulated.  clip_loss: an object with
    `preprocess(images)` and `encode_image(images)` (CLIPLoss): an edit improves when cos(clip(gen), text) > cos(clip(orig), text).
    Either may be None; its entry of the result is then None.  isc_splits: the splits of the Inception Score (torch_fidelity's 10)."""

    def __init__(self, extractor, clip_loss=None, id_loss=None, jpeg=True, isc_splits=10):
        self.extractor, self.clip_loss, self.id_loss, self.jpeg, self.isc_splits = extractor, clip_loss, id_loss, bool(jpeg), int(isc_splits)
        self.reset()

    def reset(self):
        self._f_orig, self._f_gen, self._logits = [], [], []
        self._id, self._improved, self._count = None, None, 0

    def _pixels(self, img):
        from .image_io import from_jpeg, to_bytes, to_jpeg
        u8 = to_bytes(img.detach().float(), grid=False)
        if self.jpeg:
            u8 = from_jpeg(to_jpeg(u8), device=img.device, stack=True)
        return u8

    @torch.no_grad()
    def update(self, img_orig, img_gen, text_features=None):
        if img_orig.shape != img_gen.shape or img_orig.dim() != 4 or img_orig.shape[1] != 3:
            raise ValueError(f"EditMetrics.update: images are two [B,3,H,W] tensors of one shape (got {tuple(img_orig.shape)}, {tuple(img_gen.shape)})")
        b = img_orig.shape[0]
        with torch.cuda.device(img_orig.device):
            (f_orig,) = self.extractor(self._pixels(img_orig), features=("2048",))
            f_gen, logits = self.extractor(self._pixels(img_gen), features=("2048", "logits_unbiased"))
            self._f_orig.append(f_orig), self._f_gen.append(f_gen), self._logits.append(logits)
            if self.id_loss is not None:
                term = (1 - torch.as_tensor(self.id_loss(img_gen, img_orig)[0], device=img_orig.device).float()) * b
                self._id = term if self._id is None else self._id + term
            if self.clip_loss is not None:
                if text_features is None:
                    raise ValueError("EditMetrics.update: clip_loss needs the CLIP text features of the prompt")
                text = text_features.float()
                text = text / text.norm(dim=-1, keepdim=True)
                score = []
                for img in (img_gen, img_orig):
                    e = self.clip_loss.encode_image(self.clip_loss.preprocess(img)).float()
                    score.append(((e / e.norm(dim=-1, keepdim=True)) * text).sum(-1))
                better = (score[0] > score[1]).sum()
                self._improved = better if self._improved is None else self._improved + better
        self._count += b

    def compute(self):
        """(IS, FID, ID, improve).  The first host synchronisation of the evaluation."""
        if self._count < 2:
            raise RuntimeError("EditMetrics.compute: fewer than two images were added")
        inception = isc_from_logits(torch.cat(self._logits), splits=self.isc_splits)[0]
        fid = fid_from_features(torch.cat(self._f_orig), torch.cat(self._f_gen))
        ident = None if self._id is None else float(self._id) / self._count
        improve = None if self._improved is None else float(self._improved) / self._count
        return inception, fid, ident, improve
