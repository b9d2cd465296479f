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
`calculate_iou(label_resize=...)`, uint8 labels of any size are resized on the device with Pillow's own arithmetic (image_io.py)."""
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
