"""Numpy restatement of the mask IoU of utils.py:639-726 in integer arithmetic, for the tests of where2edit_amd.evaluation: the
label remap, the one-hot matrices, the three confusion counts per region and the Jaccard scores scikit-learn's `jaccard_score`
returns on them.  CPU only, no GPU library; the mapping below is written out here, not read from the package."""
from fractions import Fraction

import numpy as np

# raw CelebAMask-HQ parsing id -> region 1..8 (utils.py:702-715); every other id -> 0
CELEBAMASK_MAP = {1: 1, 2: 2, 4: 3, 5: 3, 6: 4, 7: 4, 8: 5, 9: 5, 10: 6, 11: 7, 12: 7, 13: 8}


def float_labels_to_ids(labels):
    """utils.py:702: (label * 255).type(torch.int) on float32 labels."""
    return (np.asarray(labels, dtype=np.float32) * np.float32(255)).astype(np.int32)


def remap(ids, mapping=None):
    """Region id (0 = none) of every raw parsing id."""
    mapping = CELEBAMASK_MAP if mapping is None else mapping
    ids = np.asarray(ids).astype(np.int64)
    out = np.zeros_like(ids)
    for raw, region in mapping.items():
        out[ids == raw] = region
    return out


def one_hot(masks, ids, classes, threshold=0.8, mapping=None):
    """(pred, real): two [B*S*S, T] 0/1 matrices, the arguments of the reference's jaccard_score call (:721-724).  masks [B,T,S,S]
    float32, predicted where mask >= float32(threshold); ids [B,S,S] raw parsing ids."""
    masks = np.asarray(masks, dtype=np.float32)
    b, t, s, _ = masks.shape
    assert t == classes and np.asarray(ids).shape == (b, s, s)
    with np.errstate(invalid="ignore"):
        pred = (masks >= np.float32(threshold)).transpose(0, 2, 3, 1).reshape(-1, t).astype(np.int64)
    region = remap(ids, mapping).reshape(-1)
    real = (region[:, None] == np.arange(1, t + 1)[None, :]).astype(np.int64)
    return pred, real


def confusion_counts(masks, ids, classes, threshold=0.8, mapping=None):
    """int64 [T,3]: per region #(pred and real), #pred, #real."""
    pred, real = one_hot(masks, ids, classes, threshold, mapping)
    return np.stack([(pred & real).sum(0), pred.sum(0), real.sum(0)], 1).astype(np.int64)


def jaccard(counts):
    """(per-region IoU as exact Fractions, their mean): inter / (pred + real - inter), 0 where the union is empty."""
    per = []
    for inter, pred, real in np.asarray(counts).tolist():
        union = pred + real - inter
        per.append(Fraction(inter, union) if union else Fraction(0))
    return per, sum(per) / len(per)
