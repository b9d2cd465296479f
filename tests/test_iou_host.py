"""The mask IoU evaluation, host side (no GPU): the numpy yardstick (tests/iou_ref.py) against scikit-learn, the CelebAMask-HQ
region table and its lut, the float -> id conversion, the C ABI of the counting kernel, and MaskIoU's argument errors."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import iou_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "w2e_mask_iou_counts"


def test_iou_ref_equals_sklearn_jaccard_score():
    """Random multilabel data at T = 8 with region 5 (the ears) empty on both sides: jaccard_score gives 0 there (and warns), and the
    macro mean counts it.  The yardstick's exact rationals, rounded to double, are scikit-learn's numbers."""
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.RandomState(11)
    b, t, s = 3, 8, 12
    masks = rng.uniform(0.5, 1.0, size=(b, t, s, s)).astype(np.float32)
    masks[:, 4] = 0.1                                                    # never predicted
    ids = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 17, 18], size=(b, s, s))  # no 8 / 9: no ear pixel
    pred, real = R.one_hot(masks, ids, t)
    assert pred[:, 4].sum() == 0 and real[:, 4].sum() == 0 and real.sum() > 0 and pred.sum() > 0
    per, mean = R.jaccard(R.confusion_counts(masks, ids, t))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        each = metrics.jaccard_score(real, pred, average=None)
        macro = metrics.jaccard_score(real, pred, average="macro")
    assert [float(p) for p in per] == each.tolist()
    assert per[4] == 0 and abs(float(mean) - macro) <= 1e-15


def test_celebamask_table_and_lut_match_the_reference_remap():
    from where2edit_amd import CELEBAMASK_REGIONS, region_lut
    from where2edit_amd import evaluation as E
    assert len(CELEBAMASK_REGIONS) == 8 and all(len(r) == 3 for r in CELEBAMASK_REGIONS)
    assert [r[0] for r in CELEBAMASK_REGIONS] == ["skin", "nose", "eyes", "eyebrows", "ears", "mouth", "lips", "hair"]
    assert E.celebamask_mapping() == R.CELEBAMASK_MAP
    lut = region_lut(E.celebamask_mapping(), 8)
    assert lut.dtype == torch.uint8 and lut.shape == (256,)
    assert lut.tolist() == R.remap(np.arange(256)).tolist()
    for raw in (0, 3, 14, 15, 16, 17, 18, 255):
        assert lut[raw] == 0, raw
    assert [int(lut[i]) for i in (1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)] == [1, 2, 3, 3, 4, 4, 5, 5, 6, 7, 7, 8]


def test_lut_entry_above_the_region_count_is_refused():
    from where2edit_amd import MaskIoU, region_lut
    with pytest.raises(ValueError, match=r"maps to region 9.*8 regions"):
        region_lut({1: 9}, 8)
    with pytest.raises(ValueError, match="0..255"):
        region_lut({256: 1}, 8)
    with pytest.raises(ValueError, match="classes"):
        region_lut({}, 17)
    with pytest.raises(ValueError, match="maps to region 4"):  # the default table needs its 8 regions
        MaskIoU(classes=3)
    assert region_lut({7: 16}, 16)[7] == 16


def test_float_labels_convert_to_the_exact_ids():
    """ToTensor divides the uint8 label by 255 in fp32; (label * 255).type(torch.int) truncates: exact for every id."""
    from where2edit_amd.evaluation import labels_to_ids
    ids = torch.arange(256, dtype=torch.uint8)
    as_float = ids.to(torch.float32).div(255)
    assert torch.equal(labels_to_ids(as_float), ids)
    assert R.float_labels_to_ids(as_float.numpy()).tolist() == list(range(256))
    assert torch.equal(labels_to_ids(ids.long()), ids)


def test_binarise_is_the_two_reference_writes():
    from where2edit_amd import binarise
    lo, hi = np.nextafter(np.float32(0.8), np.float32(0)), np.nextafter(np.float32(0.8), np.float32(1))
    m = torch.tensor([0.0, 0.7, 0.75, float(lo), float(np.float32(0.8)), float(hi), 1.0, float("inf"), -float("inf")], dtype=torch.float32)
    ref = m.clone()
    ref[ref < 0.8] = 0   # utils.py:649-650
    ref[ref > 0.7] = 1
    assert torch.equal(binarise(m), ref) and binarise(m).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0]
    assert binarise(torch.tensor([float("nan")])).item() == 0


def test_counting_entry_point_is_declared_prototyped_and_exported():
    from where2edit_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "w2e_attention.h")).read()
    m = re.search(r"^int\s+" + SYMBOL + r"\s*\(([^;]*)\)\s*;", header, flags=re.M)
    assert m, "not declared in include/w2e_attention.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib._PROTOS[SYMBOL]
    want = {"*": ctypes.c_void_p, "float": ctypes.c_float, "int": ctypes.c_int}
    assert res is ctypes.c_int and len(args) == len(params) == 9
    for p, a in zip(params, args):
        kind = "*" if "*" in p else p.split()[0]
        assert a is want[kind], (p, a)
    lib = ctypes.CDLL(build.build(verbose=False))
    fn = getattr(lib, SYMBOL)
    fn.restype, fn.argtypes = res, args
    lib.w2e_last_error.restype = ctypes.c_char_p
    # argument validation happens before any HIP call
    p = ctypes.c_void_p(64)
    assert fn(None, p, p, 0.8, 1, 8, 4, p, None) != 0 and b"null" in lib.w2e_last_error()
    assert fn(p, p, p, 0.8, 1, 17, 4, p, None) != 0 and b"classes" in lib.w2e_last_error()
    assert fn(p, p, p, 0.8, 1, 0, 4, p, None) != 0
    assert fn(p, p, p, float("nan"), 1, 8, 4, p, None) != 0 and b"NaN" in lib.w2e_last_error()
    assert fn(p, p, p, 0.8, 1, 8, 0, p, None) != 0
    assert fn(p, p, p, 0.8, 0, 8, 4, p, None) == 0  # an empty batch: nothing to launch


def test_mask_iou_refuses_cpu_tensors_and_a_size_mismatch():
    from where2edit_amd import MaskIoU
    m = MaskIoU()
    with pytest.raises(RuntimeError, match=r"must be on the GPU.*\.to\('cuda'\)"):
        m.update(torch.zeros(2, 8, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"resize the labels to 4 x 4 \(nearest\)"):
        m.update(torch.zeros(2, 8, 4, 4), torch.zeros(2, 1, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"\[B, 8, S, S\]"):
        m.update(torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU only"):
        MaskIoU(device="cpu")
