"""Times `MaskIoU.update` (csrc/evaluate.hip: binarisation, label remap and the 3*T confusion counts in one pass) against the same
counts composed from stock ops (lut gather, one-hot compare, logical and, three sums) at the evaluation's own shape, 90 x 8 x 64^2,
and at a streaming one, 4 x 8 x 1024^2, and against a `copy_` of the same mask bytes (the bandwidth yardstick DESIGN.md uses).

HIP events around device-synchronised repeats; the variants are run alternately, `--repeats` times each (>= 5): `ms_min .. ms_max` is
the run-to-run spread a difference has to exceed.  An interval is a whole call of the Python entry point (checks, ctypes call), which
at 90 x 8 x 64^2 (11.8 MB, microseconds of HBM time) is most of it.  The counts of the two forms are compared before anything is timed.
GB/s = (mask bytes + label bytes) / median.  One JSON line per (shape, variant), appended to --out.

    python tools/iou_bench.py [--repeats 20] [--out profiles/mask_iou_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stock_counts(masks, labels, lut, threshold, counts):
    t = masks.shape[1]
    region = lut[labels.long()]
    real = region[:, None] == torch.arange(1, t + 1, device=masks.device, dtype=torch.uint8)[None, :, None, None]
    pred = masks >= threshold
    counts += torch.stack([(pred & real).sum((0, 2, 3)), pred.sum((0, 2, 3)), real.sum((0, 2, 3))], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mask_iou_bench.jsonl"))
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("--repeats must be >= 5: the spread is part of the result")
    if not torch.cuda.is_available():
        raise SystemExit("iou_bench needs the GPU: a host timing says nothing about this kernel")
    from where2edit_amd import MaskIoU
    from where2edit_amd.evaluation import _f32
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for b, t, s in ((90, 8, 64), (4, 8, 1024)):
        masks = torch.rand((b, t, s, s), device=dev, generator=g)
        labels = torch.randint(0, 19, (b, s, s), device=dev, generator=g).to(torch.uint8)
        sink = torch.empty_like(masks)
        metric = MaskIoU(classes=t, device=dev)
        metric.update(masks, labels)
        ref = torch.zeros((t, 3), dtype=torch.int64, device=dev)
        stock_counts(masks, labels, metric._lut, _f32(0.8), ref)
        if not torch.equal(metric.counts(), ref.cpu()):
            raise SystemExit(f"iou_bench: the kernel's counts differ from the stock-op composition at {b} x {t} x {s}^2")
        variants = {"mask_iou_update": lambda: metric.update(masks, labels),
                    "stock_ops": lambda: stock_counts(masks, labels, metric._lut, _f32(0.8), ref),
                    "copy_": lambda: sink.copy_(masks)}
        times = {n: [] for n in variants}
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        read = masks.numel() * 4 + labels.numel()
        for name, ms in times.items():
            med = statistics.median(ms)
            nbytes = 2 * masks.numel() * 4 if name == "copy_" else read  # a copy reads and writes
            lines.append({"tool": "iou_bench", "variant": name, "batch": b, "classes": t, "size": s, "bytes": nbytes, "ms_median": med,
                          "ms_min": min(ms), "ms_max": max(ms), "repeats": len(ms), "gb_per_s": nbytes / med / 1e6})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
