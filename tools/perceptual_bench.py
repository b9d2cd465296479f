#!/usr/bin/env python3
"""PerceptualLoss forward + backward (to image1) at stylegan_size 1024, image batch B in {1, 2, 4, 8}, target batch 1, on the HIP
kernels, with the same computation on stock torch ops (MIOpen convolutions, aten max-pooling / MSE) as a comparison line.

    python tools/perceptual_bench.py [--batches 1,2,4,8] [--iters 20] [--out FILE]

Timing: device events around each call after a warm-up; the median of --iters calls.  Algorithmic GFLOP = 9.42 (2B + 1): the
forward to relu2_2 is 9.42 GFLOP per 224^2 image (conv1_1 0.17, conv1_2 3.70, conv2_1 1.85, conv2_2 3.70) over the B images and
the one target, and the input gradient costs the same again for the B images.  TFLOP/s against the fp32-MFMA peak (157.3 TF).
The two paths' outputs (loss, image gradient) are compared at every timed size.  One JSON line per batch."""
import argparse
import json
import os
import statistics
import sys
import types

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3
GFLOP_PER_IMAGE = 9.42


def stock_loss(vgg, img1, img2, size):
    """The reference's composition on stock ops: the literal Upsample(7) -> AvgPool(size/32) chain, slices 1-2 as modules
    (MIOpen convolutions), MSELoss against the target run without autograd and broadcast over the batch."""
    def pre(x):
        return F.avg_pool2d(F.interpolate(x, scale_factor=7, mode="nearest"), size // 32)

    def feats(x):
        for seq in (vgg.slice1, vgg.slice2):
            x = seq(x)
        return x
    with torch.no_grad():
        f2 = feats(pre(img2))
    f1 = feats(pre(img1))
    return ((f1 - f2) ** 2).mean()


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from where2edit_amd.perceptual_loss import PerceptualLoss
    size = args.size
    torch.manual_seed(0)
    loss_mod = PerceptualLoss(types.SimpleNamespace(stylegan_size=size)).cuda()
    vgg = loss_mod.model
    lines = []
    for b in [int(v) for v in args.batches.split(",")]:
        img1 = torch.tanh(0.8 * torch.randn(b, 3, size, size, device="cuda"))
        img2 = torch.tanh(0.8 * torch.randn(1, 3, size, size, device="cuda"))
        x1 = img1.clone().requires_grad_(True)

        def hip():
            (g,) = torch.autograd.grad(loss_mod(x1, img2), x1)
            return g

        def stock():
            (g,) = torch.autograd.grad(stock_loss(vgg, x1, img2, size), x1)
            return g
        ms_hip = timed(hip, args.iters)
        ms_stock = timed(stock, args.iters)
        l_h, l_s = loss_mod(x1, img2).item(), stock_loss(vgg, x1, img2, size).item()
        g_h, g_s = hip(), stock()
        gerr = ((g_h - g_s).abs().max() / g_s.abs().max()).item()
        cos = F.cosine_similarity(g_h.flatten().double(), g_s.flatten().double(), dim=0).item()
        gflop = GFLOP_PER_IMAGE * (2 * b + 1)
        line = {"tool": "perceptual_bench", "size": size, "batch": b, "target_batch": 1, "gflop": round(gflop, 2),
                "hip_ms": round(ms_hip, 3), "hip_tflops": round(gflop / ms_hip, 2), "hip_pct_fp32_peak": round(100 * gflop / ms_hip / PEAK_TF, 1),
                "stock_ms": round(ms_stock, 3), "stock_tflops": round(gflop / ms_stock, 2), "speedup_vs_stock": round(ms_stock / ms_hip, 3),
                "loss_rel_diff": abs(l_h - l_s) / abs(l_s), "grad_rel_err": gerr, "grad_cosine": cos, "iters": args.iters}
        print(json.dumps(line), flush=True)
        lines.append(line)
        assert abs(l_h - l_s) <= 1e-4 * abs(l_s) and cos >= 0.9999, line
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(v) + "\n" for v in lines))


if __name__ == "__main__":
    main()
