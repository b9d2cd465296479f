#!/usr/bin/env python3
"""LPIPS (VGG16, v0.1) on the HIP kernels against the same network composed from stock torch ops (F.conv2d = MIOpen, F.max_pool2d,
the literal head) in the same process: forward, and forward + backward to in0, at 256^2 and 1024^2, batch 1 and 8.

    python tools/lpips_bench.py [--sizes 256,1024] [--batches 1,8] [--runs 5] [--out profiles/lpips_bench.jsonl] [--no-heads]

Timing: device events around one call; HIP and stock alternate, one run each, `--runs` times after a warm-up of both; the medians are
reported, whichever way they fall.  The two paths' distance and gradient are compared at every timed shape.
A second set of lines times the head alone (w2e_lpips_head_fwd / _bwd against the literal torch head) at the five tap shapes of a
256^2 input, batch 8, with the bytes a single pass over the tensors moves (forward: f0 + f1 read; backward: f0 + f1 read, g0 written)
and the rate that corresponds to.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stock_head(f0, f1, w):
    def unit(f):
        return f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return (w.reshape(1, -1, 1, 1) * (unit(f0) - unit(f1)) ** 2).sum(1, keepdim=True).mean((2, 3), keepdim=True)


def stock_lpips(model, in0, in1):
    """The published composition on stock ops: both inputs through the scaling layer and the five slices, the literal head per tap."""
    from where2edit_amd import vgg16 as V

    def taps(x):
        h, outs = (x - model.scaling_layer.shift) / model.scaling_layer.scale, []
        for k, r in enumerate(V.SLICES):
            for i in r:
                if i in V.POOLS:
                    h = F.max_pool2d(h, 2, 2)
                elif i in V.CONVS:
                    conv = getattr(getattr(model.net, f"slice{k + 1}"), str(i))
                    h = F.relu(F.conv2d(h, conv.weight, conv.bias, padding=1))
            outs.append(h)
        return outs
    with torch.no_grad():
        t1 = taps(in1)
    t0 = taps(in0)
    return sum(stock_head(a, b, getattr(model, f"lin{k}").model._modules["1"].weight) for k, (a, b) in enumerate(zip(t0, t1)))


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(hip, stock, runs, warmup=2):
    for _ in range(warmup):
        hip(), stock()
    torch.cuda.synchronize()
    th, ts = [], []
    for _ in range(runs):
        th.append(once(hip))
        ts.append(once(stock))
    return statistics.median(th), statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-heads", action="store_true")
    args = ap.parse_args()
    from where2edit_amd.lpips import LPIPS, head_bwd, head_fwd
    model = LPIPS().cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for size in [int(v) for v in args.sizes.split(",")]:
        for b in [int(v) for v in args.batches.split(",")]:
            in0 = torch.tanh(0.8 * torch.randn(b, 3, size, size, device="cuda", generator=g))
            in1 = (in0 + 0.1 * torch.randn(b, 3, size, size, device="cuda", generator=g)).clamp(-1, 1)
            x = in0.clone().requires_grad_(True)

            def hip_fwd():
                with torch.no_grad():
                    return model(in0, in1)

            def stock_fwd():
                with torch.no_grad():
                    return stock_lpips(model, in0, in1)

            def hip_fb():
                return torch.autograd.grad(model(x, in1).sum(), x)[0]

            def stock_fb():
                return torch.autograd.grad(stock_lpips(model, x, in1).sum(), x)[0]

            d_h, d_s = hip_fwd().reshape(-1), stock_fwd().reshape(-1)
            g_h, g_s = hip_fb(), stock_fb()
            cmp = {"distance_rel_diff": ((d_h - d_s).abs().max() / d_s.abs().max()).item(),
                   "grad_rel_err": ((g_h - g_s).abs().max() / g_s.abs().max()).item(),
                   "grad_cosine": F.cosine_similarity(g_h.flatten().double(), g_s.flatten().double(), dim=0).item()}
            del g_h, g_s
            for what, hip, stock in (("forward", hip_fwd, stock_fwd), ("forward+backward", hip_fb, stock_fb)):
                ms_h, ms_s = alternate(hip, stock, args.runs)
                emit({"tool": "lpips_bench", "what": what, "size": size, "batch": b, "hip_ms": round(ms_h, 3), "stock_ms": round(ms_s, 3),
                      "speedup_vs_stock": round(ms_s / ms_h, 3), "runs": args.runs, **cmp})
            del x, in0, in1
            torch.cuda.empty_cache()

    if not args.no_heads:
        b = 8
        for c, s in ((64, 256), (128, 128), (256, 64), (512, 32), (512, 16)):
            f0 = torch.relu(torch.randn(b, c, s, s, device="cuda", generator=g))
            f1 = torch.relu(f0 + 0.1 * torch.randn(b, c, s, s, device="cuda", generator=g))
            w = torch.rand(c, device="cuda", generator=g) / c
            gout = torch.ones(b, device="cuda")
            g0 = torch.empty_like(f0)
            fr = f0.clone().requires_grad_(True)

            def stock_b():
                return torch.autograd.grad(stock_head(fr, f1, w).sum(), fr)[0]
            ms_h, ms_s = alternate(lambda: head_fwd(f0, f1, w), lambda: stock_head(f0, f1, w), args.runs)
            mb = 2 * f0.numel() * 4 / 1e6
            emit({"tool": "lpips_bench", "what": "head forward", "channels": c, "hw": s, "batch": b, "hip_ms": round(ms_h, 4),
                  "stock_ms": round(ms_s, 4), "one_pass_mb": round(mb, 1), "hip_gb_s": round(mb / ms_h, 1), "runs": args.runs})
            ms_h, ms_s = alternate(lambda: head_bwd(f0, f1, w, gout, g0=g0, relu=True), stock_b, args.runs)
            mb = 3 * f0.numel() * 4 / 1e6
            emit({"tool": "lpips_bench", "what": "head backward (stock: forward + backward)", "channels": c, "hw": s, "batch": b,
                  "hip_ms": round(ms_h, 4), "stock_ms": round(ms_s, 4), "one_pass_mb": round(mb, 1), "hip_gb_s": round(mb / ms_h, 1),
                  "runs": args.runs})
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(v) + "\n" for v in lines))


if __name__ == "__main__":
    main()
