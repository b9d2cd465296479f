#!/usr/bin/env python3
"""FeatureExtractorInceptionV3 forward ('2048' + 'logits_unbiased') at batch 1, 8 and 32 on the HIP kernels, against the same network
composed from stock torch ops (MIOpen convolutions, aten pools and cat; the resize is the HIP kernel on both sides) in fp32 with TF32
off, in the same process.

    python tools/inception_bench.py [--batches 1,8,32] [--rounds 5] [--size 256] [--out profiles/inception_bench.jsonl] [--layers B]

Timing: device events around one forward; the two sides alternate (HIP, stock, HIP, ...) after a warm-up of each, and the median of
--rounds runs is reported.  Work: 5.71 GMAC = 11.42 GFLOP per image (the 94 convolutions and the head at 299^2); TFLOP/s against the
157.3 TF the project uses as the fp32-MFMA peak.  The two sides' features are compared at every batch.  One JSON line per batch.
--layers B: instead, time every distinct convolution shape of the network alone at batch B on both sides (for tuning)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3
GFLOP_PER_IMAGE = 2 * 5.71


def stock_forward(net, P, x299):
    """The network on stock ops from the resized fp32 input, reading the same folded parameters."""
    from where2edit_amd import inception as I

    def cv(name, t):
        _, _, _, _, _, stride, ph, pw = I.SPEC[name]
        y = F.conv2d(t, P.w[name], stride=stride, padding=(ph, pw))
        return F.relu(y * P.scale[name][None, :, None, None] + P.shift[name][None, :, None, None])

    def chain(name, t, *leaves):
        for leaf in leaves:
            t = cv(f"{name}.{leaf}", t)
        return t
    avg = lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)
    x = x299
    for name in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        x = cv(name, x)
    x = F.max_pool2d(x, 3, 2)
    x = cv("Conv2d_4a_3x3", cv("Conv2d_3b_1x1", x))
    x = F.max_pool2d(x, 3, 2)
    for name, kind in I.BLOCKS:
        if kind == "A":
            x = torch.cat([chain(name, x, "branch1x1"), chain(name, x, "branch5x5_1", "branch5x5_2"),
                           chain(name, x, "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), chain(name, avg(x), "branch_pool")], 1)
        elif kind == "B":
            x = torch.cat([chain(name, x, "branch3x3"), chain(name, x, "branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"), F.max_pool2d(x, 3, 2)], 1)
        elif kind == "C":
            x = torch.cat([chain(name, x, "branch1x1"), chain(name, x, "branch7x7_1", "branch7x7_2", "branch7x7_3"),
                           chain(name, x, "branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"),
                           chain(name, avg(x), "branch_pool")], 1)
        elif kind == "D":
            x = torch.cat([chain(name, x, "branch3x3_1", "branch3x3_2"),
                           chain(name, x, "branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"), F.max_pool2d(x, 3, 2)], 1)
        else:
            a, d = chain(name, x, "branch3x3_1"), chain(name, x, "branch3x3dbl_1", "branch3x3dbl_2")
            pooled = avg(x) if I.E_POOL[name] == I.POOL_AVG else F.max_pool2d(x, 3, 1, 1)
            x = torch.cat([chain(name, x, "branch1x1"), chain(name, a, "branch3x3_2a"), chain(name, a, "branch3x3_2b"),
                           chain(name, d, "branch3x3dbl_3a"), chain(name, d, "branch3x3dbl_3b"), chain(name, pooled, "branch_pool")], 1)
    f = x.mean((2, 3))
    return f, f @ net.fc.weight.T


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def alternate(hip, stock, rounds, warmup=2):
    for _ in range(warmup):
        hip(), stock()
    torch.cuda.synchronize()
    th, ts = [], []
    for _ in range(rounds):
        th.append(one(hip)[0])
        ts.append(one(stock)[0])
    return statistics.median(th), statistics.median(ts)


def layer_table(net, P, batch, rounds):
    """Every distinct (cin, cout, kernel, stride, padding, input size) of the network, alone."""
    from where2edit_amd import inception as I
    sizes = {}
    x = torch.zeros(1, 3, I.SIZE, I.SIZE, device="meta")

    def note(name, t):
        sizes[name] = tuple(t.shape[2:])
    stem = ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3", "pool", "Conv2d_3b_1x1", "Conv2d_4a_3x3", "pool")
    for name in stem:
        if name == "pool":
            x = F.max_pool2d(x, 3, 2)
            continue
        note(name, x)
        _, cin, cout, kh, kw, stride, ph, pw = I.SPEC[name]
        x = F.conv2d(x, torch.zeros(cout, cin, kh, kw, device="meta"), stride=stride, padding=(ph, pw))
    side = {"A": 35, "B": 35, "C": 17, "D": 17, "E": 8}
    seen, total_h, total_s = {}, 0.0, 0.0
    for name, cin, cout, kh, kw, stride, ph, pw in I.LAYERS:
        h = sizes[name][0] if name in sizes else side[dict(I.BLOCKS)[name.split(".")[0]]]  # every layer of a block runs at the block's input size
        key = (cin, cout, kh, kw, stride, ph, pw, h)
        if key in seen:
            seen[key][0] += 1
            continue
        t = torch.randn(batch, cin, h, h, device="cuda")
        hip = lambda: I.conv2d_bn_relu(t, P.w[name], P.scale[name], P.shift[name], stride, (ph, pw))
        stock = lambda: F.relu(F.conv2d(t, P.w[name], stride=stride, padding=(ph, pw)) * P.scale[name][None, :, None, None] + P.shift[name][None, :, None, None])
        mh, ms = alternate(hip, stock, rounds)
        oh = (h + 2 * ph - kh) // stride + 1
        gflop = 2e-9 * batch * oh * oh * cout * cin * kh * kw
        seen[key] = [1, name, mh, ms, gflop]
    for key, (count, name, mh, ms, gflop) in seen.items():
        total_h += count * mh
        total_s += count * ms
        print(f"{name:28s} x{count} cin {key[0]:4d} n {key[1]:4d} {key[2]}x{key[3]} s{key[4]} @{key[7]:3d}: hip {mh:7.3f} ms {gflop / mh:6.1f} TF | stock {ms:7.3f} ms "
              f"{gflop / ms:6.1f} TF | ratio {ms / mh:5.2f}", flush=True)
    print(f"sum over the 94 convolutions at batch {batch}: hip {total_h:.2f} ms, stock {total_s:.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=256, help="side of the uint8 input images")
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=0)
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    from where2edit_amd import inception as I
    net = I.FeatureExtractorInceptionV3().cuda()
    P = net.plan()
    if args.layers:
        with torch.no_grad():
            layer_table(net, P, args.layers, args.rounds)
        return
    lines = []
    for b in [int(v) for v in args.batches.split(",")]:
        x = torch.randint(0, 256, (b, args.size, args.size, 3), device="cuda", dtype=torch.uint8)
        hip = lambda: net(x)
        with torch.no_grad():
            stock = lambda: stock_forward(net, P, I.resize_input(x))
            ms_hip, ms_stock = alternate(hip, stock, args.rounds)
            (fh, lh), (fs, ls) = hip(), stock()
        ferr = ((fh - fs).abs().max() / fs.abs().max()).item()
        lerr = ((lh - ls).abs().max() / ls.abs().max()).item()
        gflop = GFLOP_PER_IMAGE * b
        line = {"tool": "inception_bench", "batch": b, "input": args.size, "gflop": round(gflop, 2), "hip_ms": round(ms_hip, 3),
                "hip_tflops": round(gflop / ms_hip, 2), "hip_pct_fp32_peak": round(100 * gflop / ms_hip / PEAK_TF, 1), "fp32_peak_tflops": PEAK_TF,
                "stock_ms": round(ms_stock, 3), "stock_tflops": round(gflop / ms_stock, 2), "stock_over_hip": round(ms_stock / ms_hip, 3),
                "features_rel_diff": ferr, "logits_rel_diff": lerr, "rounds": args.rounds}
        print(json.dumps(line), flush=True)
        lines.append(line)
        assert ferr <= 1e-4 and lerr <= 1e-4, line
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(v) + "\n" for v in lines))


if __name__ == "__main__":
    main()
