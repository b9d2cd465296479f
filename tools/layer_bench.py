#!/usr/bin/env python3
"""Per-layer microbenchmark of the modulated-conv kernels at the FFHQ-1024 generator's layer shapes
(HIP events on the launch stream, random data).  python tools/layer_bench.py [--batch 4]
python tools/layer_bench.py --upblur [--batch 8] [--repeats 5]: per up-sampling layer, the two-launch forward (all-phase UP conv +
blur launch with the fused activation) against the one-launch form (w2e_modconv_upblur), alternating, `repeats` runs each.
python tools/layer_bench.py --rgbfold [--batch 8] [--repeats 5]: per level 4^2 .. 512^2 of the backward, the pair (stride-2
input-gradient conv with the dot epilogue, w2e_torgb_bwd_actbwd) against the folded launch (w2e_modconv_down_rgbfold), likewise."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from where2edit_amd import functional as K  # noqa: E402

LAYERS = [  # cin, cout, input res, upsample
    (512, 512, 4, False), (512, 512, 4, True), (512, 512, 8, False), (512, 512, 8, True), (512, 512, 16, False),
    (512, 512, 16, True), (512, 512, 32, False), (512, 512, 32, True), (512, 512, 64, False), (512, 256, 64, True),
    (256, 256, 128, False), (256, 128, 128, True), (128, 128, 256, False), (128, 64, 256, True), (64, 64, 512, False),
    (64, 32, 512, True), (32, 32, 1024, False)]


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def upblur_table(batch, iters, repeats, sel):
    """The pair (conv + blur launch) against the fused form, per up layer from 32^2 inputs up: min / median / max over `repeats`
    alternating runs of `iters` calls each.  A layer counts as a gain only if the fused form's slowest run beats the pair's fastest."""
    from where2edit_amd import _lib
    dev = "cuda"
    kernel = (torch.outer(torch.tensor([1., 3., 3., 1.]), torch.tensor([1., 3., 3., 1.])) / 64 * 4).to(dev)
    print(f"batch {batch}: {iters} calls per run, {repeats} alternating runs of each form; ms per call as min / median / max")
    print(f"{'layer':22s} | {'conv + blur launch':>26s} | {'fused':>26s} | {'median gain':>11s} | fused max < pair min")
    for i, (cin, cout, h, up) in enumerate(LAYERS):
        if not up or h < 32 or (sel and i not in sel):
            continue
        w = torch.randn(cout, cin, 3, 3, device=dev)
        fwd = K.conv_pack(w, (cin * 9) ** -0.5, False, False)
        x = torch.randn(batch, cin, h, h, device=dev)
        s = torch.randn(batch, cin, device=dev)
        d = torch.rand(batch, cout, device=dev) + 0.5
        act = (torch.randn(1, 1, 2 * h, 2 * h, device=dev), torch.randn(1, device=dev), torch.randn(cout, device=dev))

        def pair():
            t, _ = K._modconv_raw(K.MODE_UP, x, fwd, s, d, h, h)
            return K._upfirdn2d_raw(t, kernel, 2 * h, 2 * h, 1, 1, 1, 1, True, act=(None,) + act, planar_hw=(2 * h + 1, 2 * h + 1))

        def fused():
            return K._modconv_upblur_raw(x, fwd, s, d, kernel, h, h, act)

        _lib.set_option("tune_upblur", 1)
        if not K._upblur_planned(batch, cin, cout, h, h):
            print(f"{cin:3d}->{cout:3d} @{h:4d} up: the fused form does not take this shape")
            continue
        tp, tf = [], []
        for _ in range(repeats):
            tp.append(timeit(pair, iters))
            tf.append(timeit(fused, iters))
        _lib.set_option("tune_upblur", "")
        tp.sort(), tf.sort()
        fmt = lambda t: f"{t[0]:8.3f} {t[len(t) // 2]:8.3f} {t[-1]:8.3f}"  # noqa: E731
        gain = tp[len(tp) // 2] - tf[len(tf) // 2]
        print(f"{cin:3d}->{cout:3d} @{h:4d} up      | {fmt(tp)} | {fmt(tf)} | {gain:8.3f} ms | {'yes' if tf[-1] < tp[0] else 'no'}")


def rgbfold_table(batch, iters, repeats, sel):
    """The pair (DOWN dot conv, ToRGB backward with the activation backward) against the folded launch, per up-sampling layer: the
    backward of the layer h -> 2h writes level h.  min / median / max over `repeats` alternating runs of `iters` calls each.  A level
    counts as a gain only if the folded form's slowest run beats the pair's fastest."""
    from where2edit_amd import _lib
    from where2edit_amd._lib import call, ptr, stream_ptr
    dev = "cuda"
    print(f"batch {batch}: {iters} calls per run, {repeats} alternating runs of each form; ms per call as min / median / max")
    print(f"{'level (DOWN conv K->N)':26s} | {'dot conv + torgb_bwd_actbwd':>26s} | {'folded':>26s} | {'median gain':>11s} | folded max < pair min")
    for i, (cin, cout, h, up) in enumerate(LAYERS):
        if not up or (sel and i not in sel):
            continue
        name = f"{cout:3d}->{cin:3d} @{h:4d}"
        _lib.set_option("tune_rgbfold", 1)
        planned = K._rgbfold_planned(batch, cout, cin, h, h)
        _lib.set_option("tune_rgbfold", "")
        if not planned:
            print(f"{name:26s} | the folded form does not take this launch (split over K)")
            continue
        wt = torch.randn(cout, cin, 3, 3, device=dev)
        bwd = K.conv_pack(wt, (cin * 9) ** -0.5, True, False)
        g = torch.randn(batch, cout, 2 * h + 1, 2 * h + 1, device=dev)
        x = torch.randn(batch, cin, h, h, device=dev)
        s = torch.randn(batch, cin, device=dev)
        d = torch.rand(batch, cout, device=dev) + 0.5
        gy = torch.randn(batch, 3, h, h, device=dev)
        wsc, style = torch.randn(3, cin, device=dev), torch.randn(batch, cin, device=dev)
        noise = torch.randn(1, 1, h, h, device=dev)
        gx, gpre = torch.empty_like(x), torch.empty_like(x)
        dot, gw, sums3 = torch.zeros(batch, cin, device=dev), torch.zeros(batch, cin, device=dev), torch.zeros(batch, cin, 3, device=dev)

        def pair():
            K._modconv_raw(K.MODE_DOWN, g, bwd, d, s, h, h, dot_with=x, out=gx, dot_out=dot)
            call("w2e_torgb_bwd_actbwd", ptr(x), ptr(wsc), ptr(style), ptr(gy), ptr(gx), ptr(noise), ptr(gpre), ptr(gw), ptr(sums3),
                 batch, cin, h, h, 0.2, K.SQRT2, stream_ptr())

        def folded():
            K._modconv_down_rgbfold_raw(g, bwd, d, s, h, h, x, gy, wsc, style, noise, out=gpre, dot_out=dot, sums3=sums3, gw=gw)

        tp, tf = [], []
        for _ in range(repeats):
            tp.append(timeit(pair, iters))
            tf.append(timeit(folded, iters))
        tp.sort(), tf.sort()
        fmt = lambda t: f"{t[0]:8.3f} {t[len(t) // 2]:8.3f} {t[-1]:8.3f}"  # noqa: E731
        gain = tp[len(tp) // 2] - tf[len(tf) // 2]
        print(f"{name:26s} | {fmt(tp)} | {fmt(tf)} | {gain:8.3f} ms | {'yes' if tf[-1] < tp[0] else 'no'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--upblur", action="store_true", help="compare conv + blur launch with the one-launch form on the up layers")
    ap.add_argument("--rgbfold", action="store_true", help="compare (DOWN dot conv, torgb_bwd_actbwd) with the folded launch per level")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", type=str, default="", help="comma list of layer indices")
    ap.add_argument("--warm", type=float, default=0.0, help="seconds of GPU load before the first measurement (a fresh box "
                    "starts at idle clocks: short runs of the first layers read low without it)")
    args = ap.parse_args()
    if args.warm > 0:
        import time
        a = torch.randn(4096, 4096, device="cuda")
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < args.warm:
            (a @ a).sum().item()
    if args.upblur:
        upblur_table(args.batch, args.iters, args.repeats, [int(i) for i in args.only.split(',')] if args.only else None)
        return
    if args.rgbfold:
        rgbfold_table(args.batch, args.iters, args.repeats, [int(i) for i in args.only.split(',')] if args.only else None)
        return
    B = args.batch
    dev = "cuda"
    tot = {"fwd": [0.0, 0.0], "bwd": [0.0, 0.0]}
    print(f"{'layer':28s} {'GFLOP':>8s} | {'fwd ms':>8s} {'TF/s':>7s} | {'dgrad ms':>8s} {'TF/s':>7s}")
    sel = [int(i) for i in args.only.split(',')] if args.only else range(len(LAYERS))
    for cin, cout, h, up in [LAYERS[i] for i in sel]:
        w = torch.randn(cout, cin, 3, 3, device=dev)
        scale = (cin * 9) ** -0.5
        fwd = K.conv_pack(w, scale, False, False)
        bwd = K.conv_pack(w, scale, True, not up)
        x = torch.randn(B, cin, h, h, device=dev)
        s = torch.randn(B, cin, device=dev)
        d = torch.rand(B, cout, device=dev) + 0.5
        oh = 2 * h if up else h
        noise = torch.randn(1, 1, oh, oh, device=dev)
        nw = torch.randn(1, device=dev)
        bias = torch.randn(cout, device=dev)
        flop = 2.0 * B * cin * cout * 9 * h * h
        if up:
            f = lambda: K._modconv_raw(K.MODE_UP, x, fwd, s, d, h, h)
            g = torch.randn(B, cout, 2 * h + 1, 2 * h + 1, device=dev)
            r = lambda: K._modconv_raw(K.MODE_DOWN, g, bwd, d, s, h, h, dot_with=x)
        else:
            f = lambda: K._modconv_raw(K.MODE_SAME, x, fwd, s, d, h, h, act=(noise, nw, bias))
            g = torch.randn(B, cout, h, h, device=dev)
            r = lambda: K._modconv_raw(K.MODE_SAME, g, bwd, d, s, h, h, dot_with=x)
        tf, tb = timeit(f, args.iters), timeit(r, args.iters)
        tot["fwd"][0] += tf; tot["fwd"][1] += flop; tot["bwd"][0] += tb; tot["bwd"][1] += flop
        name = f"{cin:3d}->{cout:3d} @{h:4d} {'up  ' if up else 'same'}"
        print(f"{name:28s} {flop / 1e9:8.2f} | {tf:8.3f} {flop / tf / 1e9:7.1f} | {tb:8.3f} {flop / tb / 1e9:7.1f}")
    for k, (ms, fl) in tot.items():
        print(f"total {k}: {ms:.3f} ms, {fl / 1e9:.1f} GFLOP, {fl / ms / 1e9:.1f} TFLOP/s")


if __name__ == "__main__":
    main()
