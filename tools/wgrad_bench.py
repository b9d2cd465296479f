"""Per-layer time of the conv-weight gradient (w2e_modconv_wgrad + w2e_modconv_wgrad_finish) for the 17 styled convs of the 1024^2
generator, at batch 1, 4 and 8 (HIP events, median of --iters), with the forward convolution of the same layer (ModulatedConv2d,
frozen weight, default Winograd selection) beside it and TFLOP/s against the 157.3 TF fp32-MFMA peak.

    python tools/wgrad_bench.py [--batches 1,4,8] [--iters 10] [--stock]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/wgrad_bench.py --steps 3 --batches 4

--steps N instead runs N fine-tuning steps of the 1024^2 generator (every conv weight trained: forward, CLIP preprocessing, backward
into the weights) after one warm-up step, for a kernel trace of the whole step (profiles/wgrad_step_b4_kernel_stats_summary.txt).

--stock also times torch.nn.grad.conv2d_weight on the per-sample grouped form (the reference's arithmetic on MIOpen) for the
same-resolution layers -- a comparison inside this tool only; the library never calls it."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from where2edit_amd import _lib  # noqa: E402
from where2edit_amd import functional as K  # noqa: E402
from where2edit_amd.stylegan2 import ModulatedConv2d  # noqa: E402

PEAK_TF = 157.3
CH = {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}


def layers(size=1024):
    out = [("conv1 4^2", 512, 512, 4, False)]
    res = 8
    while res <= size:
        out.append((f"up {res // 2}->{res}", CH[res // 2], CH[res], res // 2, True))
        out.append((f"same {res}^2", CH[res], CH[res], res, False))
        res *= 2
    return out


def timed(fn, iters):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def fine_tuning_steps(b, steps, size=1024):
    from where2edit_amd.stylegan2 import Generator, train_conv_weights
    g = Generator(size, 512, 8).to("cuda").eval().requires_grad_(False)
    train_conv_weights(g)
    w = torch.randn(b, g.n_latent, 512, device="cuda")
    gclip = torch.randn(b, 3, 224, 224, device="cuda")
    for i in range(steps + 1):  # (step 0: warm-up)
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        img, _ = g([w], input_is_latent=True, randomize_noise=False)
        K.clip_preprocess(img).backward(gclip)
        e.record()
        e.synchronize()
        print(json.dumps({"step": i, "batch": b, "ms": round(a.elapsed_time(e), 3)}), flush=True)
        g.zero_grad(set_to_none=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--stock", action="store_true")
    ap.add_argument("--steps", type=int, default=0)
    args = ap.parse_args()
    _lib.load()
    dev = "cuda"
    if args.steps:
        return fine_tuning_steps(int(args.batches.split(",")[0]), args.steps)
    gen = torch.Generator(device=dev).manual_seed(0)
    for b in [int(v) for v in args.batches.split(",")]:
        tot_w = tot_f = 0.0
        for name, cin, cout, h, up in layers():
            x = torch.randn(b, cin, h, h, device=dev, generator=gen)
            gh = 2 * h + 1 if up else h
            g = torch.randn(b, cout, gh, gh, device=dev, generator=gen)
            s = torch.rand(b, cin, device=dev, generator=gen) + 0.5
            d = torch.rand(b, cout, device=dev, generator=gen) + 0.5
            dz = torch.randn(b, cout, device=dev, generator=gen)
            weight = torch.randn(1, cout, cin, 3, 3, device=dev, generator=gen)
            mode = K.WGRAD_UP if up else K.WGRAD_SAME
            t_w = timed(lambda: K.modconv_wgrad(mode, g, x, d, s, weight, 0.1, dz=dz), args.iters)
            m = ModulatedConv2d(cin, cout, 3, 512, upsample=up).to(dev).requires_grad_(False)
            st = torch.randn(b, 512, device=dev, generator=gen)
            with torch.no_grad():
                t_f = timed(lambda: m(x, st), args.iters)
            flops = 2.0 * b * cin * cout * 9 * h * h
            line = {"batch": b, "layer": name, "cin": cin, "cout": cout, "wgrad_ms": round(t_w, 4),
                    "wgrad_tflops": round(flops / t_w / 1e9, 2), "wgrad_pct_peak": round(100 * flops / t_w / 1e9 / PEAK_TF, 1),
                    "fwd_conv_ms": round(t_f, 4)}
            if args.stock and not up:
                wmod = (0.1 * weight * s.view(b, 1, cin, 1, 1)).reshape(b * cout, cin, 3, 3)
                xg, gg = (x * s.view(b, cin, 1, 1)).reshape(1, b * cin, h, h), (g * d.view(b, cout, 1, 1)).reshape(1, b * cout, h, h)
                line["stock_grouped_ms"] = round(timed(lambda: torch.nn.grad.conv2d_weight(xg, wmod.shape, gg, padding=1, groups=b),
                                                       args.iters), 4)
            tot_w += t_w
            tot_f += t_f
            print(json.dumps(line), flush=True)
            del x, g
        print(json.dumps({"batch": b, "total_wgrad_ms": round(tot_w, 3), "total_fwd_conv_ms": round(tot_f, 3)}), flush=True)


if __name__ == "__main__":
    main()
