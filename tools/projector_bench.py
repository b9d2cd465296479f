#!/usr/bin/env python3
"""One projector step (where2edit_amd.project's loop body) at batch 1, for w and for W+, on the package's kernels against the same loop
with the projector's own arithmetic as stock torch ops, in the same process.

    python tools/projector_bench.py [--size 1024] [--lpips-size 256] [--runs 5] [--out profiles/projector_bench.jsonl]

Both variants run the same generator, LPIPS and Adam.  They differ in exactly what csrc/projector.hip adds:
    hip     noise_regularize / noise_normalize_ / loss_front on the kernels; the [1,1,H,W] maps go through the fused StyledConv, whose
            backward returns their gradient (w2e_noise_grad)
    stock   the literal projector.py expressions (torch.roll, reshape(...).mean([3, 5]), mean / std, F.mse_loss); the maps are handed
            over as [1,H,W] views, which sends every StyledConv through the unfused composition, where autograd gives the gradient
Timing: device events around one step; the two alternate, one step each, `--runs` times after a warm-up of both; medians, whichever way
they fall.  A second set of lines times each piece on its own (both ways), the regulariser and the normaliser on the generator's own
list of maps.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stock_regularize(noises):
    loss = 0
    for noise in noises:
        size = noise.shape[2]
        while True:
            loss = loss + (noise * torch.roll(noise, shifts=1, dims=3)).mean().pow(2) + (noise * torch.roll(noise, shifts=1, dims=2)).mean().pow(2)
            if size <= 8:
                break
            noise = noise.reshape([-1, 1, size // 2, 2, size // 2, 2]).mean([3, 5])
            size //= 2
    return loss


def stock_normalize_(noises):
    for noise in noises:
        mean, std = noise.mean(), noise.std()
        noise.data.add_(-mean).div_(std)


def stock_front(img, target, f):
    b, c, h, w = img.shape
    small = img.reshape(b, c, h // f, f, w // f, f).mean([3, 5]) if f > 1 else img
    return small, F.mse_loss(small, target)


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
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--lpips-size", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import where2edit_amd as W
    from where2edit_amd._lib import call, ptr, stream_ptr
    from where2edit_amd.lpips import LPIPS
    from where2edit_amd.stylegan2 import Generator
    torch.manual_seed(0)
    dev = "cuda"
    g_ema = Generator(args.size, 512, 8)
    for m in g_ema.modules():
        if hasattr(m, "noise") and hasattr(m.noise, "weight"):
            torch.nn.init.normal_(m.noise.weight, std=0.1)  # (the constructor's zero strengths would make every noise gradient zero)
    g_ema = g_ema.to(dev).eval().requires_grad_(False)
    lpips = LPIPS().to(dev)
    side = min(args.size, args.lpips_size)
    f = args.size // side
    target = torch.tanh(0.8 * torch.randn(1, 3, side, side, device=dev))
    mean, std = W.latent_statistics(g_ema, 4096)
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    for w_plus in (False, True):
        def make():
            latent = mean.clone().unsqueeze(1).repeat(1, g_ema.n_latent, 1) if w_plus else mean.clone()
            latent = latent.contiguous().requires_grad_(True)
            noises = [torch.randn_like(n).requires_grad_(True) for n in g_ema.make_noise()]
            return latent, noises, W.Adam([latent] + noises, lr=0.01)

        hl, hn, hopt = make()
        sl, sn, sopt = make()

        def hip_step():
            img, _ = g_ema([W.latent_noise(hl, std * 0.05)], input_is_latent=True, noise=hn)
            small, mse = W.loss_front(img, target, f)
            loss = lpips(small, target).sum() + 1e5 * W.noise_regularize(hn) + 0.1 * mse
            hopt.zero_grad()
            loss.backward()
            hopt.step()
            W.noise_normalize_(hn)

        def stock_step():
            img, _ = g_ema([W.latent_noise(sl, std * 0.05)], input_is_latent=True, noise=[n[0] for n in sn])
            small, mse = stock_front(img, target, f)
            loss = lpips(small, target).sum() + 1e5 * stock_regularize(sn) + 0.1 * mse
            sopt.zero_grad()
            loss.backward()
            sopt.step()
            stock_normalize_(sn)

        ms_h, ms_s = alternate(hip_step, stock_step, args.runs)
        emit({"tool": "projector_bench", "what": "one step", "latent": "W+" if w_plus else "w", "size": args.size, "lpips_size": side,
              "batch": 1, "hip_ms": round(ms_h, 3), "stock_ms": round(ms_s, 3), "speedup_vs_stock": round(ms_s / ms_h, 3), "runs": args.runs})
        del hl, hn, hopt, sl, sn, sopt
        torch.cuda.empty_cache()

    # the pieces on their own
    noises = [torch.randn_like(n).requires_grad_(True) for n in g_ema.make_noise()]
    floats = sum(n.numel() for n in noises)

    def reg(fn):
        def run():
            torch.autograd.grad(1e5 * fn(noises), noises)
        return run
    ms_h, ms_s = alternate(reg(W.noise_regularize), reg(stock_regularize), args.runs)
    emit({"tool": "projector_bench", "what": "noise_regularize forward + backward", "maps": len(noises), "floats": floats,
          "hip_ms": round(ms_h, 4), "stock_ms": round(ms_s, 4), "runs": args.runs})
    a = [n.detach().clone() for n in noises]
    b = [n.detach().clone() for n in noises]
    ms_h, ms_s = alternate(lambda: W.noise_normalize_(a), lambda: stock_normalize_(b), args.runs)
    emit({"tool": "projector_bench", "what": "noise_normalize_", "maps": len(noises), "floats": floats, "hip_ms": round(ms_h, 4),
          "stock_ms": round(ms_s, 4), "one_pass_mb": round(2 * floats * 4 / 1e6, 1), "runs": args.runs})
    img = torch.randn(1, 3, args.size, args.size, device=dev, requires_grad=True)

    def front(fn):
        def run():
            small, mse = fn(img, target, f)
            torch.autograd.grad((small * target).sum() + 0.1 * mse, img)
        return run
    ms_h, ms_s = alternate(front(W.loss_front), front(stock_front), args.runs)
    emit({"tool": "projector_bench", "what": "loss front forward + backward", "size": args.size, "f": f, "hip_ms": round(ms_h, 4),
          "stock_ms": round(ms_s, 4), "one_pass_mb": round(2 * img.numel() * 4 / 1e6, 1), "runs": args.runs})
    planes = g_ema.channels[args.size]
    gpre = torch.randn(planes, args.size * args.size, device=dev)
    nw, out = torch.full((1,), 0.1, device=dev), torch.empty(args.size * args.size, device=dev)
    ms_h, ms_s = alternate(lambda: call("w2e_noise_grad", ptr(gpre), ptr(nw), ptr(out), planes, args.size * args.size, 0, stream_ptr()),
                           lambda: gpre.sum(0).mul_(nw), args.runs)
    mb = gpre.numel() * 4 / 1e6
    emit({"tool": "projector_bench", "what": "w2e_noise_grad (stock: sum over planes, mul)", "planes": planes, "pixels": args.size ** 2,
          "hip_ms": round(ms_h, 4), "stock_ms": round(ms_s, 4), "one_pass_mb": round(mb, 1), "hip_gb_s": round(mb / ms_h, 1), "runs": args.runs})
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("".join(json.dumps(v) + "\n" for v in lines))


if __name__ == "__main__":
    main()
