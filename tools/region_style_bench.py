#!/usr/bin/env python3
"""Times the region-attention net's style branch (forward + backward) and one optimizer step at the shipped shape (26 S-space codes of
a 1024^2 generator, attention_layer = 13 -> 14 mapped codes, E = 512): the HIP node (csrc/region_style.hip) and where2edit_amd.Adam
(csrc/adam.hip) against the stock composition (W2E_RSTYLE_STOCK=1) and torch.optim.Adam(foreach=True).  HIP events around every
iteration, the median of --iters iterations after a warm-up; one JSON line per (case, batch, variant) with the dispatch count of one
iteration and the sum of its kernel times (`kernel_us`), both as torch.profiler sees them (null where it gives none): `median_us` is
the iteration as the stream sees it, host time included, `kernel_us` the device's share of it (`kernels_us`: per kernel, HIP branch).

    python tools/region_style_bench.py [--batches 1 8] [--iters 200] [--out profiles/region_style_bench.jsonl]
    python tools/region_style_bench.py --step-ab [--size 1024] [--batches 1 8] [--pairs 5] [--steps 20] [--out profiles/region_style_step_ab.txt]

--step-ab: RegionAttentionTrainer.train_step end to end (generator of --size, CLIP ViT-B/32, K = 20 clusters), two trainers with equal
weights in one process -- "hip" = the defaults, "stock" = W2E_RSTYLE_STOCK=1 + torch.optim.Adam, the behaviour before this path
existed --, run alternately, --pairs times each; a run's figure is the median HIP-event time of its --steps steps."""
import argparse
import copy
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import where2edit_amd  # noqa: E402
from where2edit_amd.run_attention import FullSpaceMapperFEATClusterLinStyle_Net, RegionAttentionTrainer  # noqa: E402

LAYERS, ATT, K = 18, 13, 20
DIMS = [512] * 15 + [256] * 3 + [128] * 3 + [64] * 3 + [32] * 2
COPY_RATE = 6.29e12  # bytes / s: the measured device-to-device copy rate of an MI355X (profiles/r03_mem_kernels_b4.txt)
DEV = "cuda"


def _net():
    return FullSpaceMapperFEATClusterLinStyle_Net(LAYERS, 1024, 512, attention_layer=ATT, channel_multiplier=2, cluster_layer=ATT, clusters=K,
                                                  cluster_dim=576).to(DEV).train()


def _timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times)


def _dispatches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [ev for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA]
        by_name = {}
        for ev in dev:  # "void w2e::rs_fwd_kernel<1, true>(w2e::RsGroups, float)" -> "rs_fwd_kernel<1, true>": the launches in order
            by_name.setdefault(ev.name.split("(")[0].replace("void ", "").replace("w2e::", ""), []).append(round(ev.time_range.elapsed_us(), 1))
        return (len(dev) or None), (round(sum(ev.time_range.elapsed_us() for ev in dev), 1) if dev else None), by_name
    except Exception:  # noqa: BLE001  (the counts are a courtesy; the timing does not depend on them)
        return None, None, {}


def micro(args):
    lines = []
    for batch in args.batches:
        torch.manual_seed(0)
        net = _net()
        for n, p in net.named_parameters():
            p.requires_grad_(n.startswith("mapper_"))
        text = 0.3 * torch.randn(batch, 1, 512, device=DEV)
        x = [torch.cat([text, 1.0 + 0.5 * torch.randn(batch, 1, d, device=DEV)], -1) for d in DIMS]
        x_text = x[0][:, 0, :512]
        mapped = net.mapper_layer
        probes = [torch.randn(batch, 1, d, 1, 1, device=DEV) for d in DIMS[:mapped]] + [torch.ones((), device=DEV)]
        weights = [p for n, p in net.named_parameters() if n.startswith("mapper_") and "textca" not in n and n.endswith("weight")]
        wbytes = 4 * sum(p.numel() for p in weights)

        def branch():
            out, loss = net.new_styles(x, x_text, 0.1)
            torch.autograd.backward([*out[:mapped], loss], probes)
            for p in net.parameters():
                p.grad = None

        for variant in ("hip", "stock"):
            if variant == "stock":
                os.environ["W2E_RSTYLE_STOCK"] = "1"
            else:
                os.environ.pop("W2E_RSTYLE_STOCK", None)
            med, best = _timed(branch, args.iters)
            lines.append({"case": "style_branch_fwd_bwd", "batch": batch, "variant": variant, "median_us": round(med, 1), "min_us": round(best, 1),
                          "weight_bytes": wbytes, "fraction_of_copy_rate": round(wbytes / (med * 1e-6) / COPY_RATE, 4), "iters": args.iters})
            lines[-1]["dispatches"], lines[-1]["kernel_us"], by_name = _dispatches(branch)
            if variant == "hip":
                lines[-1]["kernels_us"] = by_name
            if lines[-1]["kernel_us"]:
                lines[-1]["kernel_fraction_of_copy_rate"] = round(wbytes / (lines[-1]["kernel_us"] * 1e-6) / COPY_RATE, 4)
            print(json.dumps(lines[-1]), flush=True)
        os.environ.pop("W2E_RSTYLE_STOCK", None)
        # the optimizer: every trainable parameter of the shipped configuration (mapper_*, the unused mapper_textca_* have no gradient)
        out, loss = net.new_styles(x, x_text, 0.1)
        torch.autograd.backward([*out[:mapped], loss], probes)
        params = [p for p in net.parameters() if p.requires_grad]
        for variant, make in (("hip", lambda ps: where2edit_amd.Adam(ps, lr=0.01)), ("stock", lambda ps: torch.optim.Adam(ps, lr=0.01, foreach=True))):
            opt = make(params)
            med, best = _timed(opt.step, args.iters)
            n_t = sum(p.grad is not None for p in params)
            lines.append({"case": "adam_step", "batch": batch, "variant": variant, "median_us": round(med, 1), "min_us": round(best, 1),
                          "tensors": n_t, "param_bytes": 4 * sum(p.numel() for p in params if p.grad is not None),
                          "iters": args.iters})
            lines[-1]["dispatches"], lines[-1]["kernel_us"], _ = _dispatches(opt.step)
            print(json.dumps(lines[-1]), flush=True)
        del net
    return [json.dumps(ln) for ln in lines]


def step_ab(args):
    from where2edit_amd.attention_model import Generator
    from where2edit_amd.clip_loss import CLIPLoss
    from where2edit_amd.clip_vit import CLIP
    torch.manual_seed(0)
    g = Generator(args.size, 512, 8).to(DEV)
    clip = CLIP().to(DEV)
    n_latent = g.n_latent
    net = FullSpaceMapperFEATClusterLinStyle_Net(n_latent, 1024, 512, attention_layer=ATT, channel_multiplier=2, cluster_layer=ATT, clusters=K,
                                                 cluster_dim=576)
    loss = CLIPLoss(types.SimpleNamespace(stylegan_size=args.size), model=clip)
    out = []
    for batch in args.batches:
        trainers = {}
        for variant in ("hip", "stock"):
            tr = RegionAttentionTrainer(g, loss, copy.deepcopy(net), attention_layer=ATT, lr=0.01, steps=10000, device=DEV)
            if variant == "stock":
                tr.optimizer = torch.optim.Adam(tr.params, lr=0.01)
            trainers[variant] = tr
        gen = torch.Generator().manual_seed(1)
        w1 = torch.randn(batch, n_latent, 512, generator=gen).to(DEV)
        w2 = torch.randn(batch, n_latent, 512, generator=gen).to(DEV)
        text = torch.randn(batch, 512, generator=gen).to(DEV)

        def run(variant, steps):
            if variant == "stock":
                os.environ["W2E_RSTYLE_STOCK"] = "1"
            else:
                os.environ.pop("W2E_RSTYLE_STOCK", None)
            tr, times = trainers[variant], []
            for _ in range(steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                tr.train_step(w1, w2, text)
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            os.environ.pop("W2E_RSTYLE_STOCK", None)
            return statistics.median(times)

        for variant in ("hip", "stock"):
            run(variant, 3)  # warm-up: library load, allocator, tuning caches
        res = {"hip": [], "stock": []}
        for pair in range(args.pairs):
            for variant in ("hip", "stock") if pair % 2 == 0 else ("stock", "hip"):
                res[variant].append(run(variant, args.steps))
                out.append(f"size {args.size} batch {batch} pair {pair} {variant:5s} median step {res[variant][-1]:.3f} ms over {args.steps} steps")
                print(out[-1], flush=True)
        verdict = "every hip run <= every stock run" if max(res["hip"]) <= min(res["stock"]) else "NOT every hip run <= every stock run"
        out.append(f"size {args.size} batch {batch}: hip median {statistics.median(res['hip']):.3f} ms (max {max(res['hip']):.3f}), stock median "
                   f"{statistics.median(res['stock']):.3f} ms (min {min(res['stock']):.3f}): {verdict}")
        print(out[-1], flush=True)
        del trainers
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-ab", action="store_true")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = step_ab(args) if args.step_ab else micro(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
