"""The StyleGAN2 Discriminator at 1024^2, channel_multiplier 2, on the HIP kernels (stylegan2.Discriminator) against the stock-op
composition of the reference's arithmetic (tests/disc64.py's restatement in fp32: torch / MIOpen convolutions) at batch 1, 4 and 8.
Three variants each: forward; forward + input gradient with a frozen D (the generator step); forward + every gradient (the D step).
Device-event timing around single calls after a warm-up; the median of --iters calls, with TFLOP/s against the arithmetic of the
convolutions (~150 GFLOP per image forward, the backward twice that with weight gradients, once without).
The variant `r1` (not in the default list; batch 4 and 8 are the ones of interest) times one `d.r1_penalty(x).backward()` (four passes over D)
next to the D step of the same run and next to the stock-op composition: stock D, autograd.grad(create_graph=True), backward.

    python tools/disc_bench.py [--batches 1,4,8] [--iters 10] [--out FILE.jsonl]
    python tools/disc_bench.py --batches 4,8 --variants dstep,r1 --out profiles/r1_bench.jsonl
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/disc_bench.py --hip-only --batches 4 --variants dstep --iters 5"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import disc64  # noqa: E402
from where2edit_amd.stylegan2 import Discriminator  # noqa: E402

SIZE, CM = 1024, 2


def conv_flop(size=SIZE, cm=CM):
    """Forward FLOP of the convolutions of one image (2 per multiply-add): fromRGB, conv1 / conv2 / skip of every block, final_conv."""
    ch = lambda r: disc64.channels(r, cm)  # noqa: E731
    f = 2.0 * 3 * ch(size) * size * size
    r = size
    while r > 4:
        c, n = ch(r), ch(r // 2)
        f += 2.0 * 9 * c * c * r * r + 2.0 * 9 * c * n * (r // 2) ** 2 + 2.0 * c * n * (r // 2) ** 2
        r //= 2
    return f + 2.0 * 9 * 513 * 512 * 16


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--variants", default="fwd,gstep,dstep")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = disc64.state_dict(SIZE, CM)
    d = Discriminator(SIZE, CM)
    d.load_state_dict(sd, strict=True)
    d = d.cuda()
    sdc = {k: v.cuda() for k, v in sd.items()}
    params_stock = {k: v.clone().requires_grad_(not k.endswith(".kernel")) for k, v in sdc.items()}
    fl = conv_flop()
    lines = []
    for b in [int(v) for v in a.batches.split(",")]:
        x = disc64.images(b, SIZE).cuda()
        for var in a.variants.split(","):
            # r1: forward, reverse, tangent forward + its weight gradients (two forwards' worth), plus the small fourth pass
            mult = {"fwd": 1.0, "gstep": 2.0, "dstep": 3.0, "r1": 5.0}[var]

            def hip():
                if var == "fwd":
                    with torch.no_grad():
                        d(x)
                    return
                d.requires_grad_(var in ("dstep", "r1"))
                if var == "r1":
                    torch.autograd.grad(d.r1_penalty(x), [p for k, p in d.named_parameters() if k != "final_linear.1.bias"])
                    return
                xx = x.requires_grad_(var == "gstep")
                loss = d(xx).sum()
                if var == "gstep":
                    torch.autograd.grad(loss, [xx])
                else:
                    torch.autograd.grad(loss, [p for p in d.parameters()])

            def stock():
                if var == "fwd":
                    with torch.no_grad():
                        disc64.forward(sdc, x)
                    return
                if var == "r1":
                    xx = x.clone().requires_grad_(True)
                    (g,) = torch.autograd.grad(disc64.forward(params_stock, xx).sum(), [xx], create_graph=True)
                    ps = [v for k, v in params_stock.items() if not k.endswith(".kernel") and k != "final_linear.1.bias"]
                    torch.autograd.grad(g.pow(2).reshape(b, -1).sum(1).mean(), ps, allow_unused=True)
                elif var == "gstep":
                    xx = x.clone().requires_grad_(True)
                    torch.autograd.grad(disc64.forward(sdc, xx).sum(), [xx])
                else:
                    ps = [v for k, v in params_stock.items() if not k.endswith(".kernel")]
                    torch.autograd.grad(disc64.forward(params_stock, x).sum(), ps)

            rec = {"batch": b, "variant": var, "hip_ms": round(timed(hip, a.iters), 3)}
            rec["hip_tflops"] = round(mult * fl * b / rec["hip_ms"] / 1e9, 1)
            if not a.hip_only:
                rec["stock_ms"] = round(timed(stock, a.iters), 3)
                rec["stock_tflops"] = round(mult * fl * b / rec["stock_ms"] / 1e9, 1)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            if a.out:  # rewritten after every record: a run that is cut short leaves the lines it measured
                with open(a.out, "w") as f:
                    for r in lines:
                        f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
