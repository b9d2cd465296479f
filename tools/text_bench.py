"""CLIP text tower (ViT-B/32: width 512, 12 layers, 8 heads, context 77) on the HIP kernels (vit_hip.text_forward) against the stock
composition (CLIP._encode_text_stock) at batch 1, 8 and 24 (24 = the region-attention loop's three encode_text calls at batch 8).  Both
paths run in one process on seeded weights, alternating call by call; each is timed with device events around single calls after a
warm-up, and the median of --iters calls is reported with the FLOP count of the shapes.

    python tools/text_bench.py [--batches 1,8,24] [--iters 30] [--out FILE.jsonl]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/text_bench.py --hip-only --batches 24 --iters 20

--hip-only times the HIP path alone (for a kernel trace of it)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import seeded  # noqa: E402
from where2edit_amd.clip_vit import CLIP  # noqa: E402

WIDTH, LAYERS, HEADS, CTX, VOCAB, EMBED = 512, 12, 8, 77, 49408, 512


def model():
    m = CLIP(embed_dim=EMBED, image_resolution=32, vision_layers=1, vision_width=64, vision_patch_size=32, context_length=CTX,
             vocab_size=VOCAB, transformer_width=WIDTH, transformer_heads=HEADS, transformer_layers=LAYERS)
    m.load_state_dict(seeded.clip_state_dict(embed_dim=EMBED, image_resolution=32, vision_layers=1, vision_width=64, vision_patch=32,
                                             context_length=CTX, vocab_size=VOCAB, text_width=WIDTH, text_layers=LAYERS), strict=True)
    return m.requires_grad_(False).to("cuda").eval()


def tokens(b, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(b, CTX, dtype=torch.int64)
    for i in range(b):
        n = 1 + (i * 13) % (CTX - 1)
        t[i, 0] = VOCAB - 2
        t[i, 1:n] = torch.randint(1, VOCAB - 2, (n - 1,), generator=g)
        t[i, n] = VOCAB - 1
    return t.to("cuda")


def flops(b, l=CTX, d=WIDTH):
    """GEMMs of the 12 blocks (QKV 3d^2, out-proj d^2, MLP 8d^2 per token), the full L x L attention products (as the stock path
    computes them) and the projection."""
    return b * (LAYERS * (2 * l * 12 * d * d + 4 * l * l * d) + 2 * d * EMBED)


def time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,24")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from where2edit_amd import vit_hip
    m = model()
    lines = []
    for b in [int(v) for v in args.batches.split(",")]:
        t = tokens(b, seed=b)
        assert vit_hip.text_hip_ok(m, t)
        with torch.no_grad():
            hip = lambda: m.encode_text(t)  # noqa: E731
            stock = lambda: m._encode_text_stock(t)  # noqa: E731
            for _ in range(args.warmup):
                hip()
                if not args.hip_only:
                    stock()
            th, ts = [], []
            for _ in range(args.iters):
                th.append(time_once(hip))
                if not args.hip_only:
                    ts.append(time_once(stock))
            err = None if args.hip_only else ((hip() - stock()).abs().max() / stock().abs().max()).item()
        med = lambda v: sorted(v)[len(v) // 2] if v else None  # noqa: E731
        f = flops(b)
        line = {"tool": "text_bench", "batch": b, "context": CTX, "width": WIDTH, "layers": LAYERS, "gflop": round(f / 1e9, 2),
                "iters": args.iters, "hip_ms": round(med(th), 4), "hip_tflops": round(f / med(th) / 1e9, 2)}
        if ts:
            line.update(stock_ms=round(med(ts), 4), stock_tflops=round(f / med(ts) / 1e9, 2), speedup=round(med(ts) / med(th), 2),
                        hip_vs_stock_rel_err=float(f"{err:.3e}"))
        line["device"] = torch.cuda.get_device_name()
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
