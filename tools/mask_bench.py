#!/usr/bin/env python3
"""Times the region-attention mask branch at the shipped shapes (1024^2 generator: 18 sources, 4..1024 resolution, 512..32 channels;
attention_layer = cluster_layer = 13 -> size 64, K = 20): forward (frozen, the default path) and forward + backward (opted in,
run_attention.train_mask_branch) on the HIP kernels, against a stock-op composition of the same branch written here (full-resolution
grouped F.conv2d, F.interpolate, index_add for the cluster means) -- the only way the branch could be trained without the backward
kernels.  One JSON line per (batch, variant).

    python tools/mask_bench.py [--batches 1 4 8] [--iters 20] [--out profiles/mask_train_bench.jsonl] [--profile-step B]

--profile-step B runs warm-up + 3 opted-in steps at batch B and nothing else (for `rocprofv3 --kernel-trace --stats -- python ...`)."""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from where2edit_amd.run_attention import (FullSpaceMapperFEATClusterLinStyle_Net, _ClusterPoolTrain, cluster_pool,  # noqa: E402
                                          freeze_mask_branch, train_mask_branch)

LAYERS, ATT, K, SIZE = 18, 13, 20, 64
RES = [4, 4] + [r for r in (8, 16, 32, 64, 128, 256, 512, 1024) for _ in range(3)]
CH = [512, 3] + [c for c in (512, 512, 512, 512, 256, 128, 64, 32) for c in (c, c, 3)]


def problem(batch, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    feats = [torch.randn(batch, c, r, r, device=dev, generator=g) for r, c in zip(RES, CH)]
    feats.append(torch.randn(1, 512, 4, 4, device=dev, generator=g).repeat(batch, 1, 1, 1))
    net = FullSpaceMapperFEATClusterLinStyle_Net(LAYERS, 1024, 512, attention_layer=ATT, channel_multiplier=2, cluster_layer=ATT,
                                                 clusters=K, cluster_dim=576).to(dev).train()
    dims = [512] * 15 + [256] * 3 + [128] * 3 + [64] * 3 + [32] * 3
    text = 0.3 * torch.randn(batch, 512, device=dev, generator=g)
    x = [torch.cat([text.unsqueeze(1), 1.0 + 0.5 * torch.randn(batch, 1, dims[c], device=dev, generator=g)], -1) for c in range(26)]
    r = torch.randn(batch, 1, SIZE, SIZE, device=dev, generator=g)
    return net, x, feats, text, r


def mask_params(net):
    return [p for n, p in net.named_parameters() if (n.startswith("attention") or n.startswith("initial")) and ".conv.modulation." not in n]


def stock_mask_branch(net, feats, size, attention_text, n_codes, assign):
    """The mask branch of the reference's forward (:796-884) on stock ops: every source convolved at full resolution."""
    b = attention_text.shape[0]
    acts = []

    def styled_1x1(sc, feat, style):
        w = sc.conv.weight[0, :, :, 0, 0] * sc.conv.scale                      # [O,C]
        wm = w[None] * style[:, None, :]                                       # [B,O,C]
        wm = wm * torch.rsqrt(wm.square().sum(2, keepdim=True) + sc.conv.eps)
        o, c, h = w.shape[0], w.shape[1], feat.shape[2]
        y = F.conv2d(feat.reshape(1, b * c, h, h), wm.reshape(b * o, c, 1, 1), groups=b).reshape(b, o, h, h)
        y = y + sc.noise.weight * torch.randn(b, 1, h, h, device=feat.device)
        return F.leaky_relu(y + sc.activate.bias.view(1, -1, 1, 1), 0.2) * math.sqrt(2)

    for sc, aff, fi in net._sources(n_codes):
        acts.append(F.interpolate(styled_1x1(sc, feats[fi], aff(attention_text)), size))
    each = styled_1x1(net.attention_last, torch.cat(acts, 1), net.attention_textca_last(attention_text))
    each = torch.sigmoid(each + net.initial_bias).view(b, size * size)
    ids = F.interpolate(assign[:, None].float(), size).long().view(b, size * size)
    sums = torch.zeros(b, K, device=each.device).scatter_add(1, ids, each)
    counts = torch.zeros(b, K, device=each.device).scatter_add(1, ids, torch.ones_like(each))
    means = sums / counts.clamp_min(1)
    same = means.gather(1, ids)
    loss_reg = (torch.relu(means - 0.7) * (counts > 0)).sum() / b
    loss_tv = F.mse_loss(each, same.detach())
    amap = same.view(b, 1, size, size)
    thr = torch.where(amap < 0.8, amap - amap.detach(), amap)
    t = torch.linspace(-2, 2, 5, device=each.device)
    k1 = torch.exp(-0.5 * (t / 1.1) ** 2)
    k1 = k1 / k1.sum()
    final = F.conv2d(F.pad(thr, [2, 2, 2, 2], mode="reflect"), (k1[:, None] * k1[None, :])[None, None])
    return final, loss_reg, loss_tv


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"ms_median": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1], "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-step", type=int, default=0)
    ap.add_argument("--no-stock", action="store_true")
    a = ap.parse_args()
    dev = "cuda:0"
    lines = []
    for batch in ([a.profile_step] if a.profile_step else a.batches):
        net, x, feats, text, r = problem(batch, dev)
        params = mask_params(net)

        def hip_forward():
            each, assign = net.attention_map(feats, SIZE, text, len(x))  # (the cluster assignment is part of the HIP timings only)
            return cluster_pool(each, assign, SIZE, K)

        def hip_train():
            each, assign = net.attention_map_train(feats, SIZE, text, len(x))
            final, reg, tv = _ClusterPoolTrain.apply(each, assign, SIZE, K)[:3]
            return torch.autograd.grad((final * r).sum() + 2.0 * reg.sum() + 5.0 * tv, params)

        if a.profile_step:
            train_mask_branch(net)
            for _ in range(4):
                hip_train()
            torch.cuda.synchronize()
            return
        freeze_mask_branch(net)
        res = {"hip_forward": timed(hip_forward, a.iters)}
        train_mask_branch(net)
        res["hip_forward_backward"] = timed(hip_train, a.iters)
        if not a.no_stock:
            assign = net.attention_map(feats, SIZE, text, len(x))[1]

            def stock_forward():
                with torch.no_grad():
                    return stock_mask_branch(net, feats, SIZE, text, len(x), assign)

            def stock_train():
                final, reg, tv = stock_mask_branch(net, feats, SIZE, text, len(x), assign)
                return torch.autograd.grad((final * r).sum() + 2.0 * reg + 5.0 * tv, params)

            res["stock_forward"] = timed(stock_forward, max(3, a.iters // 4), 2)
            res["stock_forward_backward"] = timed(stock_train, max(3, a.iters // 4), 2)
        # the bytes a perfect gather would move: one float per (sample, channel, kept pixel); the 64-byte lines it touches at res > size
        useful = batch * sum(s[0].conv.in_channel for s in net._sources(len(x))) * SIZE * SIZE * 4
        for name, t in res.items():
            lines.append({"tool": "mask_bench", "batch": batch, "size": SIZE, "sources": 18, "variant": name, "gathered_bytes": useful,
                          "note": "mask branch only; the hip_* variants include w2e_cluster_assign, the stock_* ones are handed its result", **t})
            print(json.dumps(lines[-1]), flush=True)
        del net, x, feats
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
