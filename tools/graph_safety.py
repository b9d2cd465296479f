#!/usr/bin/env python3
"""Memset / memcpy operations of one eager mapper step (they become memset / memcpy NODES under hipGraph capture; on this ROCm
stack a captured hipMemsetAsync was observed not to be replayed, so a step that is to be captured should contain none that
matter).  usage: graph_safety.py [workload batch]   |   graph_safety.py mask [batch]  (the opt-in mask-branch forward + backward)"""
import collections
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


MEMOPS = ("emcpy", "copyBuffer", "emset", "fillBuffer")


def memops(prof):
    """Counter of (device op, CPU call chain, input shapes) over the memset / memcpy device operations of a profile."""
    cnt = collections.Counter()
    for e in prof.events():
        for k in (e.kernels or []):
            if any(m in k.name for m in MEMOPS):
                par, chain = e, []
                while par is not None and len(chain) < 4:
                    chain.append(par.name)
                    par = par.cpu_parent
                cnt[(k.name[:32], " <- ".join(chain), str(e.input_shapes)[:70])] += 1
    return cnt


def mask_branch_memops(batch=2, size=16):
    """memops() of the two opt-in mask-branch Functions (run_attention._MaskLogitsTrain, _ClusterPoolTrain), forward + backward, on
    seeded inputs already resident on the GPU: what the new kernels' host code itself issues."""
    from where2edit_amd.run_attention import _ClusterPoolTrain, _MaskLogitsTrain
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).cuda()  # noqa: E731
    shapes = ((512, 4), (256, 32), (32, 64))
    feats = [rnd(batch, c, r, r) for c, r in shapes]
    per = []
    for c, _ in shapes:
        per += [rnd(c, 32) / c ** 0.5, rnd(batch, c) + 1.0, rnd(32), rnd(1)]
    small = [rnd(32 * len(shapes)) / 10, rnd(batch, 32 * len(shapes)) + 1.0, rnd(1), rnd(1), rnd(1)]
    leaves = [t.requires_grad_(True) for t in small + per]
    noises = [rnd(batch, size * size) for _ in range(len(shapes) + 1)]
    assign = torch.randint(0, 5, (batch, size, size), generator=gen).int().cuda()
    r = rnd(batch, 1, size, size)

    def run():
        each = _MaskLogitsTrain.apply(feats, noises, size, 1e-8, 1e-8, *leaves)
        final, reg, tv = _ClusterPoolTrain.apply(each, assign, size, 6)[:3]
        return torch.autograd.grad((final * r).sum() + reg.sum() + tv, leaves)

    run()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA], record_shapes=True) as prof:
        run()
        torch.cuda.synchronize()
    return memops(prof)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "mask":
        cnt = mask_branch_memops(int(sys.argv[2]) if len(sys.argv) > 2 else 2)
        print(f"# memset / memcpy operations in the opt-in mask-branch forward + backward: {sum(cnt.values())}")
        for (k, chain, shp), n in cnt.most_common(60):
            print(n, k, "|", chain, "|", shp)
        return
    import bench
    WL = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    coach = bench.build_coach(1024, B, "cuda:0", False, "hip", WL)
    w = bench.synthetic_latents(coach.net.decoder, B, 0)
    mask = bench.make_mask(coach, B, 1024, 0, "cuda:0", False) if WL == 3 else None
    for _ in range(3):
        coach.train_step(w, mask)
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA], record_shapes=True) as prof:
        coach.optimizer.zero_grad()
        x, x_hat, w_hat = coach.forward_pair(w, mask)
        loss, d = coach.calc_loss(w, x, w_hat, x_hat)
        loss.backward()
        torch.cuda.synchronize()
    cnt = memops(prof)
    print(f"# memset / memcpy operations in zero_grad + forward + losses + backward (workload {WL}, batch {B}): {sum(cnt.values())}")
    for (k, chain, shp), n in cnt.most_common(60):
        print(n, k, "|", chain, "|", shp)


if __name__ == "__main__":
    main()
