"""Shared by the mask-branch training tests (CPU and GPU): the float64 evaluation of the CPU oracle's region-attention net and the
scalar whose gradients tests/golden/attention_grad.npz records."""
import torch

import make_golden_attention as M
import seeded
from oracle import attention_net as OA


def is_mask_param(name):
    """The reference's test (run_attention.py:1078) over named_parameters(); `initial_state` is a buffer, not a parameter."""
    return (name.startswith("attention") or name.startswith("initial")) and name != "initial_state"


def seeded_state_dict(initial_bias=None):
    """The seeded state_dict of make_golden_attention.py (names and shapes from the package's net; net_state_dict looks at nothing else)."""
    from where2edit_amd.run_attention import FullSpaceMapperFEATClusterLinStyle_Net
    net = FullSpaceMapperFEATClusterLinStyle_Net(M.LAYERS, 1024, 512, attention_layer=M.ATT_LAYER, channel_multiplier=2,
                                                 cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS, cluster_dim=576)
    sd = M.net_state_dict(net)
    if initial_bias is not None:
        sd["initial_bias"] = torch.tensor([float(initial_bias)])
    return net, sd


def fixture_scalar(final_map, losses, r=None):
    """make_golden_attention_grad.scalar_of, restated for any device / dtype (`r`: the weights, already on the map's device)."""
    if r is None:
        r = seeded.tensor("attgrad.r", tuple(final_map.shape)).to(final_map)
    return (final_map * r).sum() + 2.0 * losses[1].sum() + 5.0 * losses[2]


def oracle_forward(sd, x, feats, size, att_text, dtype=torch.float64, **cfg):
    """OA.forward in `dtype` with every mask parameter a leaf that requires grad.  Returns (leaves by name, out, final, losses, extra)."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        osd = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        for k in osd:
            if is_mask_param(k):
                osd[k].requires_grad_(True)
        out, final, losses, extra = OA.forward(osd, [t.to(dtype) for t in x], [f.to(dtype) for f in feats], size,
                                               attention_text=att_text.to(dtype), **cfg)
    finally:
        torch.set_default_dtype(prev)
    return osd, out, final, losses, extra


def oracle_mask_grads(sd, x, feats, size, att_text, dtype=torch.float64, **cfg):
    """{name: gradient of fixture_scalar} for every mask parameter the oracle's forward uses, the unused names, and extras."""
    osd, _, final, losses, extra = oracle_forward(sd, x, feats, size, att_text, dtype, **cfg)
    names = [k for k in osd if is_mask_param(k)]
    grads = torch.autograd.grad(fixture_scalar(final, losses), [osd[n] for n in names], allow_unused=True)
    used = {n: g for n, g in zip(names, grads) if g is not None}
    return used, sorted(n for n, g in zip(names, grads) if g is None), extra


def cluster_means(extra, clusters):
    """[(sample, cluster, mean)] of the non-empty clusters of an oracle run."""
    each, choice = extra["each"].detach(), extra["choice"]
    return [(b, k, float(each[b][choice[b] == k].mean())) for b in range(each.shape[0]) for k in range(clusters) if (choice[b] == k).any()]


def fixture_entries(g):
    """[(fixture key, parameter name, row slice or None)] of attention_grad.npz."""
    rows = int(g["rows"])
    out = []
    for key in (str(n) for n in g["grad_names"]):
        if key.endswith(f"[:{rows}]"):
            out.append((key, key[:-len(f"[:{rows}]")], rows))
        else:
            out.append((key, key, None))
    return out
