"""Generates tests/golden/attention_grad.npz: the REFERENCE's own gradients through the mask branch of its region-attention
mapper net (attention/run_attention.py:796-884), on the seeded problem of make_golden_attention.py (imported, not restated).

    python tests/golden/make_golden_attention_grad.py        (needs the reference checkout; never runs on the GPU box)

    scalar = (final_map * r).sum() + 2 * loss_reg + 5 * loss_tv

with respect to a named subset of the `attention*` / `initial*` parameters: whole small tensors, and the first rows of the large
`attention_textca_*.weight` matrices ("<name>[:ROWS]").  The noise strengths stay 0 (net_state_dict), so the randn the reference
draws in every NoiseInjection does not reach the map; the strengths' own gradients (sum g_pre * randn) are not recorded.
The seeded problem is a 256^2-shaped generator with channel_multiplier 2: its source convs have 512, 256 and 128 input channels."""
import os

import numpy as np
import torch

import make_golden_attention as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 4


def scalar_of(final_map, losses):
    r = M.seeded.tensor("attgrad.r", tuple(final_map.shape))
    return (final_map * r.to(final_map)).sum() + 2.0 * losses[1].sum() + 5.0 * losses[2]


def whole_names(all_names):
    keep = ["initial_bias", "attention_first.conv.weight", "attention_14.conv.weight", "attention_18.conv.weight",
            "attention_last.conv.weight"]
    keep += [n for n in all_names if n.startswith("attention") and n.endswith("activate.bias")]
    keep += [n for n in all_names if n.startswith("attention_textca_") and n.endswith(".bias")]
    return keep


def sliced_names(all_names):
    return [n for n in all_names if n.startswith("attention_textca_") and n.endswith(".weight")]


def main():
    ra = M.import_reference_net()
    torch.manual_seed(0)
    net = ra.FullSpaceMapperFEATClusterLinStyle_Net(M.LAYERS, 1024, 512, attention_layer=M.ATT_LAYER, channel_multiplier=2,
                                                    cluster_layer=M.CLUSTER_LAYER, clusters=M.CLUSTERS, cluster_dim=576)
    net.load_state_dict(M.net_state_dict(net), strict=True)
    net.train()
    x, att_text, _ = M.inputs()
    _, final_map, losses = net(x, M.feature_maps(), M.SIZE, attention_text=att_text)
    params = dict(net.named_parameters())
    names = [n for n in params if n.startswith("attention") or n.startswith("initial")]
    grads = torch.autograd.grad(scalar_of(final_map, losses), [params[n] for n in names], allow_unused=True)
    g = dict(zip(names, grads))
    unused = sorted(n for n in names if g[n] is None)
    assert unused and all(".conv.modulation." in n for n in unused), unused  # input_is_stylespace=True: the modulation is never called
    store = {"unused": np.asarray(unused), "rows": np.int64(ROWS)}
    for n in whole_names(names):
        store["grad." + n] = g[n].numpy()
    for n in sliced_names(names):
        store[f"grad.{n}[:{ROWS}]"] = g[n][:ROWS].numpy()
    store["grad_names"] = np.asarray(sorted(k[5:] for k in store if k.startswith("grad.")))
    path = os.path.join(HERE, "attention_grad.npz")
    np.savez_compressed(path, **store)
    print("saved", path, os.path.getsize(path), "bytes,", len(store["grad_names"]), "gradients")


if __name__ == "__main__":
    main()
