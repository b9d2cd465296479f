"""Tensors derived from frozen parameters (packed conv weights, sum_k W^2, scaled EqualLinear products, stacked style affines,
K-quad-major ViT packs, IR-SE50 / VGG plans): one cache, keyed one way.

The contract, stated here and nowhere else: an entry is reused until one of the tensors it was built from changes identity,
`data_ptr()`, `_version` or `device`.  Optimizer steps, `load_state_dict`, `.to()` and every in-place op change one of those and the
entry rebuilds by itself.  A kernel that writes through raw pointers bumps the versions itself
(`torch.autograd.graph.increment_version`, as the fused optimizers do).  A write through `.data` (`p.data.mul_`, `p.data.copy_`, an
EMA `accumulate`) changes none of them: call `invalidate(module)` -- `stylegan2.invalidate_caches` -- after such writes."""
_names = set()  # every attribute name an entry was ever stored under: what `drop` removes
_holders = []


class Holder:
    """An owner for a cache that belongs to no module; `invalidate` drops every Holder's entries."""

    def __init__(self):
        _holders.append(self)


def derived(owner, slot, tensors, build):
    """`build()`'s result, stored in `owner.__dict__` (never in its state_dict).  `slot` is the private attribute name the entry is
    stored under (`"_plan"`), or a tuple that starts with one (`("_wsc_t", id(conv))`): the entries of such slots share one dict
    under that name.  `tensors`: a list or tuple of the tensors the result depends on; None entries (an absent bias) are allowed.
    The entry keeps references to them, so neither an `id()` nor an address can be recycled under it.  (On the hot path about thirty
    times per generator forward: a hit is a dict lookup and a compare per tensor, no tuple is built.)"""
    d = owner.__dict__
    if slot.__class__ is str:
        hit = d.get(slot)
    else:
        hit = d.get(slot[0])
        if hit is not None:
            hit = hit.get(slot)
    if hit is not None and len(hit[0]) == 4 * len(tensors):
        held, i = hit[0], 0  # held: (tensor, data_ptr, _version, device) per entry of `tensors`, flat
        for t in tensors:
            if held[i] is not t or (t is not None and (held[i + 1] != t.data_ptr() or held[i + 2] != t._version or held[i + 3] != t.device)):
                break
            i += 4
        else:
            return hit[1]
    held = []
    for t in tensors:
        held += (t, None, None, None) if t is None else (t, t.data_ptr(), t._version, t.device)
    value = build()
    if slot.__class__ is str:
        _names.add(slot)
        d[slot] = (held, value)
    else:
        _names.add(slot[0])
        d.setdefault(slot[0], {})[slot] = (held, value)
    return value


def drop(owner):
    """Forget every entry of one owner."""
    d = owner.__dict__
    for name in _names:
        d.pop(name, None)


def invalidate(module):
    """Drop every derived tensor under `module` and in every Holder, and CLIP's cached text features (keyed on token contents, with
    their own logic in clip_vit).  For callers that wrote parameters through `.data`."""
    for m in module.modules():
        drop(m)
        if hasattr(m, "_text_cache"):
            m._text_cache = None
    for h in _holders:
        drop(h)
