"""The style branch of `FullSpaceMapperFEATClusterLinStyle_Net` (attention/run_attention.py:811-828) as ONE autograd node on
libw2e.so's grouped EqualLinear kernels (csrc/region_style.hip, w2e_rstyle_*).  Per S-space code c below `mapper_layer`

    x_text_hidden = mapper_text_c(x_text)               2 x EqualLinear(fused_lrelu)
    x_c_hidden    = mapper_c(x_c)                       EqualLinear
    x_c_new       = x_c + alpha * (mapper_all_c(x_c_hidden || x_text_hidden) - x_c)
    loss_delta   += mean_b ||x_c_new - x_c|| / mapper_layer

A layer of ALL codes is one launch per direction (32 groups per launch; a further launch beyond that):

    forward   1  mapper_c  +  mapper_text_c[0]   (one launch: the groups of a launch may come from different families; x_c and
                                                  x_text are read in place out of the caller's [B, 1, E + d_c] rows)
              2  mapper_text_c[1]
              3  mapper_all_c on (x_c_hidden || x_text_hidden), the concatenation never materialised
              4  the finish: x_new, the row norms, loss_delta                                            (4 calls, 5 kernels)
    backward  1  finish: gy = alpha * (g_out + g_loss * diff / ||diff|| / (B * mapper_layer))
              2  weight / bias gradients of mapper_all_c        3  its input gradient -> g_hidden, g_text_hidden
              4  weight / bias gradients of mapper_c and mapper_text_c[1] (one launch)
              5  input gradient of mapper_text_c[1]             6  weight / bias gradients of mapper_text_c[0]

Differentiable in the parameters only (the codes and the text features are inputs of the loop, never trained).  No host
synchronisation and no allocation outside torch's allocator: safe inside hipGraph capture."""
import ctypes
import os

import torch
from torch.autograd.function import once_differentiable

from . import _lib

MAX_GROUPS = 32   # RS_MAXG: groups per launch, and the most codes the node takes
MAX_BATCH = 16    # RS_MAXB


def _pa(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _ia(values):
    return (ctypes.c_int * len(values))(*values)


def _fa(values):
    return (ctypes.c_float * len(values))(*values)


def _chunks(n):
    return [(i, min(i + MAX_GROUPS, n)) for i in range(0, n, MAX_GROUPS)]


def _linear_fwd(batch, groups, b_scale, stream):
    """groups: (src0, src1, k0, k1, ld0, ld1, w, bias, out, n, w_scale, act) with device addresses as ints."""
    for lo, hi in _chunks(len(groups)):
        col = list(zip(*groups[lo:hi]))
        _lib.call("w2e_rstyle_linear_fwd", hi - lo, batch, _pa(col[0]), _pa(col[1]), _ia(col[2]), _ia(col[3]), _ia(col[4]), _ia(col[5]),
                  _pa(col[6]), _pa(col[7]), _pa(col[8]), _ia(col[9]), _fa(col[10]), float(b_scale), _ia(col[11]), stream)


def _linear_dgrad(batch, groups, stream):
    """groups: (gy, y, w, gx0, gx1, k0, k1, n, w_scale, act)."""
    for lo, hi in _chunks(len(groups)):
        col = list(zip(*groups[lo:hi]))
        _lib.call("w2e_rstyle_linear_dgrad", hi - lo, batch, _pa(col[0]), _pa(col[1]), _pa(col[2]), _pa(col[3]), _pa(col[4]), _ia(col[5]),
                  _ia(col[6]), _ia(col[7]), _fa(col[8]), _ia(col[9]), stream)


def _linear_wgrad(batch, groups, b_scale, stream):
    """groups: (gy, y, src0, src1, k0, k1, ld0, ld1, gw, gb, n, w_scale, act)."""
    for lo, hi in _chunks(len(groups)):
        col = list(zip(*groups[lo:hi]))
        _lib.call("w2e_rstyle_linear_wgrad", hi - lo, batch, _pa(col[0]), _pa(col[1]), _pa(col[2]), _pa(col[3]), _ia(col[4]), _ia(col[5]),
                  _ia(col[6]), _ia(col[7]), _pa(col[8]), _pa(col[9]), _ia(col[10]), _fa(col[11]), float(b_scale), _ia(col[12]), stream)


def _offsets(sizes):
    """Float offsets of consecutive blocks, each rounded up to 4 floats (16 bytes), and the total."""
    off, at = [], 0
    for s in sizes:
        off.append(at)
        at += (s + 3) & ~3
    return off, at


class _Geom:
    """The shapes of one call: per code c the width d_c and the row stride of x[c]; the row stride of x_text; E, the text hidden width H, the text output
    width T; the scales."""

    def __init__(self, batch, embed, dims, ldx, ldt, hidden, tout, scales, b_scale, alpha, layers):
        self.batch, self.embed, self.dims, self.ldx, self.ldt, self.hidden, self.tout = batch, embed, dims, ldx, ldt, hidden, tout
        self.scales, self.b_scale, self.alpha, self.layers = scales, b_scale, alpha, layers  # scales[c] = (mapper, text0, text1, all)
        b = batch
        self.off_d, self.n_d = _offsets([b * d for d in dims])          # [B, d_c] blocks: x_c_hidden, y, x_new, gy, g_hidden
        self.off_h, self.n_h = _offsets([b * hidden] * len(dims))       # [B, H] blocks: the text hidden layer
        self.off_t, self.n_t = _offsets([b * tout] * len(dims))         # [B, T] blocks: x_text_hidden


class _RegionStyle(torch.autograd.Function):
    """apply(geom, x_text [B, E], *x (G tensors [B, 1, E + d_c]), *params) with params = G weights then G biases of mapper_c, mapper_text_c[0],
    mapper_text_c[1], mapper_all_c (family-major).  Returns G new codes [B, 1, d_c, 1, 1] (views of one packed buffer) and
    loss_delta (0-dim)."""

    @staticmethod
    def forward(ctx, geom, x_text, *args):
        g = len(geom.dims)
        xs, params = args[:g], args[g:]
        b, e, h, t = geom.batch, geom.embed, geom.hidden, geom.tout
        dev = xs[0].device
        wm, bm, wt0, bt0, wt1, bt1, wa, ba = (params[i * g:(i + 1) * g] for i in range(8))
        st = _lib.stream_ptr()
        work = torch.empty(3 * geom.n_d + geom.n_h + geom.n_t + g * b + 4, device=dev, dtype=torch.float32)
        hid, y, xnew = work[:geom.n_d], work[geom.n_d:2 * geom.n_d], work[2 * geom.n_d:3 * geom.n_d]
        at = 3 * geom.n_d
        t1, t2 = work[at:at + geom.n_h], work[at + geom.n_h:at + geom.n_h + geom.n_t]
        at += geom.n_h + geom.n_t
        norms, loss = work[at:at + g * b], work[at + g * b:at + g * b + 1]
        P = lambda tens, off=0: tens.data_ptr() + 4 * off  # noqa: E731
        xc = [P(x, e) for x in xs]                     # x_c = x[c][:, 0, E:]
        xt = P(x_text)                                 # (x[0][:, 0, :E] in the net's forward: read in place, row stride ldt)
        groups = []
        for c, d in enumerate(geom.dims):
            groups.append((xc[c], 0, d, 0, geom.ldx[c], 0, P(wm[c]), P(bm[c]), P(hid, geom.off_d[c]), d, geom.scales[c][0], 0))
        for c in range(g):
            groups.append((xt, 0, e, 0, geom.ldt, 0, P(wt0[c]), P(bt0[c]), P(t1, geom.off_h[c]), h, geom.scales[c][1], 1))
        _linear_fwd(b, groups, geom.b_scale, st)
        _linear_fwd(b, [(P(t1, geom.off_h[c]), 0, h, 0, h, 0, P(wt1[c]), P(bt1[c]), P(t2, geom.off_t[c]), t, geom.scales[c][2], 1)
                        for c in range(g)], geom.b_scale, st)
        _linear_fwd(b, [(P(hid, geom.off_d[c]), P(t2, geom.off_t[c]), d, t, d, t, P(wa[c]), P(ba[c]), P(y, geom.off_d[c]), d,
                         geom.scales[c][3], 0) for c, d in enumerate(geom.dims)], geom.b_scale, st)
        _lib.call("w2e_rstyle_finish_fwd", g, b, _pa(xc), _ia(geom.ldx), _pa([P(y, o) for o in geom.off_d]),
                  _pa([P(xnew, o) for o in geom.off_d]), _ia(geom.dims), float(geom.alpha), int(geom.layers), _lib.ptr(norms), _lib.ptr(loss), st)
        ctx.geom = geom
        ctx.save_for_backward(work, x_text, *xs, *wt1, *wa)
        outs = [xnew[o:o + b * d].view(b, 1, d, 1, 1) for o, d in zip(geom.off_d, geom.dims)]
        return (*outs, loss.view(()))

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        geom = ctx.geom
        g = len(geom.dims)
        b, e, h, t = geom.batch, geom.embed, geom.hidden, geom.tout
        saved = ctx.saved_tensors
        work, x_text, xs, wt1, wa = saved[0], saved[1], saved[2:2 + g], saved[2 + g:2 + 2 * g], saved[2 + 2 * g:2 + 3 * g]
        dev = work.device
        st = _lib.stream_ptr()
        P = lambda tens, off=0: tens.data_ptr() + 4 * off  # noqa: E731
        hid, y = work[:geom.n_d], work[geom.n_d:2 * geom.n_d]
        at = 3 * geom.n_d
        t1, t2 = work[at:at + geom.n_h], work[at + geom.n_h:at + geom.n_h + geom.n_t]
        at += geom.n_h + geom.n_t
        norms = work[at:at + g * b]
        xc = [P(x, e) for x in xs]
        xt = P(x_text)
        g_loss = gouts[g]
        gsrc = [go.contiguous().float() if go is not None else None for go in gouts[:g]]
        g_loss = g_loss.contiguous().float() if g_loss is not None else None
        # the parameter gradients, one packed buffer (every block 16-byte aligned), family-major like `params`
        shapes = ([(d, d) for d in geom.dims] + [(d,) for d in geom.dims] + [(h, e)] * g + [(h,)] * g + [(t, h)] * g + [(t,)] * g +
                  [(d, d + t) for d in geom.dims] + [(d,) for d in geom.dims])
        sizes = [s[0] * (s[1] if len(s) > 1 else 1) for s in shapes]
        goff, gtotal = _offsets(sizes)
        gbuf = torch.empty(gtotal, device=dev, dtype=torch.float32)
        padded = [(n + 3) & ~3 for n in sizes]
        grads = [(blk if n == m else blk[:n]).view(s) for blk, n, m, s in zip(gbuf.split_with_sizes(padded), sizes, padded, shapes)]
        gwm, gbm, gwt0, gbt0, gwt1, gbt1, gwa, gba = (goff[i * g:(i + 1) * g] for i in range(8))
        G = lambda off: P(gbuf, off)  # noqa: E731
        # activations' gradients: gy and g_hidden ([B, d_c] blocks), g_t2 ([B, T]), g_t1 ([B, H])
        tmp = torch.empty(2 * geom.n_d + geom.n_t + geom.n_h, device=dev, dtype=torch.float32)
        gy, ghid = tmp[:geom.n_d], tmp[geom.n_d:2 * geom.n_d]
        gt2, gt1 = tmp[2 * geom.n_d:2 * geom.n_d + geom.n_t], tmp[2 * geom.n_d + geom.n_t:]
        _lib.call("w2e_rstyle_finish_bwd", g, b, _pa(xc), _ia(geom.ldx), _pa([P(y, o) for o in geom.off_d]),
                  _pa([None if s is None else s.data_ptr() for s in gsrc]), _lib.ptr(norms), _lib.ptr(g_loss),
                  _pa([P(gy, o) for o in geom.off_d]), _ia(geom.dims), float(geom.alpha), int(geom.layers), st)
        sc = geom.scales
        _linear_wgrad(b, [(P(gy, geom.off_d[c]), 0, P(hid, geom.off_d[c]), P(t2, geom.off_t[c]), d, t, d, t, G(gwa[c]), G(gba[c]), d,
                           sc[c][3], 0) for c, d in enumerate(geom.dims)], geom.b_scale, st)
        _linear_dgrad(b, [(P(gy, geom.off_d[c]), 0, P(wa[c]), P(ghid, geom.off_d[c]), P(gt2, geom.off_t[c]), d, t, d, sc[c][3], 0)
                          for c, d in enumerate(geom.dims)], st)
        groups = [(P(ghid, geom.off_d[c]), 0, xc[c], 0, d, 0, geom.ldx[c], 0, G(gwm[c]), G(gbm[c]), d, sc[c][0], 0)
                  for c, d in enumerate(geom.dims)]
        groups += [(P(gt2, geom.off_t[c]), P(t2, geom.off_t[c]), P(t1, geom.off_h[c]), 0, h, 0, h, 0, G(gwt1[c]), G(gbt1[c]), t, sc[c][2], 1)
                   for c in range(g)]
        _linear_wgrad(b, groups, geom.b_scale, st)
        _linear_dgrad(b, [(P(gt2, geom.off_t[c]), P(t2, geom.off_t[c]), P(wt1[c]), P(gt1, geom.off_h[c]), 0, h, 0, t, sc[c][2], 1)
                          for c in range(g)], st)
        _linear_wgrad(b, [(P(gt1, geom.off_h[c]), P(t1, geom.off_h[c]), xt, 0, e, 0, geom.ldt, 0, G(gwt0[c]), G(gbt0[c]), h, sc[c][1], 1)
                          for c in range(g)], geom.b_scale, st)
        del gsrc
        return (None, None, *([None] * g), *grads)


def _plan(net, x, x_text):
    """The checks of `applies`; returns (geom without alpha, parameter list) or None."""
    from .stylegan2 import EqualLinear
    if os.environ.get("W2E_RSTYLE_STOCK"):
        return None
    layers = getattr(net, "mapper_layer", None)
    e = getattr(net, "latent_dim", None)
    if not isinstance(layers, int) or not isinstance(e, int) or e < 1 or not isinstance(x, (list, tuple)) or not x:
        return None
    g = min(len(x), layers)
    if g < 1 or g > MAX_GROUPS:
        return None
    x0 = x[0]
    if not (torch.is_tensor(x0) and x0.is_cuda and x0.dim() == 3):
        return None
    b, dev = x0.shape[0], x0.device
    if b < 1 or b > MAX_BATCH:
        return None
    if not (torch.is_tensor(x_text) and x_text.device == dev and x_text.dtype == torch.float32 and tuple(x_text.shape) == (b, e) and
            x_text.stride(1) == 1 and x_text.stride(0) >= e) or x_text.requires_grad:
        return None
    dims, ldx = [], []
    for c in range(g):
        xc = x[c]
        if not (torch.is_tensor(xc) and xc.device == dev and xc.dtype == torch.float32 and xc.dim() == 3 and xc.shape[0] == b and
                xc.shape[1] == 1 and xc.shape[2] > e and xc.is_contiguous()) or xc.requires_grad:
            return None
        dims.append(xc.shape[2] - e)
        ldx.append(xc.shape[2])
    fams = [[], [], [], []]
    for c in range(g):
        mp, tx, al = (getattr(net, f"{n}_{c}", None) for n in ("mapper", "mapper_text", "mapper_all"))
        if not (isinstance(mp, EqualLinear) and isinstance(al, EqualLinear) and isinstance(tx, torch.nn.Sequential) and len(tx) == 2 and
                all(isinstance(m, EqualLinear) for m in tx)):
            return None
        if mp.activation or al.activation or tx[0].activation != "fused_lrelu" or tx[1].activation != "fused_lrelu":
            return None
        for fam, m in zip(fams, (mp, tx[0], tx[1], al)):
            fam.append(m)
    h, t = fams[1][0].weight.shape[0], fams[2][0].weight.shape[0]
    mb = 1 << (b - 1).bit_length()
    if b * max(max(dims), t) + 256 * mb + 4 > 16384:  # the input-gradient kernel stages gy .* act'(y) of a group in 64 KB of LDS
        return None
    lr_mul = fams[0][0].lr_mul
    for c in range(g):
        want = ((dims[c], dims[c]), (h, e), (t, h), (dims[c], dims[c] + t))
        for fam, shape in zip(fams, want):
            m = fam[c]
            if tuple(m.weight.shape) != shape or m.bias is None or m.lr_mul != lr_mul:
                return None
            for p in (m.weight, m.bias):
                if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                    return None
    try:
        _lib.load()
    except (RuntimeError, OSError):
        return None
    scales = [tuple(float(fam[c].scale) for fam in fams) for c in range(g)]
    params = []
    for fam in fams:
        params += [m.weight for m in fam] + [m.bias for m in fam]
    return (b, e, dims, ldx, int(x_text.stride(0)), h, t, scales, float(lr_mul), int(layers)), params


def applies(net, x, x_text):
    """Does the node take this call?  It needs: `W2E_RSTYLE_STOCK` unset; x a list of CUDA fp32 contiguous [B, 1, E + d_c] tensors and x_text a
    [B, E] fp32 tensor with unit inner stride on one device, none requiring grad, B <= 16; at most 32 codes below `net.mapper_layer`; for each of them the modules the reference
    builds (run_attention.py:712-722) -- `mapper_c` = EqualLinear(d_c, d_c), `mapper_text_c` = Sequential of two fused_lrelu
    EqualLinears (E -> H -> T), `mapper_all_c` = EqualLinear(d_c + T, d_c), all with a bias, one lr_mul, contiguous fp32 parameters
    on x's device --; and a loadable libw2e.so.  Returns a plan (truthy) or None: the caller then composes the stock modules."""
    return _plan(net, x, x_text)


def new_styles(net, x, x_text, strength_alpha=0.1):
    """(list of len(x) codes [B, 1, d_c, 1, 1], loss_delta) as `net.new_styles` returns them, or None where `applies` says no."""
    plan = _plan(net, x, x_text) if isinstance(strength_alpha, (int, float)) else None
    if plan is None:
        return None
    (b, e, dims, ldx, ldt, h, t, scales, b_scale, layers), params = plan
    geom = _Geom(b, e, dims, ldx, ldt, h, t, scales, b_scale, float(strength_alpha), layers)
    g = len(dims)
    with torch.cuda.device(x[0].device):
        res = _RegionStyle.apply(geom, x_text, *x[:g], *params)
    out = list(res[:g])
    for c in range(g, len(x)):
        out.append(x[c][:, :, e:].unsqueeze(3).unsqueeze(3))
    return out, res[g]
