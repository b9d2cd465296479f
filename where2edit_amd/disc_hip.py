"""The StyleGAN2 Discriminator (models/stylegan2/model.py:577-705) on the hand-written kernels: forward, input gradient and, for the
parameters that require grad, parameter gradients.  stylegan2.ConvLayer / ResBlock / Discriminator call in here.

Decomposition:
  fromRGB      w2e_fromrgb_fwd / _bwd (K8): the K = 3 1x1 conv + bias + LeakyReLU*sqrt2, its input gradient and deterministic
               weight / bias partials.
  ResBlock     conv1  w2e_conv3x3 SAME (irse_hip.conv3x3: its Winograd-form choice too), bias + PReLU(0.2) epilogue;
               conv2  Blur(pad=(2,2)) of conv1's output -> [B,C,H+1,W+1], then w2e_conv3x3 DOWN, down_pad 0, same epilogue;
               skip   Blur(pad=(2,2)) of the input, then the centre tap of a DOWN 3x3: blurred-skip index j of the reference's
                      Blur(pad=(1,1)) is index j+1 of the pad-(2,2) blur, so the stride-2 1x1 conv reads exactly the (1,1) tap;
               out    conv2 + skip in a separate in-place pass (w2e_shortcut_add_bwd).  The 1/sqrt2 of `(out + skip) / sqrt2` is
                      folded into the weights: conv2 stores lrelu(z2) (its sqrt2 cancels), the skip pack carries 1/sqrt2, and
                      lrelu(z2) itself is kept for the backward, whose branch test needs its sign (the sum has lost it).
               Every activation a ResBlock keeps is lrelu(z) WITHOUT the sqrt2; the consumer's pack carries it (LeakyReLU is
               positively homogeneous, so this is exact up to rounding).
  final_conv   w2e_mbstd_fwd writes [x | stddev] as one [B,C+1,4,4] tensor (513 channels: the conv engine zero-fills the pack past
               K, so the extra channel needs no padding), w2e_conv3x3 SAME + bias + PReLU(0.2), then w2e_affine_act_fwd * sqrt2.
  final_linear the package's EqualLinear (rocBLAS through torch), as in the generator's mapping network.
Backward: the SAME adjoint through the flipped transposed pack, the DOWN adjoint as W2E_CONV_UP phase-planar output, the blur adjoint
through w2e_upfirdn2d(in_layout = 1), the activation backward through w2e_affine_act_bwd; weight gradients through w2e_modconv_wgrad
SAME / DOWN / DOWN-CENTRE with unit styles and no demodulation, biases from w2e_channel_sums.  No atomics, no memsets, no host
synchronisation: bit-reproducible and capturable.  Generic double backward (create_graph=True) is not supported: every node is
once_differentiable and raises when differentiated a second time.
R1 (the gradient penalty mean_b |d sum(D(x)) / dx_b|^2 of the D regularisation step) has its own entry point, r1_penalty: ONE autograd
node (_R1) over D's parameters, forward-over-reverse in four passes ("R1"):
  1 primal forward   the layers above, keeping what their backward keeps;
  2 reverse for g    the backward bodies above with the cotangent 1, keeping every pre-activation cotangent gz_l, the cotangent of each
                     block's output and of the stddev channel; r1 from w2e_sumsq_rows (two stages, fixed order);
  3 tangent forward  along dx = (2/B) * g (the incoming gradient scales the finished gradients): convs without bias, LeakyReLU as the mask of the kept activation
                     (w2e_affine_act_bwd), w2e_fromrgb_jvp, w2e_mbstd_jvp; as each tangent appears, the weight gradient of the layer
                     it feeds is wgrad(gz_l, tangent) through the same weight-gradient calls as the first-order backward;
  4 primal reverse   w2e_mbstd_hvp gives the one second-order term (the stddev layer's), which runs through the ordinary backward
                     of everything below the stddev layer: the only source of bias gradients."""
import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import functional as K
from . import irse_hip as IR
from ._lib import call, ptr, stream_ptr
from .derived import derived

SQRT2 = math.sqrt(2.0)
SLOPE = 0.2
WGRAD_SAME, WGRAD_CENTRE, WGRAD_DOWN, WGRAD_DOWN_CENTRE = 0, 2, 3, 4

_VEC = {}


def _const(device, n, value):
    """A cached [n] (or [b, n]) device vector filled with `value`: the PReLU slopes, the unit styles of the weight gradient."""
    key = (device, n, value)
    v = _VEC.get(key)
    if v is None:
        shape = n if isinstance(n, tuple) else (n,)
        v = torch.full(shape, value, device=device, dtype=torch.float32)
        _VEC[key] = v
    return v


def stddev_group(batch):
    """model.py:691: group = min(B, 4); the reference's view() needs B % group == 0."""
    g = min(batch, 4)
    if batch % g:
        raise ValueError(f"Discriminator minibatch stddev: batch {batch} must be a multiple of the stddev group min(batch, 4) = {g} "
                         "(model.py:691-694 views the batch as [group, batch / group])")
    return g


# ---------------------------------------------------------------------------------------------- raw kernel calls
def blur(x):
    """Blur(pad=(2,2)) of the 4-tap [1,3,3,1] kernel: [B,C,H,W] -> [B,C,H+1,W+1] (the [2h+1] input of W2E_CONV_DOWN, down_pad 0)."""
    b, c, h, w = x.shape
    return K._upfirdn2d_raw(x, _blur_kernel(x.device), h + 1, w + 1, 1, 1, 2, 2, flip=True)


def blur_adjoint(t, h, w):
    """Adjoint of `blur` applied to the phase-planar UP output T [B,C,2,2,h/2+1,WP] of a [h+1,w+1] image: -> [B,C,h,w]."""
    if K.fir_planar_ok((4, 4), w):  # the tile kernel reads the phase-planar layout directly
        return K._upfirdn2d_raw(t, _blur_kernel(t.device), h, w, 1, 1, 1, 1, flip=False, planar_hw=(h + 1, w + 1))
    # tiny images (<= 16^2 after the block): re-interleave (a [B,C,<=17,<=17] copy) and use the generic kernel, as the generator does
    return K._upfirdn2d_raw(K.unplanar(t, w // 2), _blur_kernel(t.device), h, w, 1, 1, 1, 1, flip=False)


def _blur_kernel(device):
    k = _VEC.get(("blur", device))
    if k is None:
        k = torch.tensor([1.0, 3.0, 3.0, 1.0])
        k = (k[None, :] * k[:, None]) / 64.0
        k = k.to(device).contiguous()
        _VEC[("blur", device)] = k
    return k


def wgrad(mode, g, x, cout, cin, taps, scale):
    """dW [cout, cin, k, k] = scale * C(g, x) (w2e_modconv_wgrad, unit styles, then _finish with d = NULL).  g [B,cout,h,w]; x [B,cin,h,w]
    (SAME / CENTRE) or [B,cin,2h+1,2w+1] (DOWN / DOWN-CENTRE)."""
    b, _, h, w = g.shape
    splits = ctypes.c_int(0)
    call("w2e_modconv_wgrad_plan", mode, b, cin, cout, h, w, ctypes.byref(splits))
    slab = torch.empty(splits.value * taps * cout * cin, device=g.device, dtype=torch.float32)
    st = stream_ptr()
    call("w2e_modconv_wgrad", mode, ptr(g), ptr(x), None, ptr(_const(g.device, (b, cin), 1.0)), ptr(slab), b, cin, cout, h, w,
         splits.value, st)
    k = 1 if taps == 1 else 3
    dw = torch.empty((cout, cin, k, k), device=g.device, dtype=torch.float32)
    call("w2e_modconv_wgrad_finish", ptr(slab), splits.value, None, None, None, None, None, None, None, ptr(dw), b, cin, cout, taps,
         float(scale), st)
    return dw


def bias_grad(g):
    """sum over batch and pixels of g [B,C,h,w] -> [C] (w2e_channel_sums, then the [B,C] column sum)."""
    return IR.channel_sums(g).sum(0)


def fromrgb_fwd(x, weight, bias, scale):
    b, _, h, w = x.shape
    c = weight.shape[0]
    y = torch.empty((b, c, h, w), device=x.device, dtype=torch.float32)
    call("w2e_fromrgb_fwd", ptr(x), ptr(weight), ptr(bias), ptr(y), b, c, h * w, float(scale), stream_ptr())
    return y


def fromrgb_bwd(gy, y, x, weight, scale, need_x, need_w, need_b):
    b, c, h, w = y.shape
    gx = torch.empty_like(x) if need_x else None
    dw = torch.empty((c, 3, 1, 1), device=y.device, dtype=torch.float32) if need_w else None
    db = torch.empty((c,), device=y.device, dtype=torch.float32) if need_b else None
    part = None
    if need_w or need_b:
        rows = _lib.load().w2e_fromrgb_bwd_rows(b, h * w)
        part = torch.empty((rows, c, 4), device=y.device, dtype=torch.float32)
    call("w2e_fromrgb_bwd", ptr(gy), ptr(y), ptr(x), ptr(weight), ptr(gx), ptr(part), ptr(dw), ptr(db), b, c, h * w, float(scale),
         stream_ptr())
    return gx, dw, db


def mbstd_fwd(x):
    b, c, h, w = x.shape
    stddev_group(b)
    y = torch.empty((b, c + 1, h, w), device=x.device, dtype=torch.float32)
    call("w2e_mbstd_fwd", ptr(x), ptr(y), b, c, h * w, stream_ptr())
    return y


def mbstd_bwd(gy, x):
    b, c, h, w = x.shape
    gx = torch.empty_like(x)
    call("w2e_mbstd_bwd", ptr(gy), ptr(x), ptr(gx), b, c, h * w, stream_ptr())
    return gx


def fromrgb_jvp(dx, y, weight, scale):
    """The tangent of fromrgb_fwd along dx [B,3,h,w], from the saved output y: sqrt2 * mask(y) * scale * W dx (no bias)."""
    b, c, h, w = y.shape
    t = torch.empty_like(y)
    call("w2e_fromrgb_jvp", ptr(dx), ptr(y), ptr(weight), ptr(t), b, c, h * w, float(scale), stream_ptr())
    return t


def mbstd_jvp(x, dx):
    """The tangent of mbstd_fwd along dx: [dx | d stddev] as one [B,C+1,h,w] tensor."""
    b, c, h, w = x.shape
    stddev_group(b)
    y = torch.empty((b, c + 1, h, w), device=x.device, dtype=torch.float32)
    call("w2e_mbstd_jvp", ptr(x), ptr(dx), ptr(y), b, c, h * w, stream_ptr())
    return y


def mbstd_hvp(gy, x, dx):
    """d/dx of <gy[:, C], d stddev(x, dx)> [B,C,h,w]: gy [B,C+1,h,w] as mbstd_bwd takes it (only the stddev channel is read)."""
    b, c, h, w = x.shape
    stddev_group(b)
    mu = torch.empty_like(x)
    call("w2e_mbstd_hvp", ptr(gy), ptr(x), ptr(dx), ptr(mu), b, c, h * w, stream_ptr())
    return mu


def sumsq_rows(x):
    """[B, n] -> [B]: the per-row sum of squares, two stages of fixed order (no atomics)."""
    b, n = x.shape
    parts = _lib.load().w2e_sumsq_rows_parts(n)
    part = torch.empty((b, max(parts, 1)), device=x.device, dtype=torch.float32)
    out = torch.empty((b,), device=x.device, dtype=torch.float32)
    call("w2e_sumsq_rows", ptr(x), ptr(part), ptr(out), b, n, stream_ptr())
    return out


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------------------------- autograd nodes
class _FromRGB(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, scale):
        x = _c(x)
        y = fromrgb_fwd(x, weight.detach(), bias.detach(), scale)
        ctx.scale = scale
        ctx.save_for_backward(x, weight, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        nx, nw, nb = ctx.needs_input_grad[:3]
        gx, dw, db = fromrgb_bwd(_c(gy), y, x, weight.detach(), ctx.scale, nx, nw, nb)
        return gx, dw, db, None


class _ConvAct(torch.autograd.Function):
    """ConvLayer(C, N, 3): EqualConv2d(pad 1, no bias) + FusedLeakyReLU(N), stride 1: lrelu(z) from the conv epilogue, then * sqrt2."""

    @staticmethod
    def forward(ctx, x, weight, bias, plan):
        x = _c(x)
        b, c, h, w = x.shape
        n = weight.shape[0]
        t = IR.conv3x3(x, plan["wf"], n, h, w, bias=bias.detach(), slope=_const(x.device, n, SLOPE))
        y = IR.affine_act(t, _const(x.device, n, SQRT2))
        ctx.plan = plan
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        p = ctx.plan
        b, c, h, w = x.shape
        n = y.shape[1]
        gz = IR.affine_act_bwd(_c(gy), y, _const(y.device, n, SQRT2), _const(y.device, n, SLOPE), b, n, h, w)
        nx, nw, nb = ctx.needs_input_grad[:3]
        gx = IR.conv3x3(gz, p["wb"], c, h, w) if nx else None
        dw = wgrad(WGRAD_SAME, gz, x, n, c, 9, p["scale"]) if nw else None
        db = bias_grad(gz) if nb else None
        return gx, dw, db, None


class _MbStd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.save_for_backward(x)
        return mbstd_fwd(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return mbstd_bwd(_c(gy), x)


def _resblock_fwd(x, b1, b2, plan, n, form=None):
    """The ResBlock forward body: (out, t1, xb, t2, xs).  form: IR.conv3x3's (None = its own choice for the stride-1 conv, 0 = the direct kernel)."""
    b, c, h, w = x.shape
    oh, ow = h // 2, w // 2
    dev = x.device
    t1 = IR.conv3x3(x, plan["w1f"], c, h, w, bias=b1, slope=_const(dev, c, SLOPE), form=form)                   # lrelu(z1)
    xb = blur(t1)
    t2 = IR.conv3x3(xb, plan["w2f"], n, oh, ow, mode=K.MODE_DOWN, down_pad=0, bias=b2, slope=_const(dev, n, SLOPE))
    xs = blur(x)
    out = IR.conv3x3(xs, plan["wsf"], n, oh, ow, mode=K.MODE_DOWN, down_pad=0)                           # skip / sqrt2
    call("w2e_shortcut_add_bwd", ptr(out), ptr(t2), b, n, oh, ow, 1, 0, stream_ptr())                     # out = t2 + skip
    return out, t1, xb, t2, xs


def _resblock_bwd(p, x, t1, xb, t2, xs, gout, needs, form=None):
    """The ResBlock backward body for the cotangent gout: (gx, dw1, db1, dw2, db2, dws) as `needs` asks, and the two pre-activation
    cotangents (gz1, gz2) it went through (gz1 None when nothing needed it)."""
    nx, nw1, nb1, nw2, nb2, nws = needs
    b, n, oh, ow = gout.shape
    c, h, w = t1.shape[1], t1.shape[2], t1.shape[3]
    dev = gout.device
    gz2 = IR.affine_act_bwd(gout, t2, None, _const(dev, n, SLOPE), b, n, oh, ow)
    gx = gz1 = None
    if nx or nw1 or nb1:
        tb = IR.conv3x3(gz2, p["w2b"], c, oh, ow, mode=K.MODE_UP)                                     # d/d blur(t1), phase-planar
        gz1 = IR.affine_act_bwd(blur_adjoint(tb, h, w), t1, None, _const(dev, c, SLOPE), b, c, h, w)
    if nx:
        gx = IR.conv3x3(gz1, p["w1b"], c, h, w, form=form)
        ts = IR.conv3x3(gout, p["wsb"], c, oh, ow, mode=K.MODE_UP)                                    # d/d blur(x), skip branch
        call("w2e_shortcut_add_bwd", ptr(gx), ptr(blur_adjoint(ts, h, w)), b, c, h, w, 1, 0, stream_ptr())
    dw1 = wgrad(WGRAD_SAME, gz1, x, c, c, 9, p["s1"]) if nw1 else None
    db1 = bias_grad(gz1) if nb1 else None
    dw2 = wgrad(WGRAD_DOWN, gz2, xb, n, c, 9, p["s2"]) if nw2 else None
    db2 = bias_grad(gz2) if nb2 else None
    dws = wgrad(WGRAD_DOWN_CENTRE, gout, xs, n, c, 1, p["ss"]) if nws else None
    return (gx, dw1, db1, dw2, db2, dws), (gz1, gz2)


class _ResBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, ws, plan):
        x = _c(x)
        out, t1, xb, t2, xs = _resblock_fwd(x, b1.detach(), b2.detach(), plan, w2.shape[0])
        keep = any(ctx.needs_input_grad[1:6])  # the weight gradients read x and the two blurred tensors
        ctx.plan = plan
        ctx.save_for_backward(x if keep else None, t1, xb if keep else None, t2, xs if keep else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, t1, xb, t2, xs = ctx.saved_tensors
        grads, _ = _resblock_bwd(ctx.plan, x, t1, xb, t2, xs, _c(gout), ctx.needs_input_grad[:6])
        return grads + (None,)


# ---------------------------------------------------------------------------------------------- plans (packed weights)
def _live(*params):
    return torch.is_grad_enabled() and any(q.requires_grad for q in params)


def _cached(mod, params, derive):
    """Packed weights of `mod`: derived in every forward while a parameter is trained (graph replays and optimizer steps then see the
    live weights), else cached (derived.py)."""
    if _live(*params):
        return derive()
    return derived(mod, "_cache", params, derive)


def resblock_plan(block):
    w1, w2, ws = block.conv1[0].weight, block.conv2[1].weight, block.skip[1].weight
    s1, s2, ss = block.conv1[0].scale, block.conv2[1].scale * SQRT2, block.skip[1].scale / SQRT2

    def derive():
        with torch.no_grad():
            w1d, w2d = w1.detach().float(), w2.detach().float()
            w9 = torch.nn.functional.pad(ws.detach().float(), (1, 1, 1, 1))  # the 1x1 skip as the centre tap of a 3x3
            return {"w1f": K.conv_pack(w1d, s1, False, False), "w1b": K.conv_pack(w1d, s1, True, True),
                    "w2f": K.conv_pack(w2d, s2, False, False), "w2b": K.conv_pack(w2d, s2, True, False),
                    "wsf": K.conv_pack(w9, ss, False, False), "wsb": K.conv_pack(w9, ss, True, False),
                    "s1": s1, "s2": s2, "ss": ss}

    return _cached(block, (w1, w2, ws), derive)


def convact_plan(layer):
    wt = layer[0].weight
    scale = layer[0].scale

    def derive():
        with torch.no_grad():
            wd = wt.detach().float()
            return {"wf": K.conv_pack(wd, scale, False, False), "wb": K.conv_pack(wd, scale, True, True), "scale": scale}

    return _cached(layer, (wt,), derive)


def fromrgb(layer, x):
    conv, act = layer[0], layer[1]
    return _FromRGB.apply(x, conv.weight, act.bias, conv.scale)


def convact(layer, x):
    return _ConvAct.apply(x, layer[0].weight, layer[1].bias, convact_plan(layer))


def resblock(block, x):
    return _ResBlock.apply(x, block.conv1[0].weight, block.conv1[1].bias, block.conv2[1].weight, block.conv2[2].bias,
                           block.skip[1].weight, resblock_plan(block))


def mbstd(x):
    stddev_group(x.shape[0])
    return _MbStd.apply(x)


# ---------------------------------------------------------------------------------------------- R1: the gradient penalty as one node
def _lrelu_mask(t, y, gain):
    """t * gain * (y > 0 ? 1 : 0.2) for a [B, C] pair (w2e_affine_act_bwd on [B,C,1,1]): the EqualLinear activation's backward and tangent."""
    b, c = y.shape
    return IR.affine_act_bwd(_c(t), y, _const(y.device, c, gain), _const(y.device, c, SLOPE), b, c, 1, 1).view(b, c)


# Every stride-1 conv of the penalty runs on the direct kernel.  r1 is quadratic in g and its bias gradients are what is left after
# the stddev term's group sum cancels, so the ~1e-5 rounding of the Winograd F(4x4,3x3) forms -- invisible in a first-order step
# held to 1e-3 -- moved r1 by 1.5e-5 and a bias gradient by 3.7e-3 from float64 at 32^2 (1.6e-7 and 4.4e-4 on the direct kernel).
_R1_FORM = 0


def _add(a, b):
    return b if a is None else (a if b is None else a + b)


class _R1(torch.autograd.Function):
    """r1 = mean_b |d sum(D(x)) / dx_b|^2 with D's parameters as the differentiable inputs (module docstring: the four passes).
    inputs: x, meta, then fromRGB (weight, bias), per ResBlock (w1, b1, w2, b2, ws), final_conv (weight, bias), final_linear
    (w0, b0, w1, b1) -- the order of Discriminator.parameters().  Returns (r1, logits); logits are not differentiable here."""

    @staticmethod
    def forward(ctx, x, meta, *params):
        nblk = len(meta["blocks"])
        wr, br = params[0], params[1]
        wfc, bfc, w0, b0, w1, b1 = params[2 + 5 * nblk:]
        needs = ctx.needs_input_grad[2:]
        train = any(needs)
        b = x.shape[0]
        dev = x.device
        # pass 1: the primal forward
        acts = [fromrgb_fwd(x, wr, br, meta["rgb_scale"])]
        kept = []
        for j, plan in enumerate(meta["blocks"]):
            q = params[2 + 5 * j:7 + 5 * j]
            out, t1, xb, t2, xs = _resblock_fwd(acts[-1], q[1], q[3], plan, q[2].shape[0], form=_R1_FORM)
            kept.append((t1, xb, t2, xs) if train else (t1, None, t2, None))
            acts.append(out)
        h = acts[-1]
        c4 = wfc.shape[0]
        pfc = meta["final_conv"]
        m = mbstd_fwd(h)
        yfc = IR.affine_act(IR.conv3x3(m, pfc["wf"], c4, h.shape[2], h.shape[3], bias=bfc, slope=_const(dev, c4, SLOPE), form=_R1_FORM),
                            _const(dev, c4, SQRT2))
        s0, s1 = meta["lin_scale"]
        l0m, l1m = meta["lin_lr_mul"]
        w0s, w1s = w0 * s0, w1 * s1
        l0 = K.fused_leaky_relu(torch.nn.functional.linear(yfc.view(b, -1), w0s), b0 * l0m)
        logits = torch.nn.functional.linear(l0, w1s, b1 * l1m)
        # pass 2: the reverse pass for g = d sum(logits) / dx
        gz0 = _lrelu_mask(w1s.expand(b, -1), l0, SQRT2)
        gzfc = IR.affine_act_bwd(_c((gz0 @ w0s).view(yfc.shape)), yfc, _const(dev, c4, SQRT2), _const(dev, c4, SLOPE), b, c4, h.shape[2],
                                 h.shape[3])
        gm = IR.conv3x3(gzfc, pfc["wb"], h.shape[1] + 1, h.shape[2], h.shape[3], form=_R1_FORM)
        cots = [None] * (nblk + 1)
        gzs = [None] * nblk
        cots[nblk] = mbstd_bwd(gm, h)
        for j in range(nblk - 1, -1, -1):
            t1, xb, t2, xs = kept[j]
            grads, gzs[j] = _resblock_bwd(meta["blocks"][j], None, t1, None, t2, None, cots[j + 1], (True,) + (False,) * 5, form=_R1_FORM)
            cots[j] = grads[0]
            if not train:
                cots[j + 1] = None
        g, _, _ = fromrgb_bwd(cots[0], acts[0], x, wr, meta["rgb_scale"], True, False, False)
        r1 = sumsq_rows(g.view(b, -1)).mean()
        if train:
            ctx.meta = meta
            ctx.nblk = nblk
            flat = [x, g, gm, yfc, gzfc, l0, gz0, wr, w0, w1] + acts + cots
            for j in range(nblk):
                flat += list(kept[j]) + list(gzs[j])
            ctx.save_for_backward(*flat)
        ctx.mark_non_differentiable(logits)
        return r1, logits

    @staticmethod
    @once_differentiable
    def backward(ctx, g_r1, _g_logits):
        meta, nblk = ctx.meta, ctx.nblk
        sv = ctx.saved_tensors
        x, g, gm, yfc, gzfc, l0, gz0, wr, w0, w1 = sv[:10]
        acts, cots = sv[10:11 + nblk], sv[11 + nblk:12 + 2 * nblk]
        per = [sv[12 + 2 * nblk + 6 * j:18 + 2 * nblk + 6 * j] for j in range(nblk)]  # (t1, xb, t2, xs, gz1, gz2)
        needs = ctx.needs_input_grad[2:]
        out = [None] * len(needs)
        b = x.shape[0]
        dev = x.device
        h = acts[-1]
        c4 = yfc.shape[1]
        # pass 3: the tangent forward along dx = (2 / B) * g, the weight gradients wgrad(gz_l, tangent) on the way.  Passes 3-4 are
        # linear in the incoming gradient; it multiplies the finished gradients, not dx: folded into dx, a factor that is no power of
        # two re-rounds every tangent, and the bias gradients (what is left after a cancellation) then miss 3 x the unit result by
        # 4.4e-6 (measured at 32^2); scaled at the end they are within one rounding of it
        xd = g * (2.0 / b)
        ad = fromrgb_jvp(xd, acts[0], wr, meta["rgb_scale"])
        if needs[0]:
            _, out[0], _ = fromrgb_bwd(cots[0], acts[0], xd, wr, meta["rgb_scale"], False, True, False)
        del xd
        for j, p in enumerate(meta["blocks"]):
            t1, xb, t2, xs, gz1, gz2 = per[j]
            nw1, _, nw2, _, nws = needs[2 + 5 * j:7 + 5 * j]
            c, hh, ww = t1.shape[1], t1.shape[2], t1.shape[3]
            n, oh, ow = t2.shape[1], t2.shape[2], t2.shape[3]
            if nw1:
                out[2 + 5 * j] = wgrad(WGRAD_SAME, gz1, ad, c, c, 9, p["s1"])
            t1d = IR.affine_act_bwd(IR.conv3x3(ad, p["w1f"], c, hh, ww, form=_R1_FORM), t1, None, _const(dev, c, SLOPE), b, c, hh, ww)
            xbd = blur(t1d)
            del t1d
            if nw2:
                out[4 + 5 * j] = wgrad(WGRAD_DOWN, gz2, xbd, n, c, 9, p["s2"])
            t2d = IR.affine_act_bwd(IR.conv3x3(xbd, p["w2f"], n, oh, ow, mode=K.MODE_DOWN, down_pad=0), t2, None, _const(dev, n, SLOPE),
                                    b, n, oh, ow)
            del xbd
            xsd = blur(ad)
            if nws:
                out[6 + 5 * j] = wgrad(WGRAD_DOWN_CENTRE, cots[j + 1], xsd, n, c, 1, p["ss"])
            ad = IR.conv3x3(xsd, p["wsf"], n, oh, ow, mode=K.MODE_DOWN, down_pad=0)
            del xsd
            call("w2e_shortcut_add_bwd", ptr(ad), ptr(t2d), b, n, oh, ow, 1, 0, stream_ptr())
            del t2d
        hd = ad
        k = 2 + 5 * nblk  # final_conv.weight, .bias, final_linear.0.weight, .bias, .1.weight, .bias
        tail = any(needs[k:]) or meta["debug"] is not None
        if tail:
            pfc = meta["final_conv"]
            md = mbstd_jvp(h, hd)
            if needs[k]:
                out[k] = wgrad(WGRAD_SAME, gzfc, md, c4, h.shape[1] + 1, 9, pfc["scale"])
            fd = IR.affine_act_bwd(IR.conv3x3(md, pfc["wf"], c4, h.shape[2], h.shape[3], form=_R1_FORM), yfc, _const(dev, c4, SQRT2),
                                   _const(dev, c4, SLOPE), b, c4, h.shape[2], h.shape[3]).view(b, -1)
            s0, s1 = meta["lin_scale"]
            if needs[k + 2]:
                out[k + 2] = (gz0.t() @ fd) * s0
            l0d = _lrelu_mask(fd @ (w0 * s0).t(), l0, SQRT2)
            if needs[k + 4]:
                out[k + 4] = l0d.sum(0, keepdim=True) * s1
            # the masks are piecewise constant and the linear layers carry no second-order term: these two biases get exact zeros, and
            # final_linear.1.bias does not reach the penalty at all (None)
            if needs[k + 1]:
                out[k + 1] = _const(dev, c4, 0.0).clone()
            if needs[k + 3]:
                out[k + 3] = _const(dev, l0.shape[1], 0.0).clone()
            if meta["debug"] is not None:  # the identity sum_b (tangent logits) = 2 * r1 * grad_out (tests)
                meta["debug"]["tangent_sum"] = (l0d @ (w1 * s1).t()).sum() * g_r1
                meta["debug"]["grad_out"] = g_r1
        # pass 4: the stddev layer's second-order term through the ordinary backward of everything below it
        if any(needs[:k]):
            mu = mbstd_hvp(gm, h, hd)
            for j in range(nblk - 1, -1, -1):
                t1, xb, t2, xs, _, _ = per[j]
                nd = needs[2 + 5 * j:7 + 5 * j]
                grads, _ = _resblock_bwd(meta["blocks"][j], acts[j], t1, xb, t2, xs, mu, (any(needs[:2 + 5 * j]),) + tuple(nd), form=_R1_FORM)
                for i in range(5):
                    out[2 + 5 * j + i] = _add(out[2 + 5 * j + i], grads[1 + i])
                mu = grads[0]
                if mu is None:
                    break
            if mu is not None and (needs[0] or needs[1]):
                _, dw, db = fromrgb_bwd(mu, acts[0], x, wr, meta["rgb_scale"], False, needs[0], needs[1])
                out[0] = _add(out[0], dw)
                out[1] = db
        return (None, None) + tuple(None if o is None else o * g_r1 for o in out)


def r1_penalty(d, real, return_logits=False, debug=None):
    """The R1 gradient penalty of a Discriminator `d` on `real` [B,3,S,S]: r1 = mean_b |d sum(d(real)) / d real_b|^2 (rosinality's
    d_r1_loss), as ONE autograd node whose differentiable inputs are d's parameters: `(r1_gamma / 2 * r1 * d_reg_every).backward()`
    leaves the penalty's gradient in every parameter that requires grad (final_linear.1.bias gets none: it does not reach the penalty).
    `real.requires_grad` is accepted (the usual training loop sets it) and ignored: no gradient flows to `real`, and the logits
    returned with return_logits=True carry no graph either (call d(real) for a differentiable D(real)).  With no trainable parameter
    the result has no grad_fn and only the forward and one reverse pass run.  The batch must satisfy stddev_group.
    debug: a dict that the backward fills with "tangent_sum" and "grad_out" (tests: sum_b of the tangent logits = 2 * r1 * grad_out)."""
    if d.stddev_group != 4 or d.stddev_feat != 1:
        raise NotImplementedError("the minibatch-stddev kernels implement stddev_group 4, stddev_feat 1 (model.py:686-687)")
    if real.ndim != 4 or real.shape[1] != 3:
        raise ValueError(f"r1_penalty: real must be [B,3,S,S], got {tuple(real.shape)}")
    stddev_group(real.shape[0])
    x = _c(real.detach())
    ptr(x)  # a CPU tensor is refused here, before any weight is packed
    rgb, blocks = d.convs[0], list(d.convs)[1:]
    params = [rgb[0].weight, rgb[1].bias]
    for blk in blocks:
        if blk._blur != (1, 3, 3, 1):
            raise NotImplementedError("ResBlock kernels exist for the [1, 3, 3, 1] blur (the Discriminator's default) only")
        params += [blk.conv1[0].weight, blk.conv1[1].bias, blk.conv2[1].weight, blk.conv2[2].bias, blk.skip[1].weight]
    fc, l0, l1 = d.final_conv, d.final_linear[0], d.final_linear[1]
    params += [fc[0].weight, fc[1].bias, l0.weight, l0.bias, l1.weight, l1.bias]
    meta = {"rgb_scale": rgb[0].scale, "blocks": [resblock_plan(blk) for blk in blocks], "final_conv": convact_plan(fc),
            "lin_scale": (l0.scale, l1.scale), "lin_lr_mul": (l0.lr_mul, l1.lr_mul), "debug": debug}
    r1, logits = _R1.apply(x, meta, *params)
    return (r1, logits) if return_logits else r1
