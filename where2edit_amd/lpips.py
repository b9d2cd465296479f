"""LPIPS (Zhang et al. 2018), the VGG16 variant, version 0.1 of the published `lpips` package, on the hand-written kernels:

    LPIPS(net="vgg")(in0, in1) -> [B,1,1,1]:  sum over five taps of  mean_p sum_c w_kc (u0_c - u1_c)^2,  u = f / (|f|_2 + 1e-10)

  * the ScalingLayer `(x - shift) / scale` is w2e_affine_act_fwd (a per-channel affine map on three channels; it comes before the
    zero padding of conv1_1, so it cannot be folded into that convolution's bias);
  * the thirteen 3x3 convolutions of VGG16 configuration D are w2e_conv3x3 with bias and ReLU in the epilogue (the Winograd forms where
    the library's plan picks them), the four 2x2 max-pools w2e_maxpool2x2_fwd / w2e_maxpool2x2_relu_bwd -- all of it vgg16.py,
    the trunk perceptual_loss.Vgg16 runs to relu4_3; conv5 is its fifth slice;
  * the head is new: w2e_lpips_head_fwd / w2e_lpips_head_bwd (include/w2e_lpips.h, csrc/lpips.hip), one call per tap.

Nothing of this was checked against the `lpips` package, torchvision or the published weight files: none of them is available where
this was written.  The arithmetic is restated from the paper and the published architecture and tested against a float64
restatement (tests/lpips_ref.py).  WITHOUT LOADED FILES THE NETWORK HOLDS SEEDED RANDOM WEIGHTS: torchvision's VGG initialisation
(kaiming_normal_, fan_out, relu; zero bias) and a non-negative uniform draw for the lin layers.  Its numbers are then comparable only
with each other -- they are no LPIPS of the literature -- the same way FeatureExtractorInceptionV3 and PerceptualLoss start out.

state_dict keys, after the `lpips` package's module tree so that its files load.  THESE NAMES ARE WRITTEN FROM MEMORY OF THE PUBLISHED
CODE and could not be checked against it:

    scaling_layer.shift, scaling_layer.scale                          buffers [1,3,1,1]
    net.slice1.{0,2}  net.slice2.{5,7}  net.slice3.{10,12,14}
    net.slice4.{17,19,21}  net.slice5.{24,26,28}   .weight / .bias    torchvision's vgg16().features indices
    lin{0..4}.model.1.weight                                          [1,C,1,1], C = 64, 128, 256, 512, 512 (model.0 is the Dropout
                                                                      of the package: identity in eval mode, absent here)

Files: `model_path` -- the package's weights/v0.1/vgg.pth (`lin{k}.model.1.weight`), the same under `lins.{k}.model.1.weight`, or a
whole-module state_dict (then its `net.slice*` tensors are loaded too); `vgg_weights` -- torchvision's vgg16 state_dict
(`features.{i}.*`; `classifier.*` is ignored) or this module's `net.slice{k}.{i}.*` / `slice{k}.{i}.*`.

A frozen critic, as Vgg16, IDLoss and the Inception extractor are: forward and INPUT gradients only, one autograd node, no host
synchronisation, no memset and no atomics in either direction, so forward + backward capture into a hipGraph.  There is no CPU path
and no stock-op fallback."""
import torch
from torch.autograd.function import once_differentiable

from . import irse_hip as IR
from . import vgg16 as V
from ._lib import CONSTS, call, ptr, stream_ptr
from .derived import derived

TAPS = (2, 7, 14, 21, 28)  # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: the conv each tap follows, the last of each of V.SLICES
CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
HEAD_PARTIALS = CONSTS["W2E_LPIPS_PARTIALS"]  # floats of the head's partials slab per image (include/w2e_lpips.h)
# The names this module had while it held its own copy of the network: the trunk's table and kernel calls.  Code written against them
# keeps working; nothing in the package uses them.
CONVS, POOLS, SLICES = V.CONVS, V.POOLS, V.SLICES
_conv_relu, _maxpool = V.conv_relu, V.maxpool


def conv_names():
    """`net.slice{k}.{i}` of the thirteen convolutions, in network order."""
    return [f"net.slice{V.slice_of(i)}.{i}" for i in V.CONVS]


def state_dict_keys():
    """Every key of LPIPS().state_dict(), in module order."""
    keys = ["scaling_layer.shift", "scaling_layer.scale"]
    keys += [f"{n}.{kind}" for n in conv_names() for kind in ("weight", "bias")]
    return keys + [f"lin{k}.model.1.weight" for k in range(5)]


def lin_state_dict(sd):
    """The five lin weights of an LPIPS checkpoint, keyed `lin{k}.model.1.weight`, from the package's weights file
    (`lin{k}.model.1.weight`), its ModuleList alias (`lins.{k}.model.1.weight`) or a whole-module state_dict.  Other keys are ignored; a
    missing or misshapen tensor raises with the names it looked for."""
    sd = V.unwrap(sd)
    out = {}
    for k, c in enumerate(CHANNELS):
        name = f"lin{k}.model.1.weight"
        out[name] = V.find(sd, "LPIPS lin weights", name, (name, f"lins.{k}.model.1.weight"), (1, c, 1, 1))
    return out


def vgg_state_dict(sd):
    """The 26 feature tensors of a VGG16 checkpoint, keyed `net.slice{k}.{i}.{weight,bias}`, from torchvision's layout
    (`features.{i}.*`), this module's (`net.slice{k}.{i}.*`) or the bare `slice{k}.{i}.*`.  Other keys are ignored; a missing or
    misshapen tensor raises with the names it looked for."""
    return V.state_dict(sd, 5, "net.", ("features.{i}", "net.{name}", "{name}"), "LPIPS VGG16 weights")


class ScalingLayer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT, dtype=torch.float32)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE, dtype=torch.float32)[None, :, None, None])


class _Vgg16Features(torch.nn.Module):
    """The package's `vgg16` wrapper: slice1 .. slice5 of torchvision's vgg16().features, the layers under their feature indices."""

    def __init__(self, generator):
        super().__init__()

        def init(conv):  # torchvision's VGG init (kaiming_normal_(mode="fan_out", nonlinearity="relu"), zero bias), from `generator`
            with torch.no_grad():
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=generator) * (2.0 / (conv.out_channels * 9)) ** 0.5)
                conv.bias.zero_()
        V.add_slices(self, 5, init)


class NetLinLayer(torch.nn.Module):
    """The package's 1x1 convolution on the squared difference (Dropout at model.0 there: eval-mode identity, absent here)."""

    def __init__(self, chn_in, generator):
        super().__init__()
        conv = torch.nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False)
        with torch.no_grad():  # seeded and non-negative, as the published weights are; mean 1 / chn_in
            conv.weight.copy_(torch.rand(conv.weight.shape, generator=generator) * (2.0 / chn_in))
        self.model = torch.nn.Sequential()
        self.model.add_module("1", conv)


class _Plan(V.Plan):
    """The trunk's packed convolutions, the ScalingLayer as y = a x + b, the five lin vectors."""

    def __init__(self, model):
        super().__init__(model.net, 5)
        shift = model.scaling_layer.shift.detach().double().reshape(3)
        scale = model.scaling_layer.scale.detach().double().reshape(3)
        self.a = (1.0 / scale).float().contiguous()
        self.b = (-shift / scale).float().contiguous()
        self.lin = [getattr(model, f"lin{k}").model._modules["1"].weight.detach().float().reshape(-1).contiguous() for k in range(5)]


# ---------------------------------------------------------------------------------------------- the head's kernel calls
def head_fwd(f0, f1, lin, out=None):
    """w2e_lpips_head_fwd: f0 [B,C,h,w], f1 [B or 1,C,h,w], lin [C] -> out [B]."""
    b, c = f0.shape[0], f0.shape[1]
    pixels = f0.shape[2] * f0.shape[3]
    out = torch.empty(b, device=f0.device, dtype=torch.float32) if out is None else out
    partials = torch.empty(b * HEAD_PARTIALS, device=f0.device, dtype=torch.float32)
    call("w2e_lpips_head_fwd", ptr(f0), ptr(f1), ptr(lin), b, f1.shape[0], c, pixels, ptr(partials), partials.numel(), ptr(out), stream_ptr())
    return out


def head_bwd(f0, f1, lin, gout, g0=None, g1=None, want_g1=False, accumulate=False, relu=True):
    """w2e_lpips_head_bwd: the gradients at f0 (and f1 with want_g1), written into g0 / g1 or fresh tensors; accumulate: added to what
    g0 / g1 hold; relu: the tap's ReLU mask folded in (after the addition).  Returns (g0, g1 or None)."""
    b, c = f0.shape[0], f0.shape[1]
    pixels = f0.shape[2] * f0.shape[3]
    if accumulate and (g0 is None or (want_g1 and g1 is None)):
        raise ValueError("head_bwd: accumulate needs the tensors to add to")
    g0 = torch.empty_like(f0) if g0 is None else g0
    if want_g1 and g1 is None:
        g1 = torch.empty_like(f1)
    call("w2e_lpips_head_bwd", ptr(f0), ptr(f1), ptr(lin), ptr(gout), b, f1.shape[0], c, pixels, ptr(g0), ptr(g1) if want_g1 else None,
         int(bool(accumulate)), int(bool(relu)), stream_ptr())
    return g0, (g1 if want_g1 else None)


# ---------------------------------------------------------------------------------------------- autograd
class _LPIPS(torch.autograd.Function):
    """ScalingLayer -> the five slices -> the five heads, fused: one merged forward over [in0; in1] and one backward over the rows
    that take a gradient (in0's, and in1's too when it requires grad).  Returns (distance [B], per-tap terms [5,B]).
    Saved: the five taps of every row (the head's adjoint at a gradient row needs the other side's features too; the first four are
    also the pool inputs the arg-max is recomputed from) and the eight ReLU outputs in between of the gradient rows.  The normalised
    features are not kept: the head's adjoint recomputes the norms."""

    @staticmethod
    def forward(ctx, x0, x1, plan, need_grad, grad1):
        x0, x1 = V.contig(x0), V.contig(x1)
        b0, b1 = x0.shape[0], x1.shape[0]
        rows = ((2 * b0 if grad1 else b0) if need_grad else 0)
        h = IR.affine_act(torch.cat([x0, x1]), plan.a, plan.b)
        taps, mids = [], []
        terms = torch.empty((5, b0), device=x0.device, dtype=torch.float32)
        for k in range(5):
            outs = V.slice_fwd(plan, k, h)
            h = outs[-1]
            if need_grad:
                mids += [o[:rows] for o in outs[:-1]]
            taps.append(h)
            head_fwd(h[:b0], h[b0:], plan.lin[k], out=terms[k])
        total = ((terms[0] + terms[1]) + (terms[2] + terms[3])) + terms[4]
        if need_grad:
            ctx.plan, ctx.b0, ctx.b1, ctx.grad1 = plan, b0, b1, grad1
            ctx.save_for_backward(*taps, *mids)
        ctx.mark_non_differentiable(terms)  # (the per-tap terms are reported, not differentiated: the gradient is the distance's)
        return total, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, go, _gterms):
        saved = ctx.saved_tensors
        taps, mids = list(saved[:5]), list(saved[5:])
        plan, b0, grad1 = ctx.plan, ctx.b0, ctx.grad1
        rows = 2 * b0 if grad1 else b0
        go = V.contig(go.reshape(-1).float())
        g = None  # the gradient at the current tap (post-ReLU), arriving from the slice behind it
        for k in range(4, -1, -1):
            t = taps[k]
            acc = g is not None
            if not acc:
                g = torch.empty((rows,) + tuple(t.shape[1:]), device=t.device, dtype=torch.float32)
            # + the head's own gradient, then the tap's ReLU mask: the gradient at the pre-activation of the slice's last conv
            head_bwd(t[:b0], t[b0:], plan.lin[k], go, g0=g[:b0], g1=g[b0:] if grad1 else None, want_g1=grad1, accumulate=acc, relu=True)
            n = len(V.SLICE_CONVS[k]) - 1  # the slice's ReLU outputs in between: the last n of what is left of mids
            g = V.slice_bwd(plan, k, g, mids[len(mids) - n:])
            del mids[len(mids) - n:]
            if k > 0:  # the pool's own adjoint: the previous tap's ReLU mask joins in its head call
                g = V.maxpool_bwd(g, taps[k - 1][:rows], relu=False)
        b, _, h, w = g.shape
        g = IR.affine_act_bwd(g, None, plan.a, None, b, 3, h, w)  # gx = a[c] * gy (no activation behind the ScalingLayer)
        return g[:b0], (g[b0:] if grad1 else None), None, None, None


# ---------------------------------------------------------------------------------------------- module
class LPIPS(torch.nn.Module):
    """`lpips.LPIPS(net="vgg", version="0.1")`: forward(in0, in1, retPerLayer=False, normalize=False) -> [B,1,1,1] fp32 (and, with
    retPerLayer, the list of the five [B,1,1,1] terms).  in0 / in1: [B,3,H,W] in [-1, 1] (normalize=True: in [0, 1], mapped by 2x - 1
    first), H, W >= 16 (the pools floor odd sizes).  in1 may have batch 1 against in0's B: it is broadcast and its features are
    computed once; a broadcast in1 that requires grad is refused.  Gradients reach in0, and in1 when it requires grad, through the
    distance; the per-layer terms are reported values and carry no gradient of their own.
    Only this configuration exists: another `net` or `version`, spatial=True or lpips=False raise ValueError.
    model_path / vgg_weights: the files described at the top of this module; without them the weights are a seeded (`seed`) random
    initialisation whose distances are comparable only with each other.  The module stays where it is built: move it with .to()."""

    def __init__(self, net="vgg", version="0.1", spatial=False, lpips=True, model_path=None, vgg_weights=None, seed=0):
        super().__init__()
        if net != "vgg":
            raise ValueError(f"LPIPS: net={net!r}: only net='vgg' (VGG16) is built; the AlexNet and SqueezeNet variants are not")
        if version != "0.1":
            raise ValueError(f"LPIPS: version={version!r}: only version='0.1' is built")
        if spatial:
            raise ValueError("LPIPS: spatial=True (the per-pixel distance map) is not built; the result is the spatial mean")
        if not lpips:
            raise ValueError("LPIPS: lpips=False (unweighted features, no lin layers) is not built")
        self.pnet_type, self.version, self.spatial, self.lpips = net, version, False, True
        self.chns = list(CHANNELS)
        self.L = len(self.chns)
        g = torch.Generator().manual_seed(seed)
        self.scaling_layer = ScalingLayer()
        self.net = _Vgg16Features(g)
        for k, c in enumerate(self.chns):
            self.add_module(f"lin{k}", NetLinLayer(c, g))
        if model_path is not None:
            sd = V.unwrap(torch.load(model_path, map_location="cpu"))
            self.load_state_dict(lin_state_dict(sd), strict=False)
            if any(k.startswith("net.slice") for k in sd):
                self.load_state_dict(vgg_state_dict(sd), strict=False)
        if vgg_weights is not None:
            self.load_state_dict(vgg_state_dict(torch.load(vgg_weights, map_location="cpu")), strict=False)
        for p in self.parameters():
            p.requires_grad = False
        self.eval()

    def plan(self):
        """The packed parameters (cached: derived.py)."""
        return derived(self, "_plan", list(self.parameters()) + list(self.buffers()), lambda: _Plan(self))

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        V.refuse_trainable(self, "LPIPS")
        for name, x in (("in0", in0), ("in1", in1)):
            if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] < 16 or x.shape[3] < 16:
                raise ValueError(f"LPIPS: {name} must be [B,3,H,W] with H, W >= 16, got "
                                 f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
        b0 = in0.shape[0]
        if tuple(in1.shape[1:]) != tuple(in0.shape[1:]) or b0 < 1:
            raise ValueError(f"LPIPS: in1 {tuple(in1.shape)} must have in0's shape {tuple(in0.shape)}, or batch 1 of it")
        need_grad, grad1 = V.pair_grads("LPIPS", in0, in1, "in0", "in1")
        if normalize:
            in0, in1 = 2 * in0 - 1, 2 * in1 - 1
        in1 = in1 if grad1 else in1.detach()
        total, terms = _LPIPS.apply(in0.float(), in1.float(), self.plan(), need_grad, grad1)
        total = total.view(b0, 1, 1, 1)
        if retPerLayer:
            return total, [terms[k].view(b0, 1, 1, 1) for k in range(5)]
        return total
