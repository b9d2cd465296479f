"""VGG16 configuration D (torchvision.models.vgg16().features) on the hand-written kernels, written once: the trunk under
perceptual_loss.py (its first four slices, to relu4_3) and lpips.py (all five).  The layer table, the `slice{k}` module tree, the
checkpoint key mapper, the packed plan, the raw kernel calls, the forward and backward walk over one slice, and what the two
two-image losses decide about their target before they launch anything.  Nothing here knows a loss, a head or a preprocessing.

Every 3x3 convolution is w2e_conv3x3 (mode SAME; bias and a zero-slope PReLU = ReLU in its epilogue; the Winograd forms where the
library's plan picks them); input gradients go through the transposed, flipped pack; the ReLU between two convolutions is undone by
w2e_affine_act_bwd with a zero slope; 2x2 max-pooling is w2e_maxpool2x2_fwd, and its adjoint w2e_maxpool2x2_relu_bwd recomputes the
arg-max from the saved pool input (no index tensor) and can fold the ReLU in front of the pool in.  A frozen critic: forward and
INPUT gradients only, no stock-op fallback, no host synchronisation."""
import torch

from . import functional as K
from . import irse_hip as IR
from ._lib import call, ptr, stream_ptr

# index -> (in, out) of each conv; ReLU(inplace=True) after every conv, MaxPool2d(2, 2) at POOLS.  A slice ends at a tap: relu1_2,
# relu2_2, relu3_3, relu4_3 (criteria/perceptual_loss.py:33-40), relu5_3 (the `lpips` package).
CONVS = {0: (3, 64), 2: (64, 64), 5: (64, 128), 7: (128, 128), 10: (128, 256), 12: (256, 256), 14: (256, 256), 17: (256, 512),
         19: (512, 512), 21: (512, 512), 24: (512, 512), 26: (512, 512), 28: (512, 512)}
POOLS = (4, 9, 16, 23)
SLICES = (range(0, 4), range(4, 9), range(9, 16), range(16, 23), range(23, 30))
SLICE_CONVS = tuple(tuple(i for i in r if i in CONVS) for r in SLICES)  # the conv indices of each slice, in order


def slice_of(i):
    return next(k for k, r in enumerate(SLICES) if i in r) + 1


def convs(n):
    """CONVS restricted to the first n slices."""
    return {i: c for i, c in CONVS.items() if i < SLICES[n - 1].stop}


# ---------------------------------------------------------------------------------------------- module tree, checkpoints, plan
def add_slices(module, n, init):
    """Adds `slice1 .. slice{n}` to `module`: Sequentials with the layers under their feature indices.  `init(conv)` fills each
    convolution as it is built, in index order (the two users draw their seeded weights differently)."""
    for k, r in enumerate(SLICES[:n]):
        seq = torch.nn.Sequential()
        for i in r:
            if i in CONVS:
                layer = torch.nn.Conv2d(*CONVS[i], kernel_size=3, padding=1)
                init(layer)
            elif i in POOLS:
                layer = torch.nn.MaxPool2d(kernel_size=2, stride=2)
            else:
                layer = torch.nn.ReLU(inplace=True)
            seq.add_module(str(i), layer)
        module.add_module(f"slice{k + 1}", seq)


def unwrap(sd):
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


def find(sd, what, name, candidates, shape):
    """The tensor of `sd` under the first of `candidates` it has, as detached fp32; raises with every name it looked for."""
    for key in candidates:
        if key in sd:
            break
    else:
        raise KeyError(f"{what}: no tensor for {name} (looked for {', '.join(candidates)})")
    t = sd[key]
    if tuple(t.shape) != shape:
        raise RuntimeError(f"{what}: {key} has shape {tuple(t.shape)}, expected {shape}")
    return t.detach().float()


def state_dict(sd, n, prefix, spellings, what):
    """The feature tensors of the first n slices of a VGG16 checkpoint, keyed `{prefix}slice{k}.{i}.{weight,bias}`.  `spellings`:
    the layouts accepted, tried in order, as formats over `i` and `name` = `slice{k}.{i}`.  Other keys are ignored (`classifier.*`,
    later blocks); a missing or misshapen tensor raises."""
    sd = unwrap(sd)
    out = {}
    for i, (cin, cout) in convs(n).items():
        name = f"slice{slice_of(i)}.{i}"
        for kind, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            own = f"{prefix}{name}.{kind}"
            out[own] = find(sd, what, own, [f"{s.format(i=i, name=name)}.{kind}" for s in spellings], shape)
    return out


class Plan:
    """Packed, frozen parameters of the convolutions of `net.slice1 .. net.slice{n}`: forward pack, transposed-flipped pack (input
    gradient), bias."""

    def __init__(self, net, n):
        self.fwd, self.bwd, self.bias, self.cout = {}, {}, {}, {}
        with torch.no_grad():
            for i in convs(n):
                conv = getattr(getattr(net, f"slice{slice_of(i)}"), str(i))
                w = conv.weight.detach().float()
                self.fwd[i] = K.conv_pack(w, 1.0, transpose=False, flip=False)
                self.bwd[i] = K.conv_pack(w, 1.0, transpose=True, flip=True)
                self.bias[i] = conv.bias.detach().float().contiguous()
                self.cout[i] = w.shape[0]
            dev = self.bias[0].device
            self.zero = {c: torch.zeros(c, device=dev, dtype=torch.float32) for c in (64, 128, 256, 512)}  # ReLU = PReLU(slope 0)


def refuse_trainable(module, what):
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        raise RuntimeError(
            f"where2edit_amd: a weight of {what} requires grad.  The HIP kernels treat {what} as a frozen critic -- as the perceptual "
            "loss does (criteria/perceptual_loss.py builds Vgg16(requires_grad=False)) -- and produce input gradients only; there is "
            "no stock-op fallback.  Call .requires_grad_(False) on it.")


def pair_grads(who, image, target, image_noun, target_noun):
    """(need_grad, grad2) of a loss of an image batch against a target batch that is as large or 1 (then broadcast): whether
    anything takes a gradient, and whether the target does.  A broadcast target that requires grad is refused."""
    b1, b2 = image.shape[0], target.shape[0]
    if b2 != b1 and b2 != 1:
        raise ValueError(f"{who}: {target_noun} batch {b2} is neither the {image_noun} batch {b1} nor 1")
    grad_on = torch.is_grad_enabled()
    grad2 = grad_on and target.requires_grad
    if grad2 and b2 != b1:
        raise RuntimeError(f"{who}: a broadcast (batch-1) {target_noun} that requires grad is not supported; detach it or repeat it "
                           f"to the {image_noun} batch")
    return grad_on and (image.requires_grad or grad2), grad2


# ---------------------------------------------------------------------------------------------- raw kernel calls
def conv_relu(plan, i, x):
    _, _, h, w = x.shape
    return IR.conv3x3(x, plan.fwd[i], plan.cout[i], h, w, bias=plan.bias[i], slope=plan.zero[plan.cout[i]])


def conv_grad(plan, i, g, in_scale=None):
    _, _, h, w = g.shape
    return IR.conv3x3(g, plan.bwd[i], CONVS[i][0], h, w, in_scale=in_scale)


def relu_bwd(plan, g, y):
    b, c, h, w = g.shape
    return IR.affine_act_bwd(g, y, None, plan.zero[c], b, c, h, w)


def maxpool(x):
    b, c, h, w = x.shape
    y = torch.empty((b, c, h // 2, w // 2), device=x.device, dtype=torch.float32)
    call("w2e_maxpool2x2_fwd", ptr(x), ptr(y), b * c, h, w, stream_ptr())
    return y


def maxpool_bwd(g, x, relu):
    b, c, h, w = x.shape
    gx = torch.empty((b, c, h, w), device=g.device, dtype=torch.float32)
    call("w2e_maxpool2x2_relu_bwd", ptr(g), ptr(x), ptr(gx), b * c, h, w, int(relu), stream_ptr())
    return gx


def contig(t):
    return t if t.is_contiguous() else t.contiguous()


# ---------------------------------------------------------------------------------------------- the walks over one slice
def slice_fwd(plan, k, x):
    """SLICES[k] on x: the leading pool if it has one, then conv + ReLU for each of its convolutions.  Returns the post-ReLU
    outputs in order; the last is the slice's result."""
    h = maxpool(x) if SLICES[k].start in POOLS else x
    outs = []
    for i in SLICE_CONVS[k]:
        h = conv_relu(plan, i, h)
        outs.append(h)
    return outs


def slice_bwd(plan, k, g, inner, in_scale=None):
    """The input gradient of SLICES[k]'s convolutions.  g: the gradient at the PRE-activation of its last convolution (the caller
    has applied that ReLU's mask its own way; `in_scale` [B,K] scales g inside that convolution's call); inner: the post-ReLU
    outputs in front of each later convolution, in forward order.  Returns the gradient at the first convolution's input: the leading
    pool's adjoint is the caller's too, because it decides which ReLU to fold into it."""
    ids = SLICE_CONVS[k]
    g = conv_grad(plan, ids[-1], g, in_scale)
    for j in range(len(ids) - 2, -1, -1):
        g = conv_grad(plan, ids[j], relu_bwd(plan, g, inner[j]))
    return g
