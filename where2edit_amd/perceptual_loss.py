"""criteria/perceptual_loss.py surface: `PerceptualLoss(opts)(image1, image2) -> MSE(relu2_2(pre(image1)), relu2_2(pre(image2)))`
with `pre = avg_pool(upsample(.))` and the `.model` (a `Vgg16`), `.upsample`, `.avg_pool` attributes of the reference, on the
hand-written kernels of include/w2e_irse.h (the network itself is vgg16.py, the trunk shared with lpips.py):

  * every 3x3 convolution is w2e_conv3x3 (mode SAME, bias and a zero-slope PReLU = ReLU in its epilogue; the Winograd forms
    where irse_hip._wino_form picks them, as for IR-SE50); input gradients through the transposed, flipped pack;
  * 2x2 max-pooling is w2e_maxpool2x2_fwd; its backward, w2e_maxpool2x2_relu_bwd, recomputes the arg-max from the saved pool
    input (no index tensor) and folds relu1_2's backward in;
  * the MSE head is w2e_mse_relu_fwd: a bit-reproducible two-pass reduction that also writes the gradient with relu2_2's mask
    folded in, so the backward keeps that and not the features;
  * the 7x up-sample + average pool is the closed form of CLIPLoss (functional.clip_preprocess).

`PerceptualLoss.forward` computes slices 1-2 only: the loss reads relu2_2, so slices 3-4 (about 18.5 GFLOP per image in the
reference) cannot change its value or gradient.  `Vgg16.forward` computes all four slices, with input gradients.

Weights: `opts.vgg_weights` (optional), in torchvision's layout (`features.N.*`, the vgg16-397923af.pth state_dict; `classifier.*`
is ignored) or this module's (`slice*.N.*`, with or without the `model.` prefix).  Without it the network keeps torchvision's
published initialisation (kaiming_normal_, fan_out, relu; zero bias) -- random weights, for synthetic benchmarking, the same way
CLIPLoss falls back to a random-init ViT: there is no network to fetch the pretrained file the reference downloads.

The network is a frozen critic: forward and INPUT gradients only.  A weight that requires grad is refused (no weight-gradient
kernels, no stock-op fallback).  No host synchronisation in forward or backward."""
from collections import namedtuple

import torch
from torch.autograd.function import once_differentiable

from . import irse_hip as IR
from . import vgg16 as V
from ._lib import call, ptr, stream_ptr
from .derived import derived

VggOutputs = namedtuple("VggOutputs", ["relu1_2", "relu2_2", "relu3_3", "relu4_3"])

# The names this module had while it held the network itself: the trunk's table restricted to Vgg16's four slices, and the kernel calls.
# Code written against them keeps working; nothing in the package uses them.
CONVS, POOLS, SLICES = V.convs(4), V.POOLS[:3], V.SLICES[:4]
_conv_relu, _maxpool, _maxpool_bwd = V.conv_relu, V.maxpool, V.maxpool_bwd


def feature_state_dict(sd):
    """The 20 feature tensors of a VGG16 checkpoint, keyed `slice{k}.{i}.{weight,bias}`, from either torchvision's layout
    (`features.{i}.*`) or this module's (`slice{k}.{i}.*`, optionally under `model.`).  Other keys are ignored (`classifier.*`,
    torchvision's conv5 block); a missing or misshapen feature tensor raises."""
    return V.state_dict(sd, 4, "", ("features.{i}", "{name}", "model.{name}"), "VGG16 weights")


# ---------------------------------------------------------------------------------------------- autograd
class _Slice(torch.autograd.Function):
    """One slice of Vgg16: [MaxPool2d(2,2)] then conv + ReLU for each of its convolutions (perceptual_loss.py:33-40)."""

    @staticmethod
    def forward(ctx, x, plan, k):
        x = V.contig(x)
        outs = V.slice_fwd(plan, k, x)
        ctx.plan, ctx.k, ctx.pooled = plan, k, V.SLICES[k].start in V.POOLS
        ctx.save_for_backward(*(([x] if ctx.pooled else []) + outs))
        return outs[-1]

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        saved = ctx.saved_tensors
        x, outs = (saved[0], saved[1:]) if ctx.pooled else (None, saved)
        g = V.relu_bwd(ctx.plan, V.contig(gy), outs[-1])  # the slice's last ReLU
        g = V.slice_bwd(ctx.plan, ctx.k, g, outs[:-1])
        if ctx.pooled:  # the gradient at the slice's input: the pool's own adjoint, no ReLU folded (the previous slice applies its own)
            g = V.maxpool_bwd(g, x, relu=False)
        return g, None, None


class _PerceptualMSE(torch.autograd.Function):
    """preprocess -> slice1 -> slice2 -> MSE head, fused: one merged forward over [image1; image2] and one backward over the rows
    that take a gradient (image1's, and image2's too when it requires grad).  `pre`: apply the closed-form 7x up-sample + average
    pool (w2e_clip_preproc) here; otherwise the inputs are already preprocessed.  Saved: relu1_1, relu1_2, relu2_1 of the gradient
    rows and the head's gradient (relu2_2's mask folded in)."""

    @staticmethod
    def forward(ctx, x1, x2, plan, pre, need_grad, grad2):
        x1, x2 = V.contig(x1), V.contig(x2)
        b1, b2 = x1.shape[0], x2.shape[0]
        if pre:
            size = x1.shape[-1]
            buf = torch.empty((b1 + b2, 3, 224, 224), device=x1.device, dtype=torch.float32)
            st = stream_ptr()
            call("w2e_clip_preproc_fwd", ptr(x1), ptr(buf[:b1]), b1 * 3, size, st)
            call("w2e_clip_preproc_fwd", ptr(x2), ptr(buf[b1:]), b2 * 3, size, st)
        else:
            buf = torch.cat([x1, x2])
        r11, r12 = V.slice_fwd(plan, 0, buf)
        r21, r22 = V.slice_fwd(plan, 1, r12)
        per = r22[0].numel()
        rows = (2 * b1 if grad2 else b1) if need_grad else 0
        gpre = torch.empty((rows,) + tuple(r22.shape[1:]), device=x1.device, dtype=torch.float32) if need_grad else None
        partials = torch.empty(IR.MSE_PARTIALS, device=x1.device, dtype=torch.float32)
        loss = torch.empty((), device=x1.device, dtype=torch.float32)
        call("w2e_mse_relu_fwd", ptr(r22[:b1]), ptr(r22[b1:]), b1, b2, per, ptr(gpre[:b1]) if need_grad else None,
             ptr(gpre[b1:]) if grad2 else None, ptr(partials), IR.MSE_PARTIALS, ptr(loss), stream_ptr())
        if need_grad:
            ctx.plan, ctx.pre, ctx.b1, ctx.grad2 = plan, pre, b1, grad2
            ctx.shapes = (x1.shape, x2.shape)
            ctx.save_for_backward(r11[:rows], r12[:rows], r21[:rows], gpre)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        r11, r12, r21, gpre = ctx.saved_tensors
        plan, b1 = ctx.plan, ctx.b1
        rows = gpre.shape[0]
        scale = go.reshape(1, 1).expand(rows, 128).contiguous()  # grad_output, on the device: conv2_2's input scale
        g = V.slice_bwd(plan, 1, gpre, [r21], in_scale=scale)
        g = V.maxpool_bwd(g, r12, relu=True)  # pool1 + relu1_2
        g = V.slice_bwd(plan, 0, g, [r11])
        if not ctx.pre:
            return g[:b1], (g[b1:] if ctx.grad2 else None), None, None, None, None
        st = stream_ptr()
        s1, s2 = ctx.shapes
        g1 = torch.empty(s1, device=g.device, dtype=torch.float32)
        call("w2e_clip_preproc_bwd", ptr(g[:b1]), ptr(g1), s1[0] * 3, s1[-1], st)
        g2 = None
        if ctx.grad2:
            g2 = torch.empty(s2, device=g.device, dtype=torch.float32)
            call("w2e_clip_preproc_bwd", ptr(g[b1:]), ptr(g2), s2[0] * 3, s2[-1], st)
        return g1, g2, None, None, None, None


# ---------------------------------------------------------------------------------------------- modules
class Vgg16(torch.nn.Module):
    """criteria/perceptual_loss.py:24-53 with the reference's module tree (state_dict keys slice1.0.weight ... slice4.21.bias) and
    output namedtuple.  forward runs on the HIP kernels for any H, W >= 16 (max-pooling floors odd sizes like MaxPool2d(2, 2))."""

    def __init__(self, requires_grad=False):
        super().__init__()
        def init(conv):  # torchvision's VGG init, from the global RNG
            torch.nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
            torch.nn.init.constant_(conv.bias, 0)
        V.add_slices(self, 4, init)
        if not requires_grad:
            for param in self.parameters():
                param.requires_grad = False

    def plan(self):
        """The packed parameters (cached: derived.py)."""
        return derived(self, "_plan", list(self.parameters()), lambda: V.Plan(self, 4))

    def forward(self, X):
        V.refuse_trainable(self, "VGG16")
        if X.dim() != 4 or X.shape[1] != 3 or X.shape[2] < 16 or X.shape[3] < 16:
            raise ValueError(f"Vgg16: expected [B,3,H,W] with H, W >= 16, got {tuple(X.shape)}")
        plan = self.plan()
        outs = []
        h = X
        for k in range(4):
            h = _Slice.apply(h, plan, k)
            outs.append(h)
        return VggOutputs(*outs)


def normalize_batch(batch):
    """The reference's normalize_batch (perceptual_loss.py:56-65) is the identity: its ImageNet normalisation is commented out, so
    the [-1, 1] image goes straight into conv1_1.  Kept as the identity."""
    return batch


class PerceptualLoss(torch.nn.Module):
    """criteria/perceptual_loss.py:7-21: `forward(image1, image2)` = nn.MSELoss()(relu2_2(pre(image1)), relu2_2(pre(image2))),
    pre = avg_pool(upsample(.)) -- mean over every element.

    image2 may have batch 1 against image1's batch B: it is then broadcast (its features are computed once), and the value equals
    that of the repeated target -- what MSELoss gives under broadcasting, without its warning.  When image2 does not require grad it
    carries no autograd state; when it does, its gradient flows for equal batches (a broadcast target that requires grad is refused).
    Images of `opts.stylegan_size` take the closed-form preprocessing; other sizes run the literal Upsample -> AvgPool chain on stock
    ops, with a one-time warning (as CLIPLoss.preprocess).  The module stays where it is built: move it with .to(device)."""

    def __init__(self, opts, model=None):
        super().__init__()
        if model is None:
            model = Vgg16(requires_grad=False)
            path = getattr(opts, "vgg_weights", None)
            if path is not None:
                model.load_state_dict(feature_state_dict(torch.load(path, map_location="cpu")), strict=True)
        self.model = model
        self.upsample = torch.nn.Upsample(scale_factor=7)
        self.avg_pool = torch.nn.AvgPool2d(kernel_size=opts.stylegan_size // 32)
        self.stylegan_size = opts.stylegan_size

    def _closed_form(self, image):
        return image.dim() == 4 and image.shape[-1] == self.stylegan_size and image.shape[-2] == self.stylegan_size

    def _literal(self, image):
        if not getattr(self, "_warned_literal", False):
            import warnings
            warnings.warn(f"PerceptualLoss: image {tuple(image.shape[-2:])} is not stylegan_size {self.stylegan_size}: running the literal "
                          "Upsample(7) -> AvgPool chain on stock ops (it materialises the 49x image)")
            self._warned_literal = True
        return self.avg_pool(self.upsample(image))

    def forward(self, image1, image2):
        V.refuse_trainable(self.model, "VGG16")
        need_grad, grad2 = V.pair_grads("PerceptualLoss", image1, image2, "image", "target")
        plan = self.model.plan()
        if self._closed_form(image1) and self._closed_form(image2):
            x1, x2, pre = image1, image2, True
        else:
            x1 = self._literal(image1)
            with torch.set_grad_enabled(grad2):
                x2 = self._literal(image2)
            pre = False
        x2 = x2 if grad2 else x2.detach()
        return _PerceptualMSE.apply(x1, x2, plan, pre, need_grad, grad2)
