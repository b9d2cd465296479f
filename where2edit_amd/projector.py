"""StyleGAN2's projector (Karras et al. 2020, Appendix D; rosinality's projector.py): optimise w (or W+) and the per-layer noise maps
of a frozen generator so that G(w, noises) matches a target image under LPIPS, optionally plus MSE, with the multi-scale noise
regulariser.  The second way into the latent space beside the e4e encoder (demo_pipeline.invert_and_edit): slower, tighter.

The generator pass, LPIPS (lpips.py) and Adam (adam.py) are the package's own; the projector's arithmetic around them is
csrc/projector.hip (include/w2e_projector.h):

    noise_regularize(noises)      the regulariser and its gradient through every pyramid level, the whole list in ~20 launches
    noise_normalize_(noises)      n <- (n - mean) / std in place, the whole list in two launches
    loss_front(img, target, f)    box down-sampling to the LPIPS resolution and the MSE term; the adjoint writes the image gradient

and the noise-map gradient of the fused StyledConv (functional._StyledConv, w2e_noise_grad).  GPU only: there is no CPU path and no
stock-op fallback.  The loop is NOT graph-captured: the learning rate and the latent-noise strength change every step (they are host
scalars of the Adam launch and of latent_noise); capture is left to a later change."""
import collections
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import CONSTS, call, ptr, stream_ptr
from .run_attention import get_lr

SLOTS = CONSTS["W2E_PROJ_SLOTS"]


def _require_gpu(what, *tensors):
    for t in tensors:
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"where2edit_amd.projector: {what} runs on the GPU only (got "
                               f"{'a CPU tensor' if torch.is_tensor(t) else type(t).__name__}); there is no CPU path")


def _maps(noises, what):
    """The list as contiguous fp32 GPU tensors [B,1,s,s] on one device, with the ABI's host arrays (pointers, batch, size)."""
    noises = list(noises)
    _require_gpu(what, *noises)
    for n in noises:
        if n.dim() != 4 or n.shape[1] != 1 or n.shape[2] != n.shape[3] or n.dtype != torch.float32:
            raise ValueError(f"{what}: every map must be fp32 [B,1,s,s], got {tuple(n.shape)} {n.dtype}")
    return noises


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[ptr(t).value for t in tensors])


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


# ---------------------------------------------------------------------------------------------- noise regulariser
class _NoiseRegularize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *noises):
        maps = [n.contiguous() for n in noises]
        count = len(maps)
        batch, size = _ints([m.shape[0] for m in maps]), _ints([m.shape[2] for m in maps])
        floats = ctypes.c_int64(0)
        call("w2e_noise_reg_workspace", count, batch, size, ctypes.byref(floats))
        dev = maps[0].device
        with torch.cuda.device(dev):
            ws = torch.empty(max(floats.value, 2), device=dev, dtype=torch.float32)
            loss = torch.empty(1, device=dev, dtype=torch.float32)
            call("w2e_noise_reg_fwd", count, _pointers(maps), batch, size, ptr(ws), ws.numel(), ptr(loss), stream_ptr())
        ctx.save_for_backward(*maps)
        ctx.ws, ctx.dims = ws, (batch, size)
        return loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        maps = list(ctx.saved_tensors)
        batch, size = ctx.dims
        grads = [torch.empty_like(m) for m in maps]
        gout = gout.reshape(1).float().contiguous()
        with torch.cuda.device(maps[0].device):
            call("w2e_noise_reg_bwd", len(maps), _pointers(maps), batch, size, ptr(ctx.ws), ctx.ws.numel(), ptr(gout), _pointers(grads), 0,
                 stream_ptr())
        return tuple(grads)


def noise_regularize(noises):
    """projector.py's noise_regularize: sum over the maps [B,1,s,s] (s a power of two) and over their pyramid levels (2x2 box means
    while s > 8) of mean(n * roll(n, 1, 3))^2 + mean(n * roll(n, 1, 2))^2.  A 0-dim tensor; differentiable in every map."""
    noises = _maps(noises, "noise_regularize")
    if not noises:
        raise ValueError("noise_regularize: an empty list")
    return _NoiseRegularize.apply(*noises)


def noise_normalize_(noises):
    """projector.py's noise_normalize_: every map <- (map - mean) / std (unbiased) in place, outside autograd."""
    noises = _maps(noises, "noise_normalize_")
    if not noises:
        return noises
    for n in noises:
        if not n.is_contiguous():
            raise ValueError("noise_normalize_: the maps are rewritten in place and must be contiguous")
    dev = noises[0].device
    with torch.no_grad(), torch.cuda.device(dev):
        ws = torch.empty(len(noises) * SLOTS * 4, device=dev, dtype=torch.float32)
        numel = (ctypes.c_int64 * len(noises))(*[n.numel() for n in noises])
        call("w2e_noise_normalize", len(noises), _pointers(noises), numel, ptr(ws), ws.numel(), stream_ptr())
        torch.autograd.graph.increment_version(noises)  # written through raw pointers: autograd and the caches must see it
    return noises


# ---------------------------------------------------------------------------------------------- loss front
class _LossFront(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, target, f):
        img, target = img.contiguous(), target.contiguous()
        b, c, h, w = img.shape
        small = torch.empty((b, c, h // f, w // f), device=img.device, dtype=torch.float32)
        blocks = _lib.load().w2e_proj_front_blocks(small.numel())
        partials = torch.empty(blocks, device=img.device, dtype=torch.float64)
        with torch.cuda.device(img.device):
            call("w2e_proj_front_fwd", ptr(img), ptr(target), b, c, h, w, f, ptr(small), ctypes.c_void_p(partials.data_ptr()), stream_ptr())
        mse = (partials.sum() / small.numel()).float()
        ctx.save_for_backward(small, target)
        ctx.geom = (b, c, h, w, f)
        ctx.set_materialize_grads(False)
        return small, mse

    @staticmethod
    @once_differentiable
    def backward(ctx, g_small, g_mse):
        small, target = ctx.saved_tensors
        b, c, h, w, f = ctx.geom
        if g_small is None and g_mse is None:
            return None, None, None
        g_img = torch.empty((b, c, h, w), device=small.device, dtype=torch.float32)
        g_small = g_small.float().contiguous() if g_small is not None else None
        g_mse = g_mse.reshape(1).float().contiguous() if g_mse is not None else None
        with torch.cuda.device(small.device):
            call("w2e_proj_front_bwd", ptr(g_small), ptr(small), ptr(target), ptr(g_mse), 2.0 / small.numel(), b, c, h, w, f, ptr(g_img),
                 stream_ptr())
        return g_img, None, None


def loss_front(img, target, f=None):
    """(small, mse): the f x f box mean of img [B,C,H,W] (projector.py's reshape(...).mean([3, 5]); f = H // target's height by default,
    f = 1 a pass-through) and F.mse_loss(small, target).  Differentiable in img through both; target takes no gradient."""
    _require_gpu("loss_front", img, target)
    if img.dim() != 4 or target.dim() != 4 or img.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("loss_front: img and target must be fp32 [B,C,H,W]")
    f = img.shape[2] // target.shape[2] if f is None else int(f)
    if f < 1 or img.shape[2] % f or img.shape[3] % f or tuple(target.shape) != (img.shape[0], img.shape[1], img.shape[2] // f, img.shape[3] // f):
        raise ValueError(f"loss_front: target {tuple(target.shape)} is not img {tuple(img.shape)} down-sampled by f = {f}")
    return _LossFront.apply(img, target.detach(), f)


# ---------------------------------------------------------------------------------------------- the latent side ([B,512]-sized: torch ops)
def _randn(shape, device, generator):
    if generator is None:
        return torch.randn(shape, device=device)
    if generator.device.type == torch.device(device).type:
        return torch.randn(shape, device=device, generator=generator)
    return torch.randn(shape, generator=generator).to(device)  # a CPU generator: the same draws wherever the loop runs


def latent_noise(latent, strength, generator=None):
    """projector.py's latent_noise: latent + randn_like(latent) * strength."""
    return latent + _randn(latent.shape, latent.device, generator) * strength


def latent_statistics(g_ema, n=10000, generator=None):
    """(latent_mean [1,style_dim], latent_std 0-dim) of n mapped samples: latent_std = sqrt(sum((w - mean)^2) / n), as projector.py."""
    device = g_ema.input.input.device
    with torch.no_grad():
        w = g_ema.style(_randn((n, g_ema.style_dim), device, generator))
        mean = w.mean(0)
        std = ((w - mean).pow(2).sum() / n) ** 0.5
    return mean[None], std


Projection = collections.namedtuple("Projection", "latent noises img loss mse")
Projection.__doc__ = """What `project` returns: the latent ([B,512], or [B,n_latent,512] for W+), the list of noise maps, the image of the final
latent and noises [B,3,size,size], and the per-step histories of the total loss and of the MSE to the target ([steps] tensors)."""

_noise_regularize = noise_regularize


def project(g_ema, target, *, steps=1000, lr=0.1, lr_rampup=0.05, lr_rampdown=0.25, noise=0.05, noise_ramp=0.75, noise_regularize=1e5,
            mse=0.0, w_plus=False, latent_init=None, lpips=None, lpips_size=256, generator=None, callback=None, n_mean_latent=10000):
    """Project `target` [B,3,h,w] in [-1,1], given at h = min(g_ema.size, lpips_size), into the latent space of the frozen generator
    `g_ema`.  Per step i (projector.py): t = i / steps; lr_t = get_lr(t, lr, lr_rampdown, lr_rampup); the latent gets Gaussian noise of
    strength latent_std * noise * max(0, 1 - t / noise_ramp)^2; img = g_ema([latent], input_is_latent=True, noise=noises); the loss is
    LPIPS(small, target).sum() + noise_regularize * L(noises) + mse * MSE(small, target) with small = the box mean of img at the
    target's size; one Adam step on [latent] + noises; the maps are renormalised.

    Start: the mean latent of `n_mean_latent` samples, or `latent_init` ([B,512] or [B,n_latent,512], e.g. the e4e encoder's codes);
    w_plus repeats a [B,512] start to n_latent rows and optimises them separately.  The noise maps come from g_ema.make_noise(), redrawn
    normal: [1,1,H,W] for B = 1 (the fused StyledConv and its noise-map gradient), per-sample [B,1,H,W] for B > 1 (the unfused composition,
    autograd's gradient).  `lpips`: a where2edit_amd.LPIPS on the same device (default: a new one, seeded random weights unless files
    were loaded -- see lpips.py).  `generator`: a torch.Generator for every random draw (a CPU generator draws on the host).
    `callback(i, loss, img)` after every step (tensors; reading them synchronises).  Returns a `Projection`.  Not graph-captured."""
    if not isinstance(g_ema, torch.nn.Module) or not hasattr(g_ema, "make_noise"):
        raise TypeError("project: g_ema must be a where2edit_amd.stylegan2.Generator")
    device = g_ema.input.input.device
    _require_gpu("project", target, g_ema.input.input)
    if any(p.requires_grad for p in g_ema.parameters()):
        raise ValueError("project: g_ema must be frozen (g_ema.requires_grad_(False)): the projector optimises the latent and the noise maps only")
    side = min(g_ema.size, int(lpips_size))
    if target.dim() != 4 or tuple(target.shape[1:]) != (3, side, side) or g_ema.size % side:
        raise ValueError(f"project: target must be [B,3,{side},{side}] (min(generator size, lpips_size)), got {tuple(target.shape)}")
    batch = target.shape[0]
    target = target.detach().to(device=device, dtype=torch.float32).contiguous()
    f = g_ema.size // side
    if lpips is None:
        from .lpips import LPIPS
        lpips = LPIPS().to(device)

    latent_mean, latent_std = latent_statistics(g_ema, n_mean_latent, generator)
    if latent_init is not None:
        _require_gpu("project", latent_init)
        latent = latent_init.detach().to(device=device, dtype=torch.float32).clone()
        if latent.shape[0] != batch or latent.shape[-1] != g_ema.style_dim or latent.dim() not in (2, 3) or \
                (latent.dim() == 3 and latent.shape[1] != g_ema.n_latent):
            raise ValueError(f"project: latent_init must be [{batch},{g_ema.style_dim}] or [{batch},{g_ema.n_latent},{g_ema.style_dim}], "
                             f"got {tuple(latent_init.shape)}")
    else:
        latent = latent_mean.detach().clone().repeat(batch, 1)
    if w_plus and latent.dim() == 2:
        latent = latent.unsqueeze(1).repeat(1, g_ema.n_latent, 1)
    latent = latent.contiguous().requires_grad_(True)
    noises = []
    for n in g_ema.make_noise():
        shape = (batch,) + tuple(n.shape[1:])
        noises.append(_randn(shape, device, generator).contiguous().requires_grad_(True))

    from .adam import Adam
    optimizer = Adam([latent] + noises, lr=lr)
    losses, mses = [], []
    for i in range(steps):
        t = i / steps
        optimizer.param_groups[0]["lr"] = get_lr(t, lr, lr_rampdown, lr_rampup)
        strength = latent_std * (noise * max(0.0, 1.0 - t / noise_ramp) ** 2)
        img, _ = g_ema([latent_noise(latent, strength, generator)], input_is_latent=True, noise=noises)
        small, mse_loss = loss_front(img, target, f)
        loss = lpips(small, target).sum() + noise_regularize * _noise_regularize(noises)
        if mse:
            loss = loss + mse * mse_loss
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        noise_normalize_(noises)
        losses.append(loss.detach())
        mses.append(mse_loss.detach())
        if callback is not None:
            callback(i, losses[-1], img.detach())
    with torch.no_grad():
        img, _ = g_ema([latent], input_is_latent=True, noise=noises)
    empty = torch.empty(0, device=device)
    return Projection(latent.detach(), [n.detach() for n in noises], img.detach(), torch.stack(losses) if losses else empty,
                      torch.stack(mses) if mses else empty)


def save_projection(path, result, names):
    """Write projector.py's result file: {name: {"img": [3,H,W], "latent": [512] or [n_latent,512], "noise": [the [1,1,s,s] maps of that
    sample]}} for the samples of `result` (a Projection) under `names`.  Shared maps (B = 1) go to the one sample.  Returns the dict;
    path None: only returns it."""
    names = list(names)
    if len(names) != result.latent.shape[0]:
        raise ValueError(f"save_projection: {len(names)} names for {result.latent.shape[0]} projected samples")
    if len(set(names)) != len(names):
        raise ValueError("save_projection: the names must be distinct")
    out = {}
    for i, name in enumerate(names):
        out[name] = {"img": result.img[i].detach().cpu(), "latent": result.latent[i].detach().cpu(),
                     "noise": [n[i:i + 1].detach().cpu() if n.shape[0] > 1 else n.detach().cpu() for n in result.noises]}
    if path is not None:
        torch.save(out, path)
    return out
