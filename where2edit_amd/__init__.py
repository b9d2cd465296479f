"""where2edit_amd -- MI355X-native hot path of Where2edit (StyleGAN2 generator stack, region-attention
blend, CLIP ViT-B/32 image encoder) behind the reference's Python module/operator surface.

Layout:
  csrc/ + lib/libw2e.so   hand-written HIP (gfx950) behind the C ABI of include/w2e.h
  _abi.py                 the prototypes, structs and integer constants of include/*.h, read from the headers (no hand-written copy)
  _lib.py                 ctypes door to that library (no fallback)
  functional.py           torch.autograd.Functions over the C ABI
  op/                     models/stylegan2/op seam: FusedLeakyReLU, fused_leaky_relu, upfirdn2d
  stylegan2.py            models/stylegan2/model.py surface (Generator, ModulatedConv2d, ...)
  attention_model.py      attention/attention_model.py Generator (features + region blend)
  latent_mappers.py, styleclip_mapper.py   mapper/ surface
  clip_vit.py, clip_loss.py                criteria/clip_loss.py surface + ViT-B/32
  id_loss.py, irse_hip.py                  criteria/id_loss.py surface + IR-SE50 on the conv engine
  perceptual_loss.py                       criteria/perceptual_loss.py surface: VGG16 relu2_2 MSE on the conv engine
  vgg16.py                the VGG16 trunk under perceptual_loss.py and lpips.py: table, module tree, checkpoint mapper, plan, slice walks
  derived.py              the one cache of tensors derived from frozen parameters, and invalidate (= stylegan2.invalidate_caches)
  coach.py, ranger.py     the mapper training step (mapper/training/coach.py:70-92) + optimizer
  _fused_opt.py           what Ranger and Adam share around their one-launch kernels (csrc/multi_tensor.h on the C side)
  run_attention.py, region_style_hip.py, adam.py   the region-attention net and its training step (attention/run_attention.py): the
                          style branch as one node on csrc/region_style.hip, `Adam` = torch.optim.Adam's rule as one launch
  dist.py                 data-parallel step: shard latents, one RCCL all-reduce of mapper grads
  evaluation.py           the region mask's IoU against parsing labels (utils.py:639-726): MaskIoU, calculate_iou; FID / Inception Score /
                          identity / CLIP-improvement of edits (utils.py:434-551): calculate_metrics, EditMetrics
  inception.py            the Inception-v3 feature extractor of FID / IS on csrc/inception.hip: FeatureExtractorInceptionV3
  lpips.py                LPIPS (VGG16, v0.1) on the VGG16 kernels and the head of csrc/lpips.hip: LPIPS; evaluation.lpips_distance
  image_io.py             bytes in, bytes out on csrc/image.hip: Pillow's resize + ToTensor / Normalize (to_tensor, label_ids, resize_u8),
                          torchvision's save_image up to the PNG encoder (to_bytes), its .jpg file (to_jpeg, save_image), and
                          baseline JPEG files in (from_jpeg, load_image) on csrc/jpeg.hip and csrc/jpeg_decode.hip, PNG files in
                          (from_png, load_png, read_image) on csrc/png.hip
"""
__version__ = "0.1.0"


def set_deterministic(enabled=True):
    """Bit-reproducible results, the counterpart of the reference's `cudnn.deterministic = True`
    (attention/run_attention.py:903-904): libw2e.so stops using fp32 atomics (no split-K, fixed-order reductions;
    w2e_set_option("deterministic")) and PyTorch's own ops are switched to their deterministic algorithms (rocBLAS
    without atomics).  Costs a few percent of throughput; off by default."""
    import torch
    from . import _lib
    _lib.set_option("deterministic", 1 if enabled else 0)
    torch.use_deterministic_algorithms(bool(enabled), warn_only=True)


def train_conv_weights(module):
    """Opt-in decoder fine-tuning (stylegan2.train_conv_weights): every ModulatedConv2d weight under `module` requires grad and gets
    its gradient from the conv-weight-gradient kernels; stylegan2.freeze_conv_weights undoes it."""
    from .stylegan2 import train_conv_weights as _train
    return _train(module)


def train_mask_branch(net, enabled=True):
    """Opt-in training of the region-attention mask branch (run_attention.train_mask_branch): every `attention*` / `initial*`
    parameter of `net` requires grad and gets its gradient from the mask-branch backward kernels; run_attention.freeze_mask_branch
    (or enabled=False) undoes it."""
    from .run_attention import train_mask_branch as _train
    return _train(net, enabled)


def r1_penalty(discriminator, real, return_logits=False):
    """The R1 gradient penalty of a stylegan2.Discriminator on `real` (disc_hip.r1_penalty): one HIP autograd node over the
    Discriminator's parameters; `(r1_gamma / 2 * r1_penalty(d, real) * d_reg_every).backward()` is the lazy-regularisation step."""
    from .disc_hip import r1_penalty as _r1
    return _r1(discriminator, real, return_logits)


# where2edit_amd.evaluation's public names, importable from the package (resolved on first use: importing the package stays light)
_EVALUATION = ("CELEBAMASK_REGIONS", "region_lut", "binarise", "attention_with_text", "MaskIoU", "calculate_iou", "celebamask_samples",
               "fid_from_features", "isc_from_logits", "calculate_metrics", "EditMetrics", "lpips_distance")
_IMAGE_IO = ("resample_tables", "resize_u8", "to_tensor", "label_ids", "to_bytes", "jpeg_tables", "jpeg_header", "jpeg_coefficients", "to_jpeg",
             "save_image", "jpeg_parse", "jpeg_decode_states", "jpeg_decode_coefficients", "jpeg_pixels", "from_jpeg", "load_image",
             "png_parse", "png_plan", "png_inflate", "png_pixels", "from_png", "load_png", "read_image", "png_encode_plan", "png_filter", "png_deflate",
             "to_png", "save_png")
_PROJECTOR = ("project", "save_projection", "noise_regularize", "noise_normalize_", "latent_noise", "latent_statistics", "loss_front",
              "Projection")


def __getattr__(name):
    if name == "Adam":  # torch.optim.Adam's rule and state, the update as one launch (adam.py)
        from .adam import Adam
        return Adam
    if name == "FeatureExtractorInceptionV3":  # the FID / Inception Score network on csrc/inception.hip (inception.py)
        from .inception import FeatureExtractorInceptionV3
        return FeatureExtractorInceptionV3
    if name == "LPIPS":  # the perceptual metric: VGG16 on the conv engine, the head on csrc/lpips.hip (lpips.py)
        from .lpips import LPIPS
        return LPIPS
    if name in _EVALUATION:
        from . import evaluation
        return getattr(evaluation, name)
    if name in _PROJECTOR:  # StyleGAN2's projector: w / W+ and the noise maps against LPIPS (projector.py, csrc/projector.hip)
        from . import projector
        return getattr(projector, name)
    if name in _IMAGE_IO:
        from . import image_io
        return getattr(image_io, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
