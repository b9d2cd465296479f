/* w2e_image.h -- C ABI of the image I/O kernels (csrc/image.hip): the two ends of the reference's real-image paths in libw2e.so
 * (gfx950).  In: Pillow's 8-bit `Image.resize` (BILINEAR with its antialiasing window, NEAREST) followed by ToTensor + Normalize
 * (show_demo/try_demo.py:96-99, utils.py:594-619 transform_img / transform_label).  Out: torchvision 0.8.2's
 * `save_image(..., normalize=True, range=(lo, hi))` up to the bytes it hands to the PNG encoder (mapper/scripts/inference.py:70-77,
 * utils.py:493-503).  Both are restated in integers / separately rounded fp32 operations, so the results are the reference's own
 * pixel values, not approximations of them (DESIGN.md "Image I/O").
 * Same conventions as w2e.h: device pointers, caller-allocated outputs and workspace, asynchronous on `stream` (void*), no
 * allocation, copy, memset or atomic inside, 0 = OK, otherwise w2e_last_error(); arguments are checked before any HIP call.
 */
#ifndef W2E_IMAGE_H
#define W2E_IMAGE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2E_IMAGE_MAX_SIZE 16384      /* largest height / width, in and out */
#define W2E_IMAGE_PRECISION_BITS 22   /* the fixed point of the coefficient tables (Pillow Resample.c: 32 - 8 - 2) */

/* ---- resample ----
 * One axis, `in` -> `out` samples (where2edit_amd/image_io.py resample_tables computes these on the host, in double):
 *   K [out, ksize] int32: the window's coefficients in 2^-22 units, zero past the window's n entries;
 *   bounds [out, 2] int32: (first input index of the window, n).
 *   out[o] = clamp((2^21 + sum_{t<n} in[first + t] * K[o,t]) >> 22, 0, 255)                      (int32 throughout)
 * The horizontal pass runs first, into bytes; the vertical pass reads those bytes.  An axis with in == out is not passed (its tables
 * are NULL / ignored).  Channels are independent.  NEAREST is the same machinery with ksize = 1, K = 2^22.
 * Window indices are clamped to the image in the kernels and n to ksize: a wrong table gives wrong pixels, never an access outside
 * `src`.
 *
 * w2e_image_resize_plan (pure host): which form w2e_image_resize takes for these sizes.
 *   plan[0]  0 = fused: one launch; a 256-thread workgroup owns a tile of output rows x columns of one image, stages the input span
 *                under it in LDS, runs the horizontal pass into an LDS byte tile and the vertical pass from there;
 *            1 = two launches (horizontal, vertical) through `workspace`: taken when the fused tile's input span does not fit in
 *                64 KB of LDS (strong down-scaling: the span grows with in / out)
 *   plan[1]  bytes of workspace the call needs (0 for the fused form or when at most one axis is passed)
 *   plan[2], plan[3]  ksize of the BILINEAR tables of the x / y axis (0 for an axis that is not passed)
 *   plan[4], plan[5]  the fused form's tile: output rows, output columns (0 for form 1)
 *   plan[6]  the fused form's dynamic LDS in bytes (0 for form 1)
 * `plan` has 8 entries (plan[7] is reserved, 0).  channels is 1 or 3; every size is in 1..W2E_IMAGE_MAX_SIZE; batch >= 0. */
int w2e_image_resize_plan(int batch, int channels, int in_h, int in_w, int out_h, int out_w, int64_t* plan);

/* src: contiguous NHWC bytes [batch, in_h, in_w, channels], any alignment (16-byte loads where the address allows, bytes at the
 * ragged ends).  kx [out_w, ksize_x], bx [out_w, 2]: device tables of the horizontal axis, required when in_w != out_w, ignored
 * otherwise; ky, by likewise for the vertical axis.  ksize_x / ksize_y: the row length of the K tables handed in (the BILINEAR
 * ksize of the plan, or 1 for NEAREST).
 * lut: [channels, 256] floats (ToTensor + Normalize as a table: lut[c][v] = float32((float32(v) / 255 - mean[c]) / std[c]), computed
 * by the caller).  With it, dst is fp32 NCHW [batch, channels, out_h, out_w] = lut[c][resized byte]; with NULL, dst is uint8 NHWC
 * [batch, out_h, out_w, channels].  workspace: plan[1] bytes (may be NULL when that is 0).  An empty batch returns 0 without a
 * launch. */
int w2e_image_resize(const uint8_t* src, int batch, int channels, int in_h, int in_w, int out_h, int out_w, const int32_t* kx,
                     const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, const float* lut, void* dst,
                     void* workspace, void* stream);

/* ---- quantise ----
 * torchvision 0.8.2 make_grid(normalize=True, range=(lo, hi)) + save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8), every
 * step a separately rounded fp32 operation in this order (nothing is contracted into a fused multiply-add, the division is a
 * division):
 *   t = (min(max(x, lo), hi) + (-lo)) / divisor          divisor = float32(hi - lo + 1e-5), the sum taken in double by the caller
 *   q = trunc(min(max(t * 255 + 0.5, 0), 255))           a NaN gives 0
 * src: fp32 NCHW [batch, channels, h, w], channels 1 or 3.
 * grid != 0: dst is make_grid's canvas as HWC bytes.  batch == 1: [h, w, 3], unpadded.  Otherwise xmaps = min(nrow, batch),
 *   ymaps = ceil(batch / xmaps), dst is [ymaps * (h + padding) + padding, xmaps * (w + padding) + padding, 3]; image k sits at row
 *   (k / xmaps) * (h + padding) + padding, column (k % xmaps) * (w + padding) + padding; every other byte is
 *   trunc(min(max(pad_value * 255 + 0.5, 0), 255)).  A 1-channel source is replicated to the 3 channels.
 * grid == 0: dst is [batch, h, w, channels] bytes: no padding, no replication (nrow, padding and pad_value are ignored).
 * One streaming kernel: planar float reads, interleaved byte writes as whole 32-bit words (bytes at a ragged tail).  dst must be
 * 4-byte aligned.  lo < hi, divisor > 0, none of them NaN; nrow >= 1; 0 <= padding <= 1024. */
int w2e_image_quantize(const float* src, int batch, int channels, int h, int w, float lo, float hi, float divisor, int nrow,
                       int padding, float pad_value, int grid, uint8_t* dst, void* stream);

#ifdef __cplusplus
}
#endif
#endif
