/* w2e_lpips.h -- C ABI of the LPIPS head (Zhang et al. 2018, "The Unreasonable Effectiveness of Deep Features as a Perceptual
 * Metric", version 0.1 of the published code) in libw2e.so (gfx950): the one part of LPIPS-VGG that the VGG16 kernels of
 * w2e_irse.h (w2e_conv3x3 with the ReLU epilogue, w2e_maxpool2x2_*, w2e_affine_act_*) do not already cover.
 *
 * For one tap (a post-ReLU feature map) of two image batches, per pixel p with C channels:
 *     n  = sqrt(sum_c f_c^2),   a = n + 1e-10,   u = f / a          (unit-normalise across channels)
 *     d  = mean_p sum_c lin_c (u0_c - u1_c)^2                        (the 1x1 "lin" layer on the squared difference, spatial mean)
 * The distance is computed in this DIFFERENCE form, never as the expansion sum w u0^2 - 2 sum w u0 u1 + sum w u1^2, which cancels for
 * near-equal inputs; identical inputs give exactly 0.
 *
 * Zero-norm convention: at a pixel whose feature vector is all zero, n = 0 and u = 0, and the second (projection) term of the
 * gradient below is DEFINED as 0 there (autograd through sqrt gives NaN at that point).  Behind the tap's ReLU mask [f > 0] that
 * pixel's gradient is then exactly 0, and every output is finite.
 *
 * Same conventions as w2e_irse.h: device fp32 pointers, NCHW with the spatial dimensions flattened to `pixels`, caller-allocated
 * outputs and workspace, asynchronous on `stream` (a hipStream_t as void*), arguments checked before any HIP call, 0 = OK, otherwise
 * the message is w2e_last_error().  No atomics, no memset, no host synchronisation: both calls capture into a hipGraph.
 */
#ifndef W2E_LPIPS_H
#define W2E_LPIPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Floats of the partials slab w2e_lpips_head_fwd reduces through, PER IMAGE of f0 (the caller allocates batch times this, at least). */
#define W2E_LPIPS_PARTIALS 1024

/* out[b] = d of image b:  f0 [batch, channels, pixels], f1 [batch1, channels, pixels] with batch1 = batch or 1 (broadcast over the
 * batch), lin [channels].  Bit-reproducible: every workgroup leaves the sum of its pixel tiles in `partials` (n_partials >= batch *
 * W2E_LPIPS_PARTIALS floats, checked), then one workgroup per image adds them in a fixed order.  The grid depends on (channels,
 * pixels) only, so out[b] does not depend on the batch it was computed in. */
int w2e_lpips_head_fwd(const float* f0, const float* f1, const float* lin, int batch, int batch1, int channels, int64_t pixels,
                       float* partials, int n_partials, float* out, void* stream);

/* The adjoint.  gout [batch] is the gradient arriving at out.  With e = u0 - u1 and q_c = (gout[b] / pixels) * 2 lin_c e_c:
 *     d/df0_j =  q_j / a0 - f0_j (sum_c q_c f0_c) / (n0 a0^2)
 *     d/df1_j = -q_j / a1 + f1_j (sum_c q_c f1_c) / (n1 a1^2)          (second terms 0 where n = 0: the convention above)
 * g0 [batch, channels, pixels]; g1 (optional, same shape) only with batch1 = batch.
 * accumulate != 0: the result is added to what g0 / g1 hold (a tap also feeds the next slice: the head's gradient joins the one
 * arriving from there).  relu != 0: the tap's own ReLU mask is folded in, after the addition:
 *     g0 = [f0 > 0] * ((accumulate ? g0 : 0) + d/df0),   g1 likewise with [f1 > 0]
 * which is the gradient at the tap's pre-activation (y = relu(pre), y > 0 exactly where pre > 0). */
int w2e_lpips_head_bwd(const float* f0, const float* f1, const float* lin, const float* gout, int batch, int batch1, int channels,
                       int64_t pixels, float* g0, float* g1, int accumulate, int relu, void* stream);

#ifdef __cplusplus
}
#endif
#endif
