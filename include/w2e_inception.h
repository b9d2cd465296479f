/* w2e_inception.h -- C ABI of the Inception-v3 feature extractor's kernels (csrc/inception.hip) in libw2e.so (gfx950): the network
 * behind the reference's FID / Inception Score evaluation (utils.py:434-551 cal_evaluation / generate_imgs, which calls torch_fidelity).
 * Same conventions as w2e.h: device pointers, fp32 NCHW, caller-allocated outputs, asynchronous on `stream` (void*), no allocation,
 * copy, memset or atomic inside, 0 = OK, otherwise w2e_last_error(); arguments are checked before any HIP call.
 */
#ifndef W2E_INCEPTION_H
#define W2E_INCEPTION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define W2E_INCEPTION_SIZE 299 /* the side of the network's input */

/* ---- convolution + folded BatchNorm + activation ----
 * y[b, y_ch_off + o, oh, ow] = act(scale[o] * sum_{c,i,j} w[o,c,i,j] * x[b, c, oh*stride - ph + i, ow*stride - pw + j] + shift[o])
 * with zeros outside x; OH = (h + 2 ph - kh) / stride + 1 (floored), OW likewise.  act = max(., 0) when relu != 0, the identity
 * otherwise.  scale NULL = 1, shift NULL = 0.
 * x [batch, cin, h, w]; wt [n, cin, kh, kw] as stored (OIHW); y has y_channels channels, of which [y_ch_off, y_ch_off + n) are
 * written and no other byte is touched: the branches of an Inception block fill their slices of the concatenated tensor.
 * kh, kw in {1,3,5,7} (any pair), stride 1 or 2, 0 <= ph < kh, 0 <= pw < kw.  x, wt and y below 2 GiB each.
 * One implicit-GEMM kernel, M = batch*OH*OW, N = n, K = cin*kh*kw, all three ragged: plain fp32 products on
 * v_mfma_f32_32x32x2_f32 (no reduced-precision operand mode), every output summed by one wave in one accumulator over k in a fixed
 * order -- no atomics, no split of K, so two runs give the same bits.  A fully connected layer is the 1x1 case on [batch, cin, 1, 1]. */
int w2e_conv2d_bn_relu(const float* x, const float* wt, const float* scale, const float* shift, float* y, int batch, int cin, int h,
                       int w, int n, int kh, int kw, int stride, int ph, int pw, int relu, int y_channels, int y_ch_off, void* stream);

/* ---- 3x3 pooling ----
 * mode W2E_POOL_MAX_S2:   max, stride 2, no padding: [h, w] -> [(h-3)/2 + 1, (w-3)/2 + 1] (floored); h, w >= 3.
 * mode W2E_POOL_AVG_S1P1: average, stride 1, padding 1, the divisor being the number of taps inside the image
 *                         (avg_pool2d(count_include_pad=False)); taps are added in row-major order; h, w >= 1.
 * mode W2E_POOL_MAX_S1P1: max, stride 1, padding 1; a padded tap never wins.
 * The max modes follow PyTorch's max_pool2d as w2e_maxpool2x2_fwd does: the first maximum in row-major window order wins, a NaN in
 * the window propagates.  x [batch, channels, h, w]; y has y_channels channels, [y_ch_off, y_ch_off + channels) are written. */
#define W2E_POOL_MAX_S2 0
#define W2E_POOL_AVG_S1P1 1
#define W2E_POOL_MAX_S1P1 2
int w2e_pool3x3(const float* x, float* y, int batch, int channels, int h, int w, int mode, int y_channels, int y_ch_off, void* stream);

/* ---- input ----
 * The legacy-TensorFlow bilinear resize of torch_fidelity's extractor to 299 x 299, then (v - 128) / 128, in one launch:
 *   src = dst * (in / 299) (no half-pixel offset), i0 = floor(src), i1 = min(i0 + 1, in - 1), t = src - i0,
 *   v = top + (bottom - top) * ty with top = a + (b - a) * tx along the row, in fp32.
 * i0 and t come from the integer quotient and remainder of dst * in by 299, so no position is rounded; a 299 x 299 input passes
 * through unchanged.  src: uint8 NHWC [batch, in_h, in_w, 3]; dst: fp32 NCHW [batch, 3, 299, 299].  in_h, in_w in 1..16384. */
int w2e_inception_resize(const uint8_t* src, float* dst, int batch, int in_h, int in_w, void* stream);

#ifdef __cplusplus
}
#endif
#endif
