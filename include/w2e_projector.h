/* w2e_projector.h -- C ABI of the StyleGAN2 projector's own arithmetic in libw2e.so (gfx950): Karras et al. 2020, "Analyzing and
 * Improving the Image Quality of StyleGAN", Appendix D, as rosinality's projector.py runs it around the generator of
 * models/stylegan2/model.py.  The generator pass, LPIPS (w2e_lpips.h) and Adam (w2e_adam_step) are the library's other entry points;
 * here are the noise-map gradient of the fused StyledConv, the multi-scale noise regulariser with its gradient, the in-place
 * renormalisation of the noise maps and the loss front (box down-sampling to the LPIPS resolution with the MSE term).
 *
 * Same conventions as w2e_lpips.h: device fp32 pointers unless stated, caller-allocated outputs and workspaces, asynchronous on
 * `stream` (a hipStream_t as void*), arguments checked before any HIP call, 0 = OK, otherwise the message is w2e_last_error().
 * No atomics, no memset, no host synchronisation; every sum runs in one fixed order, so every output is bit-reproducible.
 * Lists of maps travel as HOST arrays of device pointers with host arrays of their dimensions (the scheme of w2e_adam_step).
 * What is not supported is refused with an error before anything is launched.
 */
#ifndef W2E_PROJECTOR_H
#define W2E_PROJECTOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Partial-sum slots per map (normalise) and per (map, level) (regulariser); 16 bytes each (two doubles). */
#define W2E_PROJ_SLOTS 64
/* Most blocks (= double partial sums) w2e_proj_front_fwd writes. */
#define W2E_PROJ_FRONT_PARTIALS 1024

/* Replaces: autograd's gradient of `image + self.weight * noise` (NoiseInjection, model.py:279-290) with respect to a shared
 * [1,1,oh,ow] noise map, which the fused StyledConv backward did not return:
 *     g_noise[p] (+)= noise_w[0] * sum_{plane < planes} gpre[plane, p],      p < pixels
 * gpre [planes, pixels] is the pre-activation gradient the backward already holds (planes = batch * cout rows that carry a
 * gradient); noise_w points at the layer's one strength on the device.  accumulate != 0 adds to what g_noise holds.  The planes
 * are summed in a fixed order that depends on (planes, pixels) only: S = w2e_noise_grad_slices(planes, pixels) interleaved slices
 * (plane % S), each in ascending order, then the slices in ascending order. */
int w2e_noise_grad(const float* gpre, const float* noise_w, float* g_noise, int64_t planes, int64_t pixels, int accumulate,
                   void* stream);
int w2e_noise_grad_slices(int64_t planes, int64_t pixels);

/* Replaces: noise_regularize(noises) of projector.py and its autograd gradient, about 25 stock ops per pyramid level and map:
 *     L = sum_maps sum_levels mean(n * roll(n, 1, dim 3))^2 + mean(n * roll(n, 1, dim 2))^2
 * over maps[i] = [batch[i], 1, size[i], size[i]], size a power of two; level 0 is the map, level j + 1 the 2x2 box mean of level j,
 * the last level being the first of at most 8 x 8 (a 4^2 or 8^2 map has one level, a 1024^2 map eight).  The rolls wrap; the means
 * run over the whole tensor, batch included.  The products are formed and summed in double (a float product is exact there): for white
 * noise a mean of products is about 1/sqrt(N) of the mean of their magnitudes, and the projector weighs L by 1e5.
 *
 * workspace: the `floats` w2e_noise_reg_workspace(...) reports (a host int64), at an 8-byte aligned address; it holds the partial sums,
 * the two means of every (map, level), the pooled levels and, after _bwd, the gradients of the pooled levels.  _fwd fills it and writes
 * loss[0]; _bwd must get the workspace _fwd left, with the same lists, and writes (accumulate = 0) or adds (!= 0)
 *     grads[i] = gout[0] * dL / d maps[i]
 * through every level: the two neighbours of each product plus a quarter of the coarser level's gradient.  gout: one float on the
 * device.  Launches: one per pyramid step, one or two for the products, the means and the final sum; per table of 64 (map, level)
 * pairs, not per map. */
int w2e_noise_reg_workspace(int count, const int* batch, const int* size, int64_t* floats);
int w2e_noise_reg_fwd(int count, const float* const* maps, const int* batch, const int* size, float* workspace,
                      int64_t workspace_floats, float* loss, void* stream);
int w2e_noise_reg_bwd(int count, const float* const* maps, const int* batch, const int* size, float* workspace,
                      int64_t workspace_floats, const float* gout, float* const* grads, int accumulate, void* stream);

/* Replaces: noise_normalize_(noises) of projector.py (mean, std, sub, div per map):  n <- (n - mean(n)) / std(n) in place, torch's
 * unbiased std, per map over its numel[i] >= 2 elements.  Sums of x and x^2 in double; two launches per table of 64 maps.
 * workspace: at least count * W2E_PROJ_SLOTS * 4 floats (8-byte aligned). */
int w2e_noise_normalize(int count, float* const* maps, const int64_t* numel, float* workspace, int64_t workspace_floats, void* stream);

/* Replaces: the down-sampling `img.reshape(b, c, h // f, f, w // f, f).mean([3, 5])` of projector.py and F.mse_loss(img, target):
 *     small[b,c,y,x] = mean of the f x f box of img [batch, channels, height, width];   f = 1: a copy
 *     partials[k]    = block k's sum of (small - target)^2, in double; k < w2e_proj_front_blocks(numel of small) <= W2E_PROJ_FRONT_PARTIALS
 * height and width must be multiples of f; target has small's shape.  target NULL: no partial sums. */
int w2e_proj_front_blocks(int64_t small_numel);
int w2e_proj_front_fwd(const float* img, const float* target, int batch, int channels, int height, int width, int f, float* small,
                       double* partials, void* stream);
/* The adjoint, written at the generator's resolution:
 *     g_img[b,c,y,x] = (g_small[b,c,y/f,x/f] + coef * g_mse[0] * (small - target)[b,c,y/f,x/f]) / f^2
 * g_small NULL: that term is 0; g_mse (one float on the device) NULL: the MSE term is 0 (small and target are then not read).
 * coef: 2 / numel(small) for the mean squared error. */
int w2e_proj_front_bwd(const float* g_small, const float* small, const float* target, const float* g_mse, float coef, int batch,
                       int channels, int height, int width, int f, float* g_img, void* stream);

#ifdef __cplusplus
}
#endif
#endif
