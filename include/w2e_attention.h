/* w2e_attention.h -- C ABI of the region-attention mask kernels in libw2e.so (gfx950).
 *
 * They replace the mask branch of `FullSpaceMapperFEATClusterLinStyle_Net.forward`
 * (attention/run_attention.py:754-893) -- the model the reference repository is named after:
 *   w2e_cluster_assign    :775-792  nearest k-means centroid per feature pixel; the reference builds the position
 *                                   channels, a [B*s*s, C+2P] copy and a [N,K,C+2P] broadcast temp (utils.py:244-263)
 *   w2e_attention_logits  :796-841  1 + 17 `StyledConv(C, 32, 1)` on cached generator activations, nearest-resized to
 *                                   `size`, concatenated, `StyledConv(576, 1, 1)`, + initial_bias, sigmoid
 *   w2e_cluster_pool      :843-884  per-(sample, cluster) mean (the reference's Python loop over B*K boolean masks),
 *                                   straight-through threshold 0.8, torchvision gaussian_blur(5)
 * Same conventions as w2e.h (device fp32 pointers, caller-allocated outputs / workspaces, stream as void*, 0 = OK).
 * The reference's schedule keeps every `attention*` / `initial*` parameter frozen while `t < 1.15` (run_attention.py:1076-1083),
 * which always holds, so by default only the forward kernels run.  A user who lowers that literal trains the branch: the
 * opt-in backward is
 *   w2e_attention_logits_train   the forward above, also keeping the 32 conv sums per (source, pixel) for the backward
 *   w2e_attention_logits_bwd     g_each -> every mask parameter's gradient (no gradient for the cached activations)
 *   w2e_cluster_pool_bwd         g_final + the gradients of loss_reg / loss_tv -> g_each
 * All fp32, no atomics, no memsets, fixed-order reductions (bit-reproducible), no host synchronisation.
 */
#ifndef W2E_ATTENTION_H
#define W2E_ATTENTION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* assign[b,y,x] = argmin_k sum_c (f[b,c,y,x] - cen[k,c])^2 + sum_p (xpos(x) - cen[k,C+p])^2 + sum_p (ypos(y) - cen[k,C+P+p])^2
 * with xpos(x) = 2x/(S-1) - 1, ypos likewise; feat [B,C,S,S]; centroids [K, C+2P] row-major; assign int32 [B,S,S].
 * Ties go to the lowest k (torch.argmin).  K <= 32, (C+2P)*K*4 <= 160 KB of LDS. */
int w2e_cluster_assign(const float* feat, const float* centroids, int32_t* assign, int batch, int channels, int pos_channels,
                       int size, int clusters, void* stream);

/* Lloyd's centroid-update step for the offline clustering (attention/clustering_feature.py:212-235, 373-397):
 * partial[b,k,d] = sum over the pixels of image b assigned to cluster k of dimension d (d < C: feat[b,d,.]; then the P
 * x-position and P y-position channels, evaluated as in w2e_cluster_assign), counts[b,k] = number of such pixels.
 * partial [B,K,C+2P], counts [B,K]; written, not accumulated; the caller sums over b.  K <= 32. */
int w2e_cluster_accumulate(const float* feat, const int32_t* assign, float* partial, float* counts, int batch, int channels,
                           int pos_channels, int size, int clusters, void* stream);

/* ---- offline k-means at the reference's scale (clustering_feature.py:347-397: 300 x [1,512,128,128] points, sklearn KMeans) ----
 * One persistent kernel in three modes over the same points ([B,C,S,S] + the 2P analytic position channels), a grid of
 * `grid` workgroups (w2e_kmeans_plan) walking 128-pixel tiles, each writing one row of `partial` (written, not accumulated):
 *   mode 0  assignment:  assign[b,y,x] exactly as w2e_cluster_assign (bit-identical distances), mind[b,y,x] = the squared distance
 *           to that centre (assign / mind may be NULL); partial [grid][1] = the workgroup's share of the inertia.  Takes every
 *           shape w2e_cluster_assign takes (up to D = 1024 at K = 32).
 *   mode 1  fused Lloyd step: mode 0 plus the per-cluster sums and counts of the tile, taken while it is still in cache;
 *           partial [grid][K*(D+1) + 1]: [k][d] sums (d < D = C+2P), [k][D] the count, then the inertia share.  Needs an even S
 *           and centres + sums within the 160 KB of LDS (w2e_kmeans_plan reports `fused` = 0 otherwise: run mode 0 and
 *           w2e_cluster_accumulate instead).
 *   mode 2  k-means++ seeding pass: `centroids` = T <= 8 candidate centres [T][D] (clusters = T); cand_dist[t*cand_ld + n] =
 *           |x_n - c_t|^2 for every point n = b*S*S + y*S + x (kept so that the chosen candidate is committed with one
 *           elementwise minimum, no second walk of the features); partial [grid][T] = shares of the T potentials
 *           sum_n min(mind[n], |x_n - c_t|^2); mind is read (NULL = +inf: the first centre).
 * No atomics: per-lane running sums in tile order, wave shuffles, one owner per LDS column; the result depends on the data and
 * on `grid` only.  K <= 32. */
int w2e_kmeans_plan(int batch, int channels, int pos_channels, int size, int clusters, int* grid, int* fused);
int w2e_kmeans_pass(int mode, const float* feat, const float* centroids, int32_t* assign, float* mind, float* cand_dist,
                    int64_t cand_ld, float* partial, int grid, int batch, int channels, int pos_channels, int size, int clusters,
                    void* stream);
/* acc[j] += sum over g < rows, in order, of partial[g][j] (j < n), in double: the fixed-order finish of the partials of one pass,
 * and -- called once per chunk of points -- of the chunks. */
int w2e_kmeans_reduce(const float* partial, int rows, int n, double* acc, void* stream);

#define W2E_ATT_MAX_SOURCES 32
/* One source = one cached activation and the 1x1 StyledConv(C, 32, 1, C) applied to it with a style given in S-space:
 *   a[b,o,p] = lrelu( d[b,o] * sum_i wscaled[o,i] * s[b,i] * feat[b,i,src(p)] + nw*noise[b,p] + bias[o] ) * sqrt2
 * evaluated only at the `size` x `size` pixels p that F.interpolate(., size) (nearest) would keep / replicate:
 * src(y,x) = (n(y), n(x)), n(t) = min(floor(t * ((float)res / (float)size)), res - 1) evaluated in fp32, as torch does (the
 * exact-integer floor(t*res/size) differs at some ratios that are no power of two).  w2e_cluster_pool and both backward entry
 * points read through the same index.  wscaled = scale*W [32,C];  d = the demodulation coefficients
 * [B,32]; noise [B,size*size] or NULL (NoiseInjection draws randn when no noise is passed: i.i.d., so drawing it
 * at the kept pixels is the same distribution), nw = device scalar noise strength. */
typedef struct {
    const float* feat;     /* [B, channels, res, res] */
    const float* wscaled;  /* [channels, 32] = (conv.weight[0,:,:,0,0] / sqrt(channels))^T: the transposed 1x1 weight */
    const float* style;    /* [B, channels] */
    const float* demod;    /* [B, 32] */
    const float* bias;     /* [32] (activate.bias) */
    const float* noise;    /* [B, size*size] or NULL */
    const float* noise_w;  /* device scalar (noise.weight) */
    int channels, res;
} w2e_att_source;

/* The demodulation coefficients of every source in one launch (model.py:244-246 for the [32,C,1,1] weights):
 *   sources[j].demod[b,o] = rsqrt( sum_i (wscaled_j[i,o] * style_j[b,i])^2 + eps )      (written; [B,32] per source)
 * Reads only wscaled / style / channels of each descriptor.  Deterministic. */
int w2e_attention_demod(const w2e_att_source* sources, int n_sources, int batch, float eps, void* stream);

/* each[b,p] = sigmoid( lrelu( d_last[b] * sum_{j,o} wlast[32j+o] * s_last[b,32j+o] * a_j[b,o,p] + nw_last*noise_last[b,p]
 *                              + bias_last ) * sqrt2 + initial_bias )
 * sources: HOST array of n_sources descriptors (copied into the launch).  wlast = scale*W of attention_last [32*n],
 * s_last [B,32*n], d_last [B], bias_last / initial_bias / nw_last device scalars, noise_last [B,size*size] or NULL.
 * partial: workspace of n_sources*B*size*size floats.  each: [B,size*size].  Deterministic (no atomics). */
int w2e_attention_logits(const w2e_att_source* sources, int n_sources, const float* wlast, const float* s_last,
                         const float* d_last, const float* bias_last, const float* noise_last, const float* nw_last,
                         const float* initial_bias, float* partial, float* each, int batch, int size, void* stream);

/* Per sample: mean of each[b,.] over the pixels of every cluster (assign given at cluster resolution csize, read through
 * the nearest resize to `size`), written back to the pixels -> same[b,p] (1.0 where a pixel's cluster id is out of
 * range); means[b,k] (NaN-free: 0 for empty clusters), counts[b,k];  thr = same < threshold ? 0 : same;
 * final = 5x5 gaussian (sigma 1.1, reflect padding) of thr.  size <= 128, K <= 32.  thr may be NULL. */
int w2e_cluster_pool(const float* each, const int32_t* assign, float* same, float* means, float* counts, float* thr,
                     float* final_map, int batch, int size, int csize, int clusters, float threshold, void* stream);

/* w2e_attention_logits with one more output: pre[j,b,o,p] = sum_i wscaled_j[i,o] * style_j[b,i] * feat_j[b,i,src(p)], the
 * modulated conv sums before demodulation ([n_sources, B, 32, size*size]); w2e_attention_logits_bwd reads them instead of
 * walking the activations a second time.  `partial` is an output here too (the backward reads it).  Same `each`, bit for bit. */
int w2e_attention_logits_train(const w2e_att_source* sources, int n_sources, const float* wlast, const float* s_last,
                               const float* d_last, const float* bias_last, const float* noise_last, const float* nw_last,
                               const float* initial_bias, float* partial, float* each, float* pre, int batch, int size,
                               void* stream);

/* Gradients of one source (all written, not accumulated; the paths through demod_j are included). */
typedef struct {
    float* g_wscaled;  /* [channels, 32] */
    float* g_style;    /* [B, channels] */
    float* g_bias;     /* [32] */
    float* g_noise_w;  /* [1] (0 when the source's noise is NULL) */
} w2e_att_source_grad;

/* Floats of workspace w2e_attention_logits_bwd needs (sum_channels = sum of the sources' channel counts):
 *   B*P + 4*B + n*B*32*P + n*B*ceil(P/256)*97 + n*B*32 + B*sum_channels*32      with P = size*size, n = n_sources */
#define W2E_ATT_BWD_WORKSPACE(n, B, P, sum_channels)                                                                   \
    ((int64_t)(B) * (P) + 4 * (int64_t)(B) + (int64_t)(n) * (B) * 32 * (P) + (int64_t)(n) * (B) * (((P) + 255) / 256) * 97 + \
     (int64_t)(n) * (B) * 32 + (int64_t)(B) * (sum_channels) * 32)

/* Backward of w2e_attention_logits_train.  g_each, each [B,size*size]; sources / wlast / s_last / d_last / biases / noises
 * exactly as the forward got them; partial and pre as the forward wrote them.  Outputs (written): grads[j] per source,
 * g_wlast [32n], g_s_last [B,32n] (both include the path through d_last, eps-free: d d_last / d x = -d_last^3 * x * w^2),
 * g_scalars [3] = gradients of initial_bias, bias_last, nw_last (the last is 0 when noise_last is NULL).
 * workspace: W2E_ATT_BWD_WORKSPACE floats (workspace_floats is checked against it).  Deterministic, no atomics. */
int w2e_attention_logits_bwd(const w2e_att_source* sources, const w2e_att_source_grad* grads, int n_sources, const float* wlast,
                             const float* s_last, const float* d_last, const float* bias_last, const float* noise_last,
                             const float* nw_last, const float* partial, const float* pre, const float* each,
                             const float* g_each, float* g_wlast, float* g_s_last, float* g_scalars, float* workspace,
                             int64_t workspace_floats, int batch, int size, void* stream);

/* Adjoint of w2e_cluster_pool plus the two loss terms of the net (run_attention.py:851-871):
 *   g_thr  = adjoint of the reflect-padded 5x5 gaussian applied to g_final (border taps fold back)
 *   g_same = g_thr (the straight-through threshold has slope 1 on both sides); 0 where the cluster id is out of range
 *   g_mean[b,k] = sum_{p in k} g_same[p] + g_loss_reg/B * [count > 0 and mean > 0.7]
 *   g_each[p] = g_mean[b,k(p)] / count[b,k(p)] + g_loss_tv * 2 (each[p] - same[p]) / (B*size*size)
 * g_loss_reg / g_loss_tv: device scalars (the upstream gradients of loss_reg = sum relu(mean - 0.7) / B and
 * loss_tv = mse(each, same.detach())), or NULL for 0.  g_final may be NULL for 0.  size <= 128, K <= 32. */
int w2e_cluster_pool_bwd(const float* g_final, const float* each, const float* same, const float* means, const float* counts,
                         const int32_t* assign, const float* g_loss_reg, const float* g_loss_tv, float* g_each, int batch,
                         int size, int csize, int clusters, void* stream);

/* ---- evaluation: the confusion counts of the mask IoU against parsing labels (utils.py:654-726; csrc/evaluate.hip) ----
 * mask [B,T,S,S] fp32, one soft or binary mask per prompt / region t; label [B,S,S] raw parsing ids; lut [256] raw id -> region in
 * 0..T (0 = none; the caller builds and validates it: an entry above T matches no region here); counts [T,3] 64-bit.
 * With pred = mask >= threshold (compared in fp32; a NaN is not predicted) and real = (lut[label] == t + 1):
 *   counts[t,0] += #(pred and real)    counts[t,1] += #pred    counts[t,2] += #real
 * ACCUMULATED, so that a caller streams batches into one table it zeroed once.  1 <= T <= 16, any S >= 1, B*S*S <= 2^40 per call.
 * 16-byte mask loads where S*S % 4 == 0, mask is 16-byte and label 4-byte aligned; one pixel per thread otherwise.  One 64-bit
 * integer atomic add per workgroup and counter (integer: bit-identical from run to run, also with "deterministic" = 1, which
 * forbids fp32 atomics); no memsets, no host synchronisation. */
int w2e_mask_iou_counts(const float* mask, const uint8_t* label, const uint8_t* lut, float threshold, int batch, int classes,
                        int size, unsigned long long* counts, void* stream);

/* ---- K12e: the style branch of FullSpaceMapperFEATClusterLinStyle_Net (attention/run_attention.py:811-828; csrc/region_style.hip) ----
 * A grouped, rectangular EqualLinear family: `groups` (<= 32) independent layers on `batch` (<= 16) rows, one launch per direction.
 * Group c maps one or two row-major sources -- src0[c] [batch, k0[c]] with row stride ld0[c], src1[c] [batch, k1[c]] with row stride
 * ld1[c] (k1[c] = 0: no second source) -- contracted as if concatenated, through the weight AS STORED, w[c] [n[c], k0[c] + k1[c]]
 * (model.py:130-164: row o = output feature o).  Everything per group goes by HOST arrays (device pointers, dimensions, w_scale[c] =
 * that layer's EqualLinear scale, act[c] = 0 none / 1 fused LeakyReLU, slope 0.2, gain sqrt 2), so groups of one launch may come from
 * different module families (mapper_c and mapper_text_c[0], :811 / :814), share a source (x_text) or point into packed buffers.
 * k0 >= 1, k1 >= 0, n >= 1, k0 + k1 and n at most 4096; every width has a tail path (16-byte accesses where all widths and strides of
 * a launch are multiples of 4 and all pointers 16-byte aligned).  b_scale = lr_mul.  fp32 FMA, fixed summation order, no atomics.
 *   rstyle_linear_fwd    out[c][m, o] = act(w_scale * sum_k a[m, k] W[o, k] + b_scale * bias[c][o])    (bias, or bias[c], may be NULL)
 *   rstyle_linear_dgrad  gx[m, i] = w_scale * sum_o gpre[m, o] W[o, i],  gpre = gy .* act'(y)  (y[c] = the layer's output; unread
 *                        where act[c] = 0); columns i < k0 go to gx0[c] [batch, k0], the others to gx1[c] [batch, k1]; a NULL entry is
 *                        a gradient nobody needs and is not computed (not both).  gpre is staged in LDS: batch * max n + 256 * MB <= 16384
 *                        floats, MB = batch rounded up to a power of two.
 *   rstyle_linear_wgrad  gw[c] = w_scale * gpre^T a  [n, k0 + k1],  gb[c] = b_scale * column sums of gpre (gb, or gb[c], may be NULL);
 *                        WRITTEN, not accumulated.
 * The finish (:820-821), per code c of width dims[c]; x[c] [batch, dims[c]] is read in place with row stride ldx[c]:
 *   rstyle_finish_fwd    diff = alpha * (y - x);  x_new[c] = x + diff;  norms[c * batch + m] = ||diff[m, :]||_2;
 *                        loss_delta[0] = sum_c mean_m norms[c, m] / layers     (two kernels; norms: groups * batch floats)
 *   rstyle_finish_bwd    gy[c][m, j] = alpha * (g_out[c][m, j] + g_loss[0] * diff[m, j] / norms[c, m] / (batch * layers)); a row with
 *                        norms == 0 takes 0 from the norm term (as torch's norm backward does; never NaN).  g_out[c] NULL = zeros;
 *                        g_loss (a device scalar) NULL = 0. */
int w2e_rstyle_linear_fwd(int groups, int batch, const float* const* src0, const float* const* src1, const int* k0, const int* k1,
                          const int* ld0, const int* ld1, const float* const* w, const float* const* bias, float* const* out,
                          const int* n, const float* w_scale, float b_scale, const int* act, void* stream);
int w2e_rstyle_linear_dgrad(int groups, int batch, const float* const* gy, const float* const* y, const float* const* w,
                            float* const* gx0, float* const* gx1, const int* k0, const int* k1, const int* n, const float* w_scale,
                            const int* act, void* stream);
int w2e_rstyle_linear_wgrad(int groups, int batch, const float* const* gy, const float* const* y, const float* const* src0,
                            const float* const* src1, const int* k0, const int* k1, const int* ld0, const int* ld1, float* const* gw,
                            float* const* gb, const int* n, const float* w_scale, float b_scale, const int* act, void* stream);
int w2e_rstyle_finish_fwd(int groups, int batch, const float* const* x, const int* ldx, const float* const* y, float* const* x_new,
                          const int* dims, float alpha, int layers, float* norms, float* loss_delta, void* stream);
int w2e_rstyle_finish_bwd(int groups, int batch, const float* const* x, const int* ldx, const float* const* y,
                          const float* const* g_out, const float* norms, const float* g_loss, float* const* gy, const int* dims,
                          float alpha, int layers, void* stream);

#ifdef __cplusplus
}
#endif
#endif
