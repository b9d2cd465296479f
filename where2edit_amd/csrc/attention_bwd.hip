// Backward of the region-attention mask branch (include/w2e_attention.h): w2e_cluster_pool_bwd and w2e_attention_logits_bwd, the
// opt-in path behind run_attention.train_mask_branch.  fp32 VALU, no atomics, no memsets; every reduction has a fixed tree (lanes ->
// wave shuffles -> wave partials in LDS added in wave order -> tiles / samples added in index order), so two runs are bit-identical.
//
// The forward saved the 32 conv sums of every (source, pixel) (`pre`, 9.4 MB per sample at the shipped shapes), so the cached
// activations -- the expensive, strided gather from maps of up to 1024^2 -- are read exactly once per backward, by the contraction
// G[b,i,o] = sum_p feat[b,i,src(p)] * g_m[b,o,p].  Re-evaluating the sums instead would read every activation twice.
#include "../../include/w2e_attention.h"
#include "device.h"

namespace w2e {

constexpr float SQRT2 = 1.4142135623730951f;
constexpr int TILE_VALS = 97;  // per (source, sample, 256-pixel tile): g_lcoef[32], g_bias[32], g_demod[32], g_noise_w

struct AttBwdLaunch {
    w2e_att_source src[W2E_ATT_MAX_SOURCES];
    w2e_att_source_grad grad[W2E_ATT_MAX_SOURCES];
    int chan_off[W2E_ATT_MAX_SOURCES];
    const float *wlast, *s_last, *d_last, *bias_last, *noise_last, *nw_last, *partial, *pre, *each, *g_each;
    float *g_wlast, *g_s_last, *g_scalars;
    float *gz, *headp, *gm, *tilep, *gdd, *G;  // workspace slices
    int n_sources, batch, size, tiles, sum_channels;
};

// ---------------------------------------------------------------------------------------- head: g_each -> g_Z
// One workgroup per sample.  each = sigmoid(u), u = lrelu(v) * sqrt2 + initial_bias, v = Z * d_last + nw_last * noise_last + bias_last,
// Z = sum_j partial_j.  Writes gz[b,p] = dL/dZ and the per-sample sums {g_u, g_v, g_v * noise_last, g_v * Z}.
__global__ __launch_bounds__(256) void att_bwd_head_kernel(const AttBwdLaunch L) {
    __shared__ float red[4][4];
    const int b = blockIdx.x, npix = L.size * L.size;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float dl = L.d_last[b], bl = L.bias_last[0], nw = L.noise_last ? L.nw_last[0] : 0.f;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int p = threadIdx.x; p < npix; p += 256) {
        const int64_t e = (int64_t)b * npix + p;
        float z = 0.f;
        for (int j = 0; j < L.n_sources; ++j) z += L.partial[(int64_t)j * L.batch * npix + e];
        const float nl = L.noise_last ? L.noise_last[e] : 0.f;
        const float v = z * dl + (L.noise_last ? nw * nl : 0.f) + bl;
        const float ea = L.each[e];
        const float gu = L.g_each[e] * ea * (1.f - ea);
        const float gv = gu * SQRT2 * (v > 0.f ? 1.f : 0.2f);
        L.gz[e] = gv * dl;
        a0 += gu, a1 += gv, a2 += gv * nl, a3 += gv * z;
    }
    a0 = wave_sum(a0), a1 = wave_sum(a1), a2 = wave_sum(a2), a3 = wave_sum(a3);
    if (lane == 0) red[wave][0] = a0, red[wave][1] = a1, red[wave][2] = a2, red[wave][3] = a3;
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        L.headp[b * 4 + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

// ---------------------------------------------------------------------------------------- per-pixel: g_Z -> g_m
// grid (256-pixel tiles, batch, source); a thread owns a pixel and the 32 outputs of its source, as in the forward.  From the saved
// sums m: pre = m * d + nw * noise + bias, a = lrelu(pre) * sqrt2, g_a = g_Z * lcoef, g_pre = g_a * sqrt2 * slope, g_m = g_pre * d.
// Writes g_m [j][b][o][p] and the tile's sums of g_Z * a (-> g_lcoef), g_pre (-> g_bias), g_pre * m (-> g_demod), g_pre * noise.
__global__ __launch_bounds__(256) void att_bwd_pixel_kernel(const AttBwdLaunch L) {
    __shared__ float dcoef[32], bcoef[32], lcoef[32];
    __shared__ float red[4][TILE_VALS];
    const int j = blockIdx.z, b = blockIdx.y, size = L.size, npix = size * size;
    const w2e_att_source& s = L.src[j];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const bool live = pix < npix;
    if (threadIdx.x < 32) {
        dcoef[threadIdx.x] = s.demod[b * 32 + threadIdx.x];
        bcoef[threadIdx.x] = s.bias[threadIdx.x];
        lcoef[threadIdx.x] = L.wlast[j * 32 + threadIdx.x] * L.s_last[(int64_t)b * 32 * L.n_sources + j * 32 + threadIdx.x];
    }
    __syncthreads();
    const float gz = live ? L.gz[(int64_t)b * npix + pix] : 0.f;
    const float nr = (s.noise && live) ? s.noise[(int64_t)b * npix + pix] : 0.f;
    const float nz = s.noise ? s.noise_w[0] * nr : 0.f;
    const int64_t base = ((int64_t)j * L.batch + b) * 32 * npix + (live ? pix : 0);
    float gsum = 0.f;
#pragma unroll 4
    for (int o = 0; o < 32; ++o) {
        const float m = live ? L.pre[base + (int64_t)o * npix] : 0.f;
        const float pre = m * dcoef[o] + nz + bcoef[o];
        const float a = (pre > 0.f ? pre : 0.2f * pre) * SQRT2;
        const float gpre = gz * lcoef[o] * SQRT2 * (pre > 0.f ? 1.f : 0.2f);
        if (live) L.gm[base + (int64_t)o * npix] = gpre * dcoef[o];
        gsum += gpre;
        const float r0 = wave_sum(gz * a), r1 = wave_sum(gpre), r2 = wave_sum(gpre * m);
        if (lane == 0) red[wave][o] = r0, red[wave][32 + o] = r1, red[wave][64 + o] = r2;
    }
    const float r3 = wave_sum(gsum * nr);
    if (lane == 0) red[wave][96] = r3;
    __syncthreads();
    if (threadIdx.x < TILE_VALS) {
        const int q = threadIdx.x;
        L.tilep[(((int64_t)j * L.batch + b) * L.tiles + blockIdx.x) * TILE_VALS + q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
    }
}

// ---------------------------------------------------------------------------------------- small sums: tiles, samples, the last conv
// One workgroup per source j: joins the tile sums in index order and finishes everything that is [B,32]-sized:
//   gdd[j,b,o] = -g_demod * d^3 (the factor of the demodulation path), g_bias_j, g_noise_w_j, the source's 32-slice of g_wlast and
//   g_s_last (lcoef = wlast * s_last, and d_last = rsqrt(sum (wlast * s_last)^2 + eps));  workgroup 0 also writes the three scalars.
__global__ __launch_bounds__(256) void att_bwd_small_kernel(const AttBwdLaunch L) {
    const int j = blockIdx.x, B = L.batch, T = L.tiles, n32 = 32 * L.n_sources;
    const w2e_att_source& s = L.src[j];
    auto tile_sum = [&](int b, int q) {
        const float* t = L.tilep + ((int64_t)j * B + b) * T * TILE_VALS + q;
        float acc = 0.f;
        for (int k = 0; k < T; ++k) acc += t[(int64_t)k * TILE_VALS];
        return acc;
    };
    for (int idx = threadIdx.x; idx < B * 32; idx += 256) {
        const int b = idx >> 5, o = idx & 31, c = j * 32 + o;
        const float glc = tile_sum(b, o), gd = tile_sum(b, 64 + o);
        const float d = s.demod[b * 32 + o];
        L.gdd[((int64_t)j * B + b) * 32 + o] = -gd * d * d * d;
        const float wl = L.wlast[c], sl = L.s_last[(int64_t)b * n32 + c], dl = L.d_last[b];
        const float gdl = -L.headp[b * 4 + 3] * dl * dl * dl;
        L.g_s_last[(int64_t)b * n32 + c] = glc * wl + gdl * wl * wl * sl;
    }
    if (threadIdx.x < 32) {
        const int o = threadIdx.x, c = j * 32 + o;
        const float wl = L.wlast[c];
        float gw = 0.f, gb = 0.f;
        for (int b = 0; b < B; ++b) {
            const float sl = L.s_last[(int64_t)b * n32 + c], dl = L.d_last[b];
            const float gdl = -L.headp[b * 4 + 3] * dl * dl * dl;
            gw += tile_sum(b, o) * sl + gdl * wl * sl * sl;
            gb += tile_sum(b, 32 + o);
        }
        L.g_wlast[c] = gw;
        L.grad[j].g_bias[o] = gb;
    } else if (threadIdx.x == 64) {
        float g = 0.f;
        for (int b = 0; b < B; ++b) g += tile_sum(b, 96);
        L.grad[j].g_noise_w[0] = g;
    } else if (threadIdx.x >= 128 && threadIdx.x < 131 && j == 0) {
        const int q = threadIdx.x - 128;  // 0: initial_bias (sum g_u), 1: bias_last (sum g_v), 2: nw_last (sum g_v * noise_last)
        float g = 0.f;
        for (int b = 0; b < B; ++b) g += L.headp[b * 4 + q];
        L.g_scalars[q] = g;
    }
}

// ---------------------------------------------------------------------------------------- the contraction over pixels
// G[b,i,o] = sum_p feat[b,i,src(p)] * g_m[b,o,p]: per (source, sample) a [C x P] x [P x 32] product whose left operand is gathered from
// the cached activation (one float per (res/size)^2 block when res > size, replicated pixels when res < size).
// grid (32-channel chunks, batch, source).  Per 128-pixel tile the workgroup stages feat^T [128][32] and g_m^T [128][32] in LDS (each thread
// issues 16 independent gather loads before its first store); wave w then owns pixels [32w, 32w+32) of the tile and lane (cg, og) a
// 4-channel x 4-output register block: two broadcast ds_read_b128 per 16 FMAs.  The four waves' blocks are added in wave order.
constexpr int CT_PIX = 128, CT_ROW = 36;  // 36-float rows: 16-byte aligned, rows of one store instruction land in different banks

__global__ __launch_bounds__(256) void att_bwd_contract_kernel(const AttBwdLaunch L) {
    __shared__ __attribute__((aligned(16))) float fT[CT_PIX * CT_ROW];
    __shared__ __attribute__((aligned(16))) float gT[CT_PIX * CT_ROW];
    const int j = blockIdx.z, b = blockIdx.y, c0 = blockIdx.x * 32;
    const w2e_att_source& s = L.src[j];
    const int C = s.channels, R = s.res, size = L.size, npix = size * size;
    if (c0 >= C) return;  // (uniform per workgroup)
    const int cn = (C - c0 < 32) ? C - c0 : 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cg = lane >> 3, og = lane & 7;
    const int pl = threadIdx.x & (CT_PIX - 1), half = threadIdx.x >> 7;
    const int64_t plane = (int64_t)R * R;
    const float scale = (float)R / (float)size;  // the forward's gather (att_source_kernel): torch's fp32 nearest index
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
    for (int p0 = 0; p0 < npix; p0 += CT_PIX) {
        const int pix = p0 + pl;
        const bool live = pix < npix;
        const int y = live ? pix / size : 0, x = live ? pix % size : 0;
        const int sy = nearest_src(y, scale, R), sx = nearest_src(x, scale, R);
        const float* f = s.feat + ((int64_t)b * C + c0 + half * 16) * plane + (int64_t)sy * R + sx;
        const float* g = L.gm + (((int64_t)j * L.batch + b) * 32 + half * 16) * npix + (live ? pix : 0);
        float fv[16], gv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) fv[u] = (live && half * 16 + u < cn) ? f[(int64_t)u * plane] : 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) gv[u] = live ? g[(int64_t)u * npix] : 0.f;
        __syncthreads();  // the previous tile's reads are done
        float4* fr = reinterpret_cast<float4*>(fT + pl * CT_ROW + half * 16);
        float4* gr = reinterpret_cast<float4*>(gT + pl * CT_ROW + half * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            fr[q] = make_float4(fv[4 * q], fv[4 * q + 1], fv[4 * q + 2], fv[4 * q + 3]);
            gr[q] = make_float4(gv[4 * q], gv[4 * q + 1], gv[4 * q + 2], gv[4 * q + 3]);
        }
        __syncthreads();
#pragma unroll 8
        for (int q = 0; q < 32; ++q) {
            const int row = (wave * 32 + q) * CT_ROW;
            const float4 f4 = *reinterpret_cast<const float4*>(fT + row + cg * 4);
            const float4 g4 = *reinterpret_cast<const float4*>(gT + row + og * 4);
            const float fa[4] = {f4.x, f4.y, f4.z, f4.w}, ga[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[a][c] += fa[a] * ga[c];
        }
    }
    __syncthreads();
    float* red = fT;  // [4 waves][32 channels][32 outputs] = 4096 floats <= CT_PIX * CT_ROW
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) red[wave * 1024 + (cg * 4 + a) * 32 + og * 4 + c] = acc[a][c];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = threadIdx.x * 4 + u, i = e >> 5, o = e & 31;
        const float t = (red[e] + red[1024 + e]) + (red[2048 + e] + red[3072 + e]);
        if (i < cn) L.G[((int64_t)b * L.sum_channels + L.chan_off[j] + c0 + i) * 32 + o] = t;
    }
}

// ---------------------------------------------------------------------------------------- weights and styles
// grid (8-channel groups, source); thread = (channel i, output o).  m = sum_i wscaled[i,o] * style[b,i] * feat, d = rsqrt(sum_i
// (wscaled * style)^2 + eps), so with gdd = -g_demod * d^3:
//   g_wscaled[i,o] = sum_b style[b,i] * G[b,i,o] + gdd[b,o] * wscaled[i,o] * style[b,i]^2
//   g_style[b,i]   = sum_o wscaled[i,o] * G[b,i,o] + gdd[b,o] * wscaled[i,o]^2 * style[b,i]      (32-lane butterfly: fixed order)
__global__ __launch_bounds__(256) void att_bwd_weight_kernel(const AttBwdLaunch L) {
    const int j = blockIdx.y;
    const w2e_att_source& s = L.src[j];
    const int C = s.channels, B = L.batch;
    const int i = blockIdx.x * 8 + (threadIdx.x >> 5), o = threadIdx.x & 31;
    if (blockIdx.x * 8 >= C) return;  // (uniform per workgroup)
    const bool live = i < C;           // (uniform per 32-lane group: the butterfly below never mixes channels)
    const float w = live ? s.wscaled[(int64_t)i * 32 + o] : 0.f;
    float gw = 0.f;
    for (int b = 0; b < B; ++b) {
        const float Gv = live ? L.G[((int64_t)b * L.sum_channels + L.chan_off[j] + i) * 32 + o] : 0.f;
        const float st = live ? s.style[(int64_t)b * C + i] : 0.f;
        const float gdd = L.gdd[((int64_t)j * B + b) * 32 + o];
        gw += st * Gv + gdd * w * st * st;
        float t = w * Gv + gdd * w * w * st;
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if (live && o == 0) L.grad[j].g_style[(int64_t)b * C + i] = t;
    }
    if (live) L.grad[j].g_wscaled[(int64_t)i * 32 + o] = gw;
}

// ---------------------------------------------------------------------------------------- cluster pooling, backward
// One workgroup per sample, the reduction tree of cluster_pool_kernel.  The adjoint of the reflect-padded gaussian gathers, for every
// input position, the output positions whose taps read it: directly (y' = y - d), folded at the low border (y' + d = -y) and folded at
// the high border (y' + d = 2 size - 2 - y).
__global__ __launch_bounds__(256) void cluster_pool_bwd_kernel(const float* __restrict__ g_final, const float* __restrict__ each,
                                                               const float* __restrict__ same, const float* __restrict__ means,
                                                               const float* __restrict__ counts, const int32_t* __restrict__ assign,
                                                               const float* __restrict__ g_loss_reg, const float* __restrict__ g_loss_tv,
                                                               float* __restrict__ g_each, int batch, int size, int csize, int K) {
    extern __shared__ float lds[];  // [size*size] x 2
    __shared__ float part[4];
    __shared__ float kgrad[32];
    const int b = blockIdx.x, npix = size * size;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* a = assign + (int64_t)b * csize * csize;
    const float scale = (float)csize / (float)size;
    auto cluster_of = [&](int p) {
        const int y = p / size, x = p % size;
        return a[nearest_src(y, scale, csize) * csize + nearest_src(x, scale, csize)];
    };
    float* ga = lds;
    float* gb = lds + npix;
    for (int p = threadIdx.x; p < npix; p += 256) ga[p] = g_final ? g_final[(int64_t)b * npix + p] : 0.f;
    __syncthreads();
    const float g0 = 1.f, g1 = expf(-0.5f * (1.f / 1.1f) * (1.f / 1.1f)), g2 = expf(-0.5f * (2.f / 1.1f) * (2.f / 1.1f));
    const float gs = g0 + 2.f * g1 + 2.f * g2;
    const float kk[3] = {g0 / gs, g1 / gs, g2 / gs};
    // adjoint along one axis: `at(t)` reads position t of the line, `c` is the input position
    auto adjoint = [&](auto at, int c) {
        float acc = 0.f;
#pragma unroll
        for (int d = -2; d <= 2; ++d) {
            const float kd = kk[d < 0 ? -d : d];
            int t = c - d;
            if (t >= 0 && t < size) acc += kd * at(t);
            t = -c - d;
            if (c >= 1 && t >= 0 && t < size) acc += kd * at(t);
            t = 2 * size - 2 - c - d;
            if (c <= size - 2 && t >= 0 && t < size) acc += kd * at(t);
        }
        return acc;
    };
    for (int p = threadIdx.x; p < npix; p += 256) {  // the forward's second pass (columns) first
        const int y = p / size, x = p % size;
        gb[p] = adjoint([&](int t) { return ga[t * size + x]; }, y);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < npix; p += 256) {
        const int y = p / size, x = p % size;
        const int k = cluster_of(p);
        const float v = adjoint([&](int t) { return gb[y * size + t]; }, x);
        ga[p] = (k >= 0 && k < K) ? v : 0.f;  // an out-of-range id holds the constant 1: nothing passes
    }
    __syncthreads();
    const float greg = g_loss_reg ? g_loss_reg[0] / (float)batch : 0.f;
    for (int k = 0; k < K; ++k) {
        float sg = 0.f;
        for (int p = threadIdx.x; p < npix; p += 256)
            if (cluster_of(p) == k) sg += ga[p];
        sg = wave_sum(sg);
        if (lane == 0) part[wave] = sg;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float n = counts[b * K + k], m = means[b * K + k];
            const float gm = (part[0] + part[1]) + (part[2] + part[3]) + ((n > 0.f && m > 0.7f) ? greg : 0.f);
            kgrad[k] = n > 0.f ? gm / n : 0.f;
        }
        __syncthreads();
    }
    const float gtv = g_loss_tv ? g_loss_tv[0] * 2.f / ((float)batch * (float)npix) : 0.f;
    for (int p = threadIdx.x; p < npix; p += 256) {
        const int k = cluster_of(p);
        const int64_t e = (int64_t)b * npix + p;
        g_each[e] = ((k >= 0 && k < K) ? kgrad[k] : 0.f) + gtv * (each[e] - same[e]);
    }
}

}  // namespace w2e

using namespace w2e;

extern "C" int w2e_attention_logits_bwd(const w2e_att_source* sources, const w2e_att_source_grad* grads, int n_sources,
                                        const float* wlast, const float* s_last, const float* d_last, const float* bias_last,
                                        const float* noise_last, const float* nw_last, const float* partial, const float* pre,
                                        const float* each, const float* g_each, float* g_wlast, float* g_s_last, float* g_scalars,
                                        float* workspace, int64_t workspace_floats, int batch, int size, void* stream) {
    W2E_REQUIRE(sources && grads && wlast && s_last && d_last && bias_last && partial && pre && each && g_each,
                "attention_logits_bwd: null input tensor");
    W2E_REQUIRE(g_wlast && g_s_last && g_scalars && workspace, "attention_logits_bwd: null output tensor");
    W2E_REQUIRE(n_sources >= 1 && n_sources <= W2E_ATT_MAX_SOURCES, "attention_logits_bwd: 1 <= n_sources <= %d", W2E_ATT_MAX_SOURCES);
    W2E_REQUIRE(batch >= 0 && batch < 65536 && size > 0 && size <= 4096, "attention_logits_bwd: bad dims");
    W2E_REQUIRE(!noise_last || nw_last, "attention_logits_bwd: noise_last without nw_last");
    if (batch == 0) return 0;
    AttBwdLaunch L{};
    int sum_c = 0, max_c = 0;
    for (int j = 0; j < n_sources; ++j) {
        const w2e_att_source& s = sources[j];
        const w2e_att_source_grad& g = grads[j];
        W2E_REQUIRE(s.feat && s.wscaled && s.style && s.demod && s.bias, "attention_logits_bwd: source %d has a null tensor", j);
        W2E_REQUIRE(g.g_wscaled && g.g_style && g.g_bias && g.g_noise_w, "attention_logits_bwd: source %d has a null gradient", j);
        W2E_REQUIRE(s.channels > 0 && s.channels <= (1 << 20) && s.res > 0, "attention_logits_bwd: source %d: bad dims", j);
        W2E_REQUIRE(!s.noise || s.noise_w, "attention_logits_bwd: source %d: noise without noise_w", j);
        L.src[j] = s, L.grad[j] = g, L.chan_off[j] = sum_c;
        sum_c += s.channels;
        if (s.channels > max_c) max_c = s.channels;
    }
    const int npix = size * size, tiles = (int)ceil_div(npix, 256);
    const int64_t need = W2E_ATT_BWD_WORKSPACE(n_sources, batch, npix, sum_c);
    W2E_REQUIRE(workspace_floats >= need, "attention_logits_bwd: workspace of %lld floats, %lld needed", (long long)workspace_floats,
                (long long)need);
    L.wlast = wlast, L.s_last = s_last, L.d_last = d_last, L.bias_last = bias_last, L.noise_last = noise_last, L.nw_last = nw_last;
    L.partial = partial, L.pre = pre, L.each = each, L.g_each = g_each;
    L.g_wlast = g_wlast, L.g_s_last = g_s_last, L.g_scalars = g_scalars;
    float* w = workspace;
    L.gz = w, w += (int64_t)batch * npix;
    L.headp = w, w += 4 * (int64_t)batch;
    L.gm = w, w += (int64_t)n_sources * batch * 32 * npix;
    L.tilep = w, w += (int64_t)n_sources * batch * tiles * TILE_VALS;
    L.gdd = w, w += (int64_t)n_sources * batch * 32;
    L.G = w;
    L.n_sources = n_sources, L.batch = batch, L.size = size, L.tiles = tiles, L.sum_channels = sum_c;
    hipStream_t st = (hipStream_t)stream;
    att_bwd_head_kernel<<<(unsigned)batch, 256, 0, st>>>(L);
    W2E_LAUNCH_CHECK("attention_logits_bwd (head)");
    att_bwd_pixel_kernel<<<dim3((unsigned)tiles, (unsigned)batch, (unsigned)n_sources), 256, 0, st>>>(L);
    W2E_LAUNCH_CHECK("attention_logits_bwd (pixels)");
    att_bwd_small_kernel<<<(unsigned)n_sources, 256, 0, st>>>(L);
    W2E_LAUNCH_CHECK("attention_logits_bwd (small sums)");
    att_bwd_contract_kernel<<<dim3((unsigned)ceil_div(max_c, 32), (unsigned)batch, (unsigned)n_sources), 256, 0, st>>>(L);
    W2E_LAUNCH_CHECK("attention_logits_bwd (contraction)");
    att_bwd_weight_kernel<<<dim3((unsigned)ceil_div(max_c, 8), (unsigned)n_sources), 256, 0, st>>>(L);
    W2E_LAUNCH_CHECK("attention_logits_bwd (weights)");
    return 0;
}

extern "C" int w2e_cluster_pool_bwd(const float* g_final, const float* each, const float* same, const float* means,
                                    const float* counts, const int32_t* assign, const float* g_loss_reg, const float* g_loss_tv,
                                    float* g_each, int batch, int size, int csize, int clusters, void* stream) {
    W2E_REQUIRE(each && same && means && counts && assign && g_each, "cluster_pool_bwd: null tensor");
    W2E_REQUIRE(batch >= 0 && size >= 3 && size <= 128 && csize > 0, "cluster_pool_bwd: 3 <= size <= 128 (got %d)", size);
    W2E_REQUIRE(clusters >= 1 && clusters <= 32, "cluster_pool_bwd: 1 <= clusters <= 32 (got %d)", clusters);
    if (batch == 0) return 0;
    const size_t lds = sizeof(float) * 2 * (size_t)size * size;
    static unsigned done = 0;
    // (128 KB at size 128: see w2e_cluster_pool)
    if (lds > 64 * 1024) W2E_REQUIRE(big_lds_once((const void*)cluster_pool_bwd_kernel, &done, 128 * 1024), "cluster_pool_bwd: LDS opt-in failed");
    cluster_pool_bwd_kernel<<<batch, 256, lds, (hipStream_t)stream>>>(g_final, each, same, means, counts, assign, g_loss_reg, g_loss_tv,
                                                                     g_each, batch, size, csize, clusters);
    W2E_LAUNCH_CHECK("cluster_pool_bwd");
    return 0;
}
