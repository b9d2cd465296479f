// The LPIPS head (include/w2e_lpips.h): per pixel, unit-normalise two feature vectors across channels, take the lin-weighted squared
// difference, average over pixels -- and the adjoint.  Both kernels are memory-bound.
//
// Geometry (both kernels): features are NCHW, so adjacent lanes take adjacent pixels (float4 groups of four where pixels % 4 == 0)
// and walk the channels.  A workgroup of 256 threads is PX pixel lanes x G = 256 / PX channel groups: thread (px, g) walks channels
// g, g + G, ...  The partial sums over channels meet in LDS and every thread adds the G partials of its pixel in the same fixed
// order.  PX shrinks with the tap: 64 lanes x 4 groups on the large shallow taps, 16 x 16 in the middle, 4 x 64 on the deep taps
// (14 x 14 or 1 x 1 pixels, 512 channels), where one lane would otherwise walk 512 strided loads alone.  PX depends on (pixels)
// only, so a result does not depend on the batch it was computed in.
//
// The norms have to be known before the difference can be formed (the expansion that would avoid this cancels: w2e_lpips.h), so a
// tile is read twice in the forward and three times in the backward.  The second and third reads repeat, per thread, the addresses
// of the first within the same workgroup a few microseconds later: a tile is at most 64 * 4 pixels * 512 channels * 2 tensors * 4 B
// = 1 MiB, and comes back from L2 / MALL, not from HBM.
#include "../../include/w2e_lpips.h"
#include "device.h"

namespace w2e {

constexpr int LP_BLOCK = 256;
constexpr float LP_EPS = 1e-10f;

template <int VEC>
__device__ __forceinline__ void lp_load(const float* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int VEC>
__device__ __forceinline__ void lp_store(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *p = v[0];
    }
}

// u0 - u1 with u = f / a: two correctly rounded quotients and one subtraction.  A quotient, not f * (1 / a): the rounding error of
// the reciprocal is the same for every channel of a pixel, so it adds a multiple of u itself to u0 - u1 -- against near-equal inputs
// (|u0 - u1| ~ 0.01 |u|) that is 6e-6 of the difference, all in one direction, and it showed in the gradient (1.5e-5 from float64
// at 512 x 2 x 2 where the fp32 closed form on the CPU is 5e-6 away).  Contraction is off so that nothing fuses into the
// subtraction: identical inputs must give exactly 0.
__device__ __forceinline__ float lp_diff(float f0, float a0, float f1, float a1) {
#pragma clang fp contract(off)
    const float u0 = f0 / a0;
    const float u1 = f1 / a1;
    return u0 - u1;
}

__device__ __forceinline__ float lp_block_sum(float v, float* sm) {  // fixed order; valid in thread 0
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    return r;
}

// The G partials of this thread's pixel, added in the order g = 0, 1, ..., G - 1 by every thread of the pixel alike.
template <int VEC>
__device__ __forceinline__ void lp_group_sum(const float (*sn)[VEC], int px, int px_log2, float (&out)[VEC]) {
    const int groups = LP_BLOCK >> px_log2;
#pragma unroll
    for (int v = 0; v < VEC; ++v) out[v] = 0.f;
    for (int g = 0; g < groups; ++g) {
        const float* row = sn[(g << px_log2) + px];
#pragma unroll
        for (int v = 0; v < VEC; ++v) out[v] += row[v];
    }
}

// Squared norms of both feature vectors of this thread's VEC pixels: partials over the thread's channels into LDS, then the fixed-order
// sum.  Ends with every thread holding nsq0 / nsq1 of its pixels; the LDS arrays are free again after the trailing barrier.
template <int VEC>
__device__ __forceinline__ void lp_norms(const float* __restrict__ p0, const float* __restrict__ p1, bool active, int C, int64_t P, int g,
                                         int groups, int px, int px_log2, float (*sn0)[VEC], float (*sn1)[VEC], float (&nsq0)[VEC],
                                         float (&nsq1)[VEC]) {
    float s0[VEC], s1[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) s0[v] = s1[v] = 0.f;
    if (active) {
        for (int c = g; c < C; c += groups) {
            float a[VEC], b[VEC];
            lp_load<VEC>(p0 + c * P, a);
            lp_load<VEC>(p1 + c * P, b);
            // explicit FMAs: both sides round alike whatever the compiler packs, so identical inputs have identical norms
#pragma unroll
            for (int v = 0; v < VEC; ++v) s0[v] = __fmaf_rn(a[v], a[v], s0[v]), s1[v] = __fmaf_rn(b[v], b[v], s1[v]);
        }
    }
#pragma unroll
    for (int v = 0; v < VEC; ++v) sn0[threadIdx.x][v] = s0[v], sn1[threadIdx.x][v] = s1[v];
    __syncthreads();
    lp_group_sum<VEC>(sn0, px, px_log2, nsq0);
    lp_group_sum<VEC>(sn1, px, px_log2, nsq1);
    __syncthreads();
}

// grid (blocks per image, batch).  Every block adds its tiles tile = blockIdx.x, + gridDim.x, ... and leaves the sum in
// partials[blockIdx.y * gridDim.x + blockIdx.x].
template <int VEC>
__global__ __launch_bounds__(LP_BLOCK) void lpips_head_fwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                                   const float* __restrict__ lin, int C, int64_t P, int64_t groups_px,
                                                                   int px_log2, int64_t tiles, int bcast, float* __restrict__ partials) {
    __shared__ float sn0[LP_BLOCK][VEC], sn1[LP_BLOCK][VEC];
    __shared__ float sm[LP_BLOCK / 64];
    const int px = threadIdx.x & ((1 << px_log2) - 1), g = threadIdx.x >> px_log2, groups = LP_BLOCK >> px_log2;
    const int b = blockIdx.y;
    const float* img0 = f0 + (int64_t)b * C * P;
    const float* img1 = f1 + (bcast ? 0 : (int64_t)b * C * P);
    float acc = 0.f;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t pg = (tile << px_log2) + px;
        const bool active = pg < groups_px;
        const float* p0 = img0 + pg * VEC;
        const float* p1 = img1 + pg * VEC;
        float nsq0[VEC], nsq1[VEC];
        lp_norms<VEC>(p0, p1, active, C, P, g, groups, px, px_log2, sn0, sn1, nsq0, nsq1);
        if (active) {
            float a0[VEC], a1[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) a0[v] = sqrtf(nsq0[v]) + LP_EPS, a1[v] = sqrtf(nsq1[v]) + LP_EPS;
            for (int c = g; c < C; c += groups) {
                float a[VEC], bb[VEC];
                lp_load<VEC>(p0 + c * P, a);
                lp_load<VEC>(p1 + c * P, bb);
                const float w = lin[c];
                float t = 0.f;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float e = lp_diff(a[v], a0[v], bb[v], a1[v]);
                    t += e * e;
                }
                acc += w * t;
            }
        }
    }
    const float s = lp_block_sum(acc, sm);
    if (threadIdx.x == 0) partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// One block per image: the image's partials in a fixed order, times 1 / pixels.
__global__ __launch_bounds__(LP_BLOCK) void lpips_head_final_kernel(const float* __restrict__ partials, int per_image, float inv_pixels,
                                                                     float* __restrict__ out) {
    __shared__ float sm[LP_BLOCK / 64];
    const float* p = partials + (int64_t)blockIdx.x * per_image;
    float acc = 0.f;
    for (int i = threadIdx.x; i < per_image; i += LP_BLOCK) acc += p[i];
    const float s = lp_block_sum(acc, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = s * inv_pixels;
}

// grid (blocks per image, batch); no reduction leaves the block.
template <int VEC>
__global__ __launch_bounds__(LP_BLOCK) void lpips_head_bwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1,
                                                                   const float* __restrict__ lin, const float* __restrict__ gout, int C,
                                                                   int64_t P, int64_t groups_px, int px_log2, int64_t tiles, int bcast,
                                                                   float two_over_pixels, float* __restrict__ g0, float* __restrict__ g1,
                                                                   int accumulate, int relu) {
    __shared__ float sn0[LP_BLOCK][VEC], sn1[LP_BLOCK][VEC];
    const int px = threadIdx.x & ((1 << px_log2) - 1), g = threadIdx.x >> px_log2, groups = LP_BLOCK >> px_log2;
    const int b = blockIdx.y;
    const int64_t off0 = (int64_t)b * C * P;
    const float* img0 = f0 + off0;
    const float* img1 = f1 + (bcast ? 0 : off0);
    const float k2 = gout[b] * two_over_pixels;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t pg = (tile << px_log2) + px;
        const bool active = pg < groups_px;
        const float* p0 = img0 + pg * VEC;
        const float* p1 = img1 + pg * VEC;
        float nsq0[VEC], nsq1[VEC];
        lp_norms<VEC>(p0, p1, active, C, P, g, groups, px, px_log2, sn0, sn1, nsq0, nsq1);
        float a0[VEC], a1[VEC], i0[VEC], i1[VEC], r0[VEC], r1[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float n0 = sqrtf(nsq0[v]), n1 = sqrtf(nsq1[v]);
            a0[v] = n0 + LP_EPS, a1[v] = n1 + LP_EPS;
            i0[v] = 1.f / a0[v], i1[v] = 1.f / a1[v];  // (for q / a only: an error relative to the term, nothing it could cancel against)
            r0[v] = n0 > 0.f ? 1.f / (n0 * a0[v] * a0[v]) : 0.f;  // the zero-norm convention (w2e_lpips.h)
            r1[v] = n1 > 0.f ? 1.f / (n1 * a1[v] * a1[v]) : 0.f;
        }
        // sum_c lin_c e_c f0_c and sum_c lin_c e_c f1_c (the factor 2 gout / pixels joins below)
        float s0[VEC], s1[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) s0[v] = s1[v] = 0.f;
        if (active) {
            for (int c = g; c < C; c += groups) {
                float a[VEC], bb[VEC];
                lp_load<VEC>(p0 + c * P, a);
                lp_load<VEC>(p1 + c * P, bb);
                const float w = lin[c];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float we = w * lp_diff(a[v], a0[v], bb[v], a1[v]);
                    s0[v] += we * a[v], s1[v] += we * bb[v];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) sn0[threadIdx.x][v] = s0[v], sn1[threadIdx.x][v] = s1[v];
        __syncthreads();
        lp_group_sum<VEC>(sn0, px, px_log2, s0);
        lp_group_sum<VEC>(sn1, px, px_log2, s1);
        __syncthreads();
        if (active) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) s0[v] *= k2 * r0[v], s1[v] *= k2 * r1[v];
            float* o0 = g0 + off0 + pg * VEC;
            float* o1 = g1 ? g1 + off0 + pg * VEC : nullptr;
            for (int c = g; c < C; c += groups) {
                float a[VEC], bb[VEC], d0[VEC], d1[VEC];
                lp_load<VEC>(p0 + c * P, a);
                lp_load<VEC>(p1 + c * P, bb);
                const float kw = k2 * lin[c];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const float q = kw * lp_diff(a[v], a0[v], bb[v], a1[v]);
                    d0[v] = q * i0[v] - a[v] * s0[v];
                    d1[v] = bb[v] * s1[v] - q * i1[v];
                }
                if (accumulate) {
                    float old[VEC];
                    lp_load<VEC>(o0 + c * P, old);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) d0[v] += old[v];
                }
                if (relu) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) d0[v] = a[v] > 0.f ? d0[v] : 0.f;
                }
                lp_store<VEC>(o0 + c * P, d0);
                if (o1) {
                    if (accumulate) {
                        float old[VEC];
                        lp_load<VEC>(o1 + c * P, old);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) d1[v] += old[v];
                    }
                    if (relu) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) d1[v] = bb[v] > 0.f ? d1[v] : 0.f;
                    }
                    lp_store<VEC>(o1 + c * P, d1);
                }
            }
        }
    }
}

// The tile geometry of one tap: VEC (4 where the rows stay 16-byte aligned), the pixel lanes of a workgroup and the tile count.
struct LpGeometry {
    int vec, px_log2;
    int64_t groups_px, tiles;
};

static LpGeometry lp_geometry(int64_t pixels, bool aligned16) {
    LpGeometry q;
    q.vec = ((pixels & 3) == 0 && aligned16) ? 4 : 1;
    q.groups_px = pixels / q.vec;
    q.px_log2 = q.groups_px >= 4096 ? 6 : q.groups_px >= 64 ? 4 : 2;
    q.tiles = ceil_div(q.groups_px, (int64_t)1 << q.px_log2);
    return q;
}

static bool lp_aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0);
}

}  // namespace w2e

using namespace w2e;

extern "C" int w2e_lpips_head_fwd(const float* f0, const float* f1, const float* lin, int batch, int batch1, int channels, int64_t pixels,
                                  float* partials, int n_partials, float* out, void* stream) {
    W2E_REQUIRE(f0 && f1 && lin && partials && out, "lpips_head_fwd: null tensor");
    W2E_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 1 && pixels >= 1, "lpips_head_fwd: bad size (batch %d, channels %d, pixels %lld)",
                batch, channels, (long long)pixels);
    W2E_REQUIRE(batch1 == batch || batch1 == 1, "lpips_head_fwd: the second batch %d is neither %d nor 1", batch1, batch);
    W2E_REQUIRE((int64_t)n_partials >= (int64_t)batch * W2E_LPIPS_PARTIALS, "lpips_head_fwd: the partials slab holds %d floats, needs %lld",
                n_partials, (long long)batch * W2E_LPIPS_PARTIALS);
    const LpGeometry q = lp_geometry(pixels, lp_aligned16(f0, f1, nullptr, nullptr));
    const int per_image = (int)std::min<int64_t>(q.tiles, W2E_LPIPS_PARTIALS);
    const int bcast = (batch1 == 1 && batch > 1) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(per_image, batch);
    if (q.vec == 4)
        lpips_head_fwd_kernel<4><<<grid, LP_BLOCK, 0, s>>>(f0, f1, lin, channels, pixels, q.groups_px, q.px_log2, q.tiles, bcast, partials);
    else
        lpips_head_fwd_kernel<1><<<grid, LP_BLOCK, 0, s>>>(f0, f1, lin, channels, pixels, q.groups_px, q.px_log2, q.tiles, bcast, partials);
    W2E_LAUNCH_CHECK("lpips_head_fwd");
    lpips_head_final_kernel<<<batch, LP_BLOCK, 0, s>>>(partials, per_image, (float)(1.0 / (double)pixels), out);
    W2E_LAUNCH_CHECK("lpips_head_fwd (final sum)");
    return 0;
}

extern "C" int w2e_lpips_head_bwd(const float* f0, const float* f1, const float* lin, const float* gout, int batch, int batch1, int channels,
                                  int64_t pixels, float* g0, float* g1, int accumulate, int relu, void* stream) {
    W2E_REQUIRE(f0 && f1 && lin && gout && g0, "lpips_head_bwd: null tensor");
    W2E_REQUIRE(batch >= 1 && batch <= 65535 && channels >= 1 && pixels >= 1, "lpips_head_bwd: bad size (batch %d, channels %d, pixels %lld)",
                batch, channels, (long long)pixels);
    W2E_REQUIRE(batch1 == batch || batch1 == 1, "lpips_head_bwd: the second batch %d is neither %d nor 1", batch1, batch);
    W2E_REQUIRE(!(g1 && batch1 != batch), "lpips_head_bwd: g1 (the second input's gradient) needs equal batches");
    const LpGeometry q = lp_geometry(pixels, lp_aligned16(f0, f1, g0, g1));
    const int per_image = (int)std::min<int64_t>(q.tiles, W2E_LPIPS_PARTIALS);  // (the forward's grid)
    const int bcast = (batch1 == 1 && batch > 1) ? 1 : 0;
    const float two_over_pixels = (float)(2.0 / (double)pixels);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(per_image, batch);
    if (q.vec == 4)
        lpips_head_bwd_kernel<4><<<grid, LP_BLOCK, 0, s>>>(f0, f1, lin, gout, channels, pixels, q.groups_px, q.px_log2, q.tiles, bcast,
                                                           two_over_pixels, g0, g1, accumulate ? 1 : 0, relu ? 1 : 0);
    else
        lpips_head_bwd_kernel<1><<<grid, LP_BLOCK, 0, s>>>(f0, f1, lin, gout, channels, pixels, q.groups_px, q.px_log2, q.tiles, bcast,
                                                           two_over_pixels, g0, g1, accumulate ? 1 : 0, relu ? 1 : 0);
    W2E_LAUNCH_CHECK("lpips_head_bwd");
    return 0;
}
