// Offline k-means on the up-sampled activations (include/w2e_attention.h, "offline k-means"): one persistent kernel in three
// modes -- assignment + min distance, the fused Lloyd step (assignment + per-cluster sums + counts + inertia in one launch), and
// the k-means++ seeding pass (distances to T candidates at once + the T potentials) -- and a fixed-order finish step.
//
// Shape of the pass.  300 x [1,512,128,128] points are 11 GB.  A workgroup is 8 waves and walks 128-pixel tiles: wave w owns the 64
// pixels of half w/4 and the channel quarter w%4, 16 channel planes' loads in flight (the training-time kernel of attention.hip
// launches 4 waves with 8 in flight, and its LDS use at K = 20, D = 576 admits one workgroup per CU; that more loads in flight
// buy bandwidth here is the design's expectation -- DESIGN.md K12c holds what was measured).  The distance arithmetic is
// the training-time kernel's, operation for operation (quarters accumulated in channel order, position channels after quarter 3,
// joined ((q0+q1)+q2)+q3, ties to the lowest k), so the assignment is bit-identical.
//
// Fused step.  Once a tile's 128 assignments are known the tile (128 px x C x 4 B = 256 KB at C = 512; 64 MB over 256 CUs, which
// is expected, not measured, to still sit in the 256 MB Infinity Cache) is read a second time with the roles turned: thread t
// owns feature dimension t (and t + 512), walks the 128 pixels in order with 16-byte loads and adds into its own column of the
// [K][D+1] running sums in LDS (last column: the count).  Each such wave-wide load touches 64 cache lines S*S*4 bytes apart and
// every 128-byte line is asked for by 8 loads: the price of one owner per column.  Consecutive pixels of one cluster are summed in
// a register and flushed when the cluster changes.  Pixels in order, no atomics: the result is a function of the data and the
// grid size only.
#include "../../include/w2e_attention.h"
#include "device.h"

namespace w2e {
namespace {

constexpr int KM_THREADS = 512;  // 8 waves: 2 pixel halves x 4 channel quarters
constexpr int KM_TILE = 128;     // pixels per tile
constexpr int KM_FLY = 16;       // channel planes in flight per wave

enum { KM_ASSIGN = 0, KM_STEP = 1, KM_SEED = 2 };

__host__ __device__ inline int64_t km_lds_floats(int D, int KP, int K, int mode, int slots = 6) {
    return (int64_t)D * KP + (int64_t)slots * 64 * KP + KM_TILE + 2 * KP + (mode == KM_STEP ? (int64_t)K * (D + 1) : 0);
}

// SLOTS: blocks of [64][KP] partial distances.  6: one per (half, quarter 1..3), the halves join at once.  3, for centres that leave no
// room for six (mode 0 only: D = 1024 at K = 32 is 128 KB of centres): the halves take turns at the same three blocks, at two more
// barriers per tile; the additions and their order are the same, so is every bit of the result.
template <int KP, int MODE, int SLOTS = 6>
__global__ __launch_bounds__(KM_THREADS) void kmeans_pass_kernel(const float* __restrict__ feat, const float* __restrict__ cen,
                                                                 int32_t* __restrict__ assign, float* __restrict__ mind,
                                                                 float* __restrict__ candd, int64_t cand_ld,
                                                                 float* __restrict__ partial, int C, int P, int S, int K,
                                                                 int n_tiles, int tiles_per_img) {
    extern __shared__ float lds[];  // [D][KP] centres | [SLOTS][64][KP] partial distances | [128] tile assignment | [2][KP] | [K][D+1] sums
    const int D = C + 2 * P, D1 = D + 1, npix = S * S;
    float* part = lds + D * KP;
    int* tk = reinterpret_cast<int*>(part + SLOTS * 64 * KP);
    float* red = reinterpret_cast<float*>(tk + KM_TILE);
    float* sums = red + 2 * KP;
    for (int e = threadIdx.x; e < D * KP; e += KM_THREADS) {
        const int d = e / KP, k = e % KP;
        lds[e] = k < K ? cen[(int64_t)k * D + d] : 0.f;
    }
    if (MODE == KM_STEP)
        for (int e = threadIdx.x; e < K * D1; e += KM_THREADS) sums[e] = 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = wave >> 2, q = wave & 3;
    constexpr int NT = MODE == KM_SEED ? KP : 1;
    float tot[NT];  // per-lane running inertia (or the T potentials), tiles in order
#pragma unroll
    for (int t = 0; t < NT; ++t) tot[t] = 0.f;
    const int c_lo = (C * q) >> 2, c_hi = (C * (q + 1)) >> 2;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int b = tile / tiles_per_img, px0 = (tile % tiles_per_img) * KM_TILE;
        const int pix = px0 + half * 64 + lane;
        const bool live = pix < npix;
        float dist[KP];
#pragma unroll
        for (int k = 0; k < KP; ++k) dist[k] = 0.f;
        const float* f = feat + (int64_t)b * C * npix + (live ? pix : 0);
        for (int c0 = c_lo; c0 < c_hi; c0 += KM_FLY) {
            float v16[KM_FLY];
#pragma unroll
            for (int u = 0; u < KM_FLY; ++u) v16[u] = (c0 + u < c_hi) ? f[(int64_t)(c0 + u) * npix] : 0.f;
#pragma unroll
            for (int u = 0; u < KM_FLY; ++u) {
                if (c0 + u >= c_hi) break;
                const float v = v16[u];
                const float4* row = reinterpret_cast<const float4*>(lds + (c0 + u) * KP);
#pragma unroll
                for (int j = 0; j < KP / 4; ++j) {
                    const float4 m = row[j];
                    float t;
                    t = v - m.x, dist[4 * j + 0] += t * t;
                    t = v - m.y, dist[4 * j + 1] += t * t;
                    t = v - m.z, dist[4 * j + 2] += t * t;
                    t = v - m.w, dist[4 * j + 3] += t * t;
                }
            }
        }
        if (q == 3) {
            const int y = pix / S, x = pix % S;
            const float xp = (float)x * 2.f / (float)(S - 1) - 1.f, yp = (float)y * 2.f / (float)(S - 1) - 1.f;
            for (int pc = 0; pc < 2 * P; ++pc) {
                const float v = pc < P ? xp : yp;
                const float* row = lds + (C + pc) * KP;
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    const float t = v - row[k];
                    dist[k] += t * t;
                }
            }
        }
        constexpr int TURNS = SLOTS == 6 ? 1 : 2;
#pragma unroll
        for (int turn = 0; turn < TURNS; ++turn) {
            const bool mine = SLOTS == 6 || half == turn;
            const int blk = SLOTS == 6 ? half * 3 : 0;
            if (q != 0 && mine) {
                float4* dst = reinterpret_cast<float4*>(part + ((blk + q - 1) * 64 + lane) * KP);
#pragma unroll
                for (int j = 0; j < KP / 4; ++j) dst[j] = make_float4(dist[4 * j], dist[4 * j + 1], dist[4 * j + 2], dist[4 * j + 3]);
            }
            __syncthreads();
            if (q == 0 && mine) {
                const float* p1 = part + ((blk + 0) * 64 + lane) * KP;
                const float* p2 = part + ((blk + 1) * 64 + lane) * KP;
                const float* p3 = part + ((blk + 2) * 64 + lane) * KP;
#pragma unroll
                for (int k = 0; k < KP; ++k) dist[k] = ((dist[k] + p1[k]) + p2[k]) + p3[k];
                if (MODE == KM_SEED) {
                    if (live) {
                        const int64_t n = (int64_t)b * npix + pix;
                        const float m = mind ? mind[n] : __builtin_inff();
#pragma unroll
                        for (int t = 0; t < KP; ++t)
                            if (t < K) {
                                candd[t * cand_ld + n] = dist[t];
                                tot[t] += fminf(m, dist[t]);
                            }
                    }
                } else {
                    int best = 0;
                    float bd = dist[0];
#pragma unroll
                    for (int k = 1; k < KP; ++k)
                        if (k < K && dist[k] < bd) bd = dist[k], best = k;
                    if (live) {
                        const int64_t n = (int64_t)b * npix + pix;
                        if (assign) assign[n] = best;
                        if (mind) mind[n] = bd;
                        tot[0] += bd;
                    }
                    tk[half * 64 + lane] = live ? best : -1;
                }
            }
            __syncthreads();  // (also: `part` is free again before a faster wave writes the next tile's partials)
        }
        if (MODE == KM_STEP) {
            for (int d = threadIdx.x; d <= D; d += KM_THREADS) {
                const float* row = feat + ((int64_t)b * C + (d < C ? d : 0)) * npix + px0;
                int cur = -1;
                float acc = 0.f;
                for (int g0 = 0; g0 < KM_TILE / 4; g0 += 8) {
                    float4 v8[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int p = px0 + 4 * (g0 + u);
                        if (d < C) {
                            v8[u] = p + 3 < npix ? *reinterpret_cast<const float4*>(row + 4 * (g0 + u)) : make_float4(0.f, 0.f, 0.f, 0.f);
                        } else {
                            float a[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int pp = p + j;
                                a[j] = d == D ? 1.f : (float)(d < C + P ? pp % S : pp / S) * 2.f / (float)(S - 1) - 1.f;
                            }
                            v8[u] = make_float4(a[0], a[1], a[2], a[3]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int4 kk = reinterpret_cast<const int4*>(tk)[g0 + u];
                        const int ks[4] = {kk.x, kk.y, kk.z, kk.w};
                        const float vs[4] = {v8[u].x, v8[u].y, v8[u].z, v8[u].w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int k = __builtin_amdgcn_readfirstlane(ks[j]);  // the same for every thread: the tile's pixel
                            if (k != cur) {
                                if (cur >= 0) sums[cur * D1 + d] += acc;
                                cur = k, acc = 0.f;
                            }
                            acc += vs[j];
                        }
                    }
                }
                if (cur >= 0) sums[cur * D1 + d] += acc;
            }
        }
    }
    __syncthreads();
    const int n_out = MODE == KM_STEP ? K * D1 + 1 : (MODE == KM_SEED ? K : 1);
    float* out = partial + (int64_t)blockIdx.x * n_out;
    if (MODE == KM_STEP)
        for (int e = threadIdx.x; e < K * D1; e += KM_THREADS) out[e] = sums[e];
    if (q == 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float s = wave_sum(tot[t]);
            if (lane == 0) red[half * KP + t] = s;
        }
    }
    __syncthreads();
    const int nt = MODE == KM_SEED ? K : 1;
    if ((int)threadIdx.x < nt) out[(MODE == KM_STEP ? K * D1 : 0) + threadIdx.x] = red[threadIdx.x] + red[KP + threadIdx.x];
}

// acc[j] += sum_g partial[g][j], g in order, in double: the fixed-order finish of the per-workgroup partials (and, called once per
// chunk, of the chunks).
__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const float* __restrict__ partial, int rows, int n, double* __restrict__ acc) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = acc[j];
    for (int g = 0; g < rows; ++g) s += (double)partial[(int64_t)g * n + j];
    acc[j] = s;
}

inline int km_kp(int clusters) { return clusters <= 8 ? 8 : clusters <= 16 ? 16 : clusters <= 24 ? 24 : 32; }

template <int KP, int MODE, int SLOTS = 6>
int km_launch(unsigned* done, size_t lds, int grid, hipStream_t s, const float* feat, const float* cen, int32_t* assign, float* mind,
              float* candd, int64_t cand_ld, float* partial, int C, int P, int S, int K, int n_tiles, int tiles_per_img) {
    if (lds > 64 * 1024) W2E_REQUIRE(big_lds_once((const void*)kmeans_pass_kernel<KP, MODE, SLOTS>, done), "kmeans_pass: LDS opt-in failed");
    kmeans_pass_kernel<KP, MODE, SLOTS><<<grid, KM_THREADS, lds, s>>>(feat, cen, assign, mind, candd, cand_ld, partial, C, P, S, K, n_tiles,
                                                                      tiles_per_img);
    return 0;
}

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_kmeans_plan(int batch, int channels, int pos_channels, int size, int clusters, int* grid, int* fused) {
    W2E_REQUIRE(grid && fused, "kmeans_plan: null output");
    W2E_REQUIRE(batch >= 0 && channels > 0 && pos_channels >= 0 && size > 1, "kmeans_plan: bad dims");
    W2E_REQUIRE(clusters >= 1 && clusters <= 32, "kmeans_plan: 1 <= clusters <= 32 (got %d)", clusters);
    const int64_t tiles = (int64_t)batch * ceil_div((int64_t)size * size, KM_TILE);
    const int cus = cu_count();
    *grid = (int)(tiles < 1 ? 1 : tiles < cus ? tiles : cus);
    const int D = channels + 2 * pos_channels;
    *fused = km_lds_floats(D, km_kp(clusters), clusters, KM_STEP) * 4 <= 160 * 1024 && size % 2 == 0;
    return 0;
}

extern "C" int w2e_kmeans_pass(int mode, const float* feat, const float* centroids, int32_t* assign, float* mind, float* cand_dist,
                               int64_t cand_ld, float* partial, int grid, int batch, int channels, int pos_channels, int size,
                               int clusters, void* stream) {
    W2E_REQUIRE(mode == KM_ASSIGN || mode == KM_STEP || mode == KM_SEED, "kmeans_pass: mode %d", mode);
    W2E_REQUIRE(feat && centroids && partial, "kmeans_pass: null tensor");
    W2E_REQUIRE(batch >= 0 && channels > 0 && pos_channels >= 0 && size > 1, "kmeans_pass: bad dims");
    W2E_REQUIRE(clusters >= 1 && clusters <= (mode == KM_SEED ? 8 : 32), "kmeans_pass: 1 <= clusters <= %d (got %d)",
                mode == KM_SEED ? 8 : 32, clusters);
    const int64_t npix = (int64_t)size * size;
    if (mode == KM_SEED) W2E_REQUIRE(cand_dist && cand_ld >= batch * npix, "kmeans_pass: candidate distance planes [T][ld], ld >= B*S*S");
    if (mode == KM_STEP) W2E_REQUIRE(size % 2 == 0, "kmeans_pass: the fused step reads 4 pixels at a time: even size (got %d)", size);
    if (mode == KM_STEP) W2E_REQUIRE((uintptr_t)feat % 16 == 0, "kmeans_pass: the fused step reads 4 pixels at a time: feat must be 16-byte aligned");
    const int tiles_per_img = (int)ceil_div(npix, KM_TILE);
    const int64_t tiles = (int64_t)batch * tiles_per_img;
    W2E_REQUIRE(tiles < (1ll << 31), "kmeans_pass: too many tiles");
    W2E_REQUIRE(grid >= 1 && grid <= 4096, "kmeans_pass: grid %d (w2e_kmeans_plan)", grid);
    const int KP = km_kp(clusters), D = channels + 2 * pos_channels;
    // mode 0 takes every shape w2e_cluster_assign takes ((D + 256) * {8,16,32} floats there): where six blocks of partial distances
    // do not fit beside the centres, the three-block kernel runs.  KP = 24 has none: w2e_cluster_assign pads K = 17..24 to 32 and
    // stops at D = 1024, the six-block form at D = 1315
    const bool three = mode == KM_ASSIGN && KP != 24 && km_lds_floats(D, KP, clusters, mode) * 4 > 160 * 1024;
    const size_t lds = (size_t)km_lds_floats(D, KP, clusters, mode, three ? 3 : 6) * 4;
    W2E_REQUIRE(lds <= 160 * 1024, "kmeans_pass: mode %d with %d clusters of %d dimensions needs %zu B of LDS", mode, clusters, D, lds);
    hipStream_t s = (hipStream_t)stream;
    static unsigned done[12];
    int rc = 0;
#define KM_GO3(KP_, MODE_, SLOTS_, slot)                                                                                          \
    rc = km_launch<KP_, MODE_, SLOTS_>(&done[slot], lds, grid, s, feat, centroids, assign, mind, cand_dist, cand_ld, partial, \
                                       channels, pos_channels, size, clusters, (int)tiles, tiles_per_img)
#define KM_GO(KP_, MODE_, slot) KM_GO3(KP_, MODE_, 6, slot)
    if (mode == KM_SEED) KM_GO(8, KM_SEED, 8);
    else if (three) {
        if (KP == 8) KM_GO3(8, KM_ASSIGN, 3, 9);
        else if (KP == 16) KM_GO3(16, KM_ASSIGN, 3, 10);
        else KM_GO3(32, KM_ASSIGN, 3, 11);
    } else if (mode == KM_ASSIGN) {
        if (KP == 8) KM_GO(8, KM_ASSIGN, 0);
        else if (KP == 16) KM_GO(16, KM_ASSIGN, 1);
        else if (KP == 24) KM_GO(24, KM_ASSIGN, 2);
        else KM_GO(32, KM_ASSIGN, 3);
    } else {
        if (KP == 8) KM_GO(8, KM_STEP, 4);
        else if (KP == 16) KM_GO(16, KM_STEP, 5);
        else if (KP == 24) KM_GO(24, KM_STEP, 6);
        else KM_GO(32, KM_STEP, 7);
    }
#undef KM_GO
#undef KM_GO3
    if (rc) return rc;
    W2E_LAUNCH_CHECK("kmeans_pass");
    return 0;
}

extern "C" int w2e_kmeans_reduce(const float* partial, int rows, int n, double* acc, void* stream) {
    W2E_REQUIRE(partial && acc, "kmeans_reduce: null tensor");
    W2E_REQUIRE(rows >= 0 && n >= 1, "kmeans_reduce: bad dims");
    kmeans_reduce_kernel<<<(int)ceil_div(n, 256), 256, 0, (hipStream_t)stream>>>(partial, rows, n, acc);
    W2E_LAUNCH_CHECK("kmeans_reduce");
    return 0;
}
