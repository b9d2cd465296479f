// K20 (projector): the arithmetic of StyleGAN2's projector (paper, Appendix D; rosinality's projector.py) around the generator pass --
// the noise-map gradient of the fused StyledConv, the multi-scale noise regulariser and its gradient, the in-place renormalisation of
// the noise maps, and the loss front (box down-sampling to the LPIPS resolution with the MSE term).  include/w2e_projector.h states
// what each entry point computes and replaces.  All fp32 in and out, no atomics, every sum in one fixed order.  The sums that cancel
// (the regulariser's means of products, the normaliser's moments) run in double: a product of two floats is exact there, and these
// kernels wait for memory, not for the fp64 pipe.  Lists of maps travel as tables in the kernel arguments (multi_tensor.h's scheme).
#include "common.h"
#include "device.h"
#include "multi_tensor.h"
#include "../../include/w2e_projector.h"

namespace w2e {

// ------------------------------------------------------------------------------------------ noise-map gradient
// A thread owns V consecutive pixels and the planes of one slice (plane % S == slice), in ascending order; the block then adds the S
// slices of a pixel group in ascending order through LDS.  Block: PG = 256 / S pixel groups x S slices, pixel groups fastest (the
// threads of a slice read consecutive addresses of a plane).
static int noise_grad_slices(int64_t planes, int64_t pixels) {
    const int64_t groups = (pixels % 4 == 0) ? pixels / 4 : pixels;
    int s = 1;
    while (s < 64 && 2 * s <= planes && groups * s < 65536) s *= 2;  // enough threads to cover the device, or no more planes to split
    return s;
}

template <int V>
__global__ __launch_bounds__(256) void noise_grad_kernel(const float* __restrict__ gpre, const float* __restrict__ noise_w,
                                                         float* __restrict__ g_noise, int64_t planes, int64_t pixels, int64_t groups,
                                                         int S, int accumulate) {
    __shared__ float part[256 * V];
    const int PG = 256 / S;
    const int pg = threadIdx.x % PG, slice = threadIdx.x / PG;
    const int64_t group = (int64_t)blockIdx.x * PG + pg;
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    if (group < groups) {
        const float* src = gpre + group * V;
#pragma unroll 4
        for (int64_t p = slice; p < planes; p += S) {
            if constexpr (V == 4) {
                const float4 t = *reinterpret_cast<const float4*>(src + p * pixels);
                acc[0] += t.x, acc[1] += t.y, acc[2] += t.z, acc[3] += t.w;
            } else {
                acc[0] += src[p * pixels];
            }
        }
    }
    if (S > 1) {
#pragma unroll
        for (int v = 0; v < V; ++v) part[threadIdx.x * V + v] = acc[v];
        __syncthreads();
        if (slice == 0) {
            for (int s = 1; s < S; ++s)
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] += part[(s * PG + pg) * V + v];
        }
    }
    if (slice == 0 && group < groups) {
        const float nw = noise_w[0];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float* o = g_noise + group * V + v;
            *o = accumulate ? *o + nw * acc[v] : nw * acc[v];
        }
    }
}

// ------------------------------------------------------------------------------------------ block sums in double
// The 256 threads' values, added in one fixed order (wave butterfly, then the four waves in order); the result in thread 0.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ void block_sum2_d(double& a, double& b, double (*sh)[2]) {
    a = wave_sum_d(a), b = wave_sum_d(b);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sh[wave][0] = a, sh[wave][1] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
        b = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
    }
}
// The first `n` (<= 64) slots of a partial-sum slab by one wave: every lane ends with both sums.
__device__ __forceinline__ void slots_sum_d(const double* slab, int n, double& a, double& b) {
    const int lane = threadIdx.x & 63;
    a = lane < n ? slab[2 * lane] : 0.0;
    b = lane < n ? slab[2 * lane + 1] : 0.0;
    a = wave_sum_d(a), b = wave_sum_d(b);
}

constexpr int PJ_SLOTS = W2E_PROJ_SLOTS;
constexpr int PJ_PER_BLOCK = 4096;  // elements a block takes before a tensor gets another block (up to PJ_SLOTS of them)

static inline int blocks_of(int64_t n) {
    const int64_t b = ceil_div(n, PJ_PER_BLOCK);
    return (int)(b < 1 ? 1 : (b > PJ_SLOTS ? PJ_SLOTS : b));
}

// ------------------------------------------------------------------------------------------ noise regulariser
// One entry per (map, level).  src: the level's values [batch, s, s]; dst / aux: what the kernel at hand writes or also reads.
struct RegTable {
    const float* src[MT_MAXT];
    float* dst[MT_MAXT];
    const float* aux[MT_MAXT];
    int s[MT_MAXT];       // side of the level (a power of two)
    int n[MT_MAXT];       // batch * s * s
    int slot[MT_MAXT];    // index of the (map, level) among all of the call: its partial-sum slab and its means
    int first[MT_MAXT];   // first unit (block) of the entry
    int count, units;
};

__device__ inline int reg_entry_of(const RegTable& tb, int unit) {
    int t = 0;
    while (t + 1 < tb.count && unit >= tb.first[t + 1]) ++t;
    return t;
}

// dst (level j + 1, side s / 2) = 2x2 box mean of src (level j, side s): one thread per output element.
__global__ __launch_bounds__(256) void reg_pool_kernel(RegTable tb) {
    const int t = reg_entry_of(tb, blockIdx.x);
    const int s = tb.s[t], h = s >> 1, n_out = tb.n[t] >> 2;
    const int i = (blockIdx.x - tb.first[t]) * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int x = i & (h - 1), y = (i / h) & (h - 1), b = i / (h * h);
    const float* p = tb.src[t] + (int64_t)b * s * s + (int64_t)(2 * y) * s + 2 * x;
    tb.dst[t][i] = ((p[0] + p[1]) + (p[s] + p[s + 1])) * 0.25f;
}

// partials[slot][k] = block k's sums of n * roll(n, 1, dim 3) and n * roll(n, 1, dim 2), in double.
__global__ __launch_bounds__(256) void reg_products_kernel(RegTable tb, double* __restrict__ partials) {
    __shared__ double sh[4][2];
    const int t = reg_entry_of(tb, blockIdx.x);
    const int k = blockIdx.x - tb.first[t];
    const int nb = (t + 1 < tb.count ? tb.first[t + 1] : tb.units) - tb.first[t];
    const int s = tb.s[t], n = tb.n[t], m = s - 1;
    const float* __restrict__ src = tb.src[t];
    double a = 0.0, b = 0.0;
    for (int i = k * 256 + threadIdx.x; i < n; i += nb * 256) {
        const int x = i & m, y = (i / s) & m, base = i - (y * s + x);
        const double v = src[i];
        a += v * (double)src[base + y * s + ((x - 1) & m)];
        b += v * (double)src[base + ((y - 1) & m) * s + x];
    }
    block_sum2_d(a, b, sh);
    if (threadIdx.x == 0) {
        double* o = partials + ((int64_t)tb.slot[t] * PJ_SLOTS + k) * 2;
        o[0] = a, o[1] = b;
    }
}

// means[slot] = (mean of the dim-3 products, mean of the dim-2 products), sq[slot] = their squares' sum: one wave per entry.
__global__ __launch_bounds__(64) void reg_means_kernel(RegTable tb, const double* __restrict__ partials, double* __restrict__ means,
                                                       double* __restrict__ sq) {
    const int t = blockIdx.x;
    const int nb = (t + 1 < tb.count ? tb.first[t + 1] : tb.units) - tb.first[t];
    double a, b;
    slots_sum_d(partials + (int64_t)tb.slot[t] * PJ_SLOTS * 2, nb, a, b);
    if (threadIdx.x == 0) {
        a /= (double)tb.n[t], b /= (double)tb.n[t];
        means[2 * tb.slot[t]] = a, means[2 * tb.slot[t] + 1] = b;
        sq[tb.slot[t]] = a * a + b * b;
    }
}

// loss[0] = sum of sq[0 .. entries): one wave, lane-strided in ascending order, then the butterfly.
__global__ __launch_bounds__(64) void reg_loss_kernel(const double* __restrict__ sq, int entries, float* __restrict__ loss) {
    double a = 0.0;
    for (int i = threadIdx.x; i < entries; i += 64) a += sq[i];
    a = wave_sum_d(a);
    if (threadIdx.x == 0) loss[0] = (float)a;
}

// dst (gradient of the level) = gout * (2 m3 / N) (left + right) + gout * (2 m2 / N) (up + down) + aux[coarser pixel] / 4.
// dst is a workspace level (never accumulated into) or the map's gradient (accumulate on request).
__global__ __launch_bounds__(256) void reg_grad_kernel(RegTable tb, const double* __restrict__ means, const float* __restrict__ gout,
                                                       int accumulate) {
    const int t = reg_entry_of(tb, blockIdx.x);
    const int s = tb.s[t], n = tb.n[t], m = s - 1;
    const int i = (blockIdx.x - tb.first[t]) * 256 + threadIdx.x;
    if (i >= n) return;
    const double scale = 2.0 * (double)gout[0] / (double)n;
    const float c3 = (float)(scale * means[2 * tb.slot[t]]), c2 = (float)(scale * means[2 * tb.slot[t] + 1]);
    const float* __restrict__ src = tb.src[t];
    const int x = i & m, y = (i / s) & m, base = i - (y * s + x);
    const float lr = src[base + y * s + ((x - 1) & m)] + src[base + y * s + ((x + 1) & m)];
    const float ud = src[base + ((y - 1) & m) * s + x] + src[base + ((y + 1) & m) * s + x];
    float g = c3 * lr + c2 * ud;
    if (tb.aux[t]) {
        const int h = s >> 1;
        g += 0.25f * tb.aux[t][(base >> 2) + (y >> 1) * h + (x >> 1)];
    }
    float* o = tb.dst[t] + i;
    *o = accumulate ? *o + g : g;
}

// ------------------------------------------------------------------------------------------ noise normalise
struct NormTable {
    float* p[MT_MAXT];
    int n[MT_MAXT];
    int slot[MT_MAXT];
    int first[MT_MAXT];
    int count, units;
};

__device__ inline int norm_entry_of(const NormTable& tb, int unit) {
    int t = 0;
    while (t + 1 < tb.count && unit >= tb.first[t + 1]) ++t;
    return t;
}

__global__ __launch_bounds__(256) void norm_moments_kernel(NormTable tb, double* __restrict__ partials) {
    __shared__ double sh[4][2];
    const int t = norm_entry_of(tb, blockIdx.x);
    const int k = blockIdx.x - tb.first[t];
    const int nb = (t + 1 < tb.count ? tb.first[t + 1] : tb.units) - tb.first[t];
    const float* __restrict__ p = tb.p[t];
    double a = 0.0, b = 0.0;
    for (int i = k * 256 + threadIdx.x; i < tb.n[t]; i += nb * 256) {
        const double v = p[i];
        a += v, b += v * v;
    }
    block_sum2_d(a, b, sh);
    if (threadIdx.x == 0) {
        double* o = partials + ((int64_t)tb.slot[t] * PJ_SLOTS + k) * 2;
        o[0] = a, o[1] = b;
    }
}

// Every block adds its map's partial sums again (the same slots in the same order: the same mean and deviation in every block), then
// rewrites its share of the map.
__global__ __launch_bounds__(256) void norm_apply_kernel(NormTable tb, const double* __restrict__ partials) {
    const int t = norm_entry_of(tb, blockIdx.x);
    const int k = blockIdx.x - tb.first[t];
    const int nb = (t + 1 < tb.count ? tb.first[t + 1] : tb.units) - tb.first[t];
    double sx, sxx;
    slots_sum_d(partials + (int64_t)tb.slot[t] * PJ_SLOTS * 2, nb, sx, sxx);
    const double n = (double)tb.n[t];
    const double mean = sx / n;
    const double var = (sxx - sx * mean) / (n - 1.0);
    const double rstd = 1.0 / sqrt(var);
    float* __restrict__ p = tb.p[t];
    for (int i = k * 256 + threadIdx.x; i < tb.n[t]; i += nb * 256) p[i] = (float)(((double)p[i] - mean) * rstd);
}

// ------------------------------------------------------------------------------------------ loss front
// One thread per element of `small`; 32-bit index arithmetic (the launcher refuses more than 2^30 image elements).  F = 4 / 2: a box row is one
// float4 / float2 load (16-byte aligned img, f = F); F = 0: any f, scalar loads.  Every form adds the box in row order, left to right.
template <int F>
__global__ __launch_bounds__(256) void front_fwd_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                        float* __restrict__ small, double* __restrict__ partials, int n_small,
                                                        int oh, int ow, int width, int f, float inv) {
    __shared__ double sh[4][2];
    double a = 0.0, unused = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_small; i += gridDim.x * 256) {
        const int x = i % ow, row = i / ow;  // row = plane * oh + y: the box starts at image row `row * f`
        const float* p = img + ((int64_t)row * f) * width + x * f;
        float v = 0.f;
        if constexpr (F == 4) {
#pragma unroll
            for (int dy = 0; dy < 4; ++dy) {
                const float4 t = *reinterpret_cast<const float4*>(p + (int64_t)dy * width);
                v += t.x, v += t.y, v += t.z, v += t.w;
            }
        } else if constexpr (F == 2) {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const float2 t = *reinterpret_cast<const float2*>(p + (int64_t)dy * width);
                v += t.x, v += t.y;
            }
        } else {
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) v += p[(int64_t)dy * width + dx];
        }
        v *= inv;
        small[i] = v;
        if (target) {
            const double d = (double)v - (double)target[i];
            a += d * d;
        }
    }
    if (partials) {
        block_sum2_d(a, unused, sh);
        if (threadIdx.x == 0) partials[blockIdx.x] = a;
    }
}

// One thread per V consecutive pixels of a row of g_img (V = 4: width % 4 == 0 and a 16-byte aligned g_img, one float4 store).
template <int V>
__global__ __launch_bounds__(256) void front_bwd_kernel(const float* __restrict__ g_small, const float* __restrict__ small,
                                                        const float* __restrict__ target, const float* __restrict__ g_mse, float coef,
                                                        float* __restrict__ g_img, int n_groups, int height, int width, int f, float inv) {
    const float c = g_mse ? coef * g_mse[0] : 0.f;
    const int oh = height / f, ow = width / f, per_row = width / V;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_groups; i += gridDim.x * 256) {
        const int x = (i % per_row) * V, row = i / per_row;  // row = plane * height + y
        const int y = row % height, plane = row / height;
        const int jrow = (plane * oh + y / f) * ow;
        float g[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int j = jrow + (x + v) / f;
            float t = g_small ? g_small[j] : 0.f;
            if (g_mse) t += c * (small[j] - target[j]);
            g[v] = t * inv;
        }
        float* o = g_img + (int64_t)row * width + x;
        if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(g[0], g[1], g[2], g[3]);
        else o[0] = g[0];
    }
}

// ------------------------------------------------------------------------------------------ host side of the regulariser
static inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline int reg_levels(int size) {
    int levels = 1;
    for (; size > 8; size >>= 1) ++levels;
    return levels;
}

// The workspace in floats: [partials: entries * SLOTS * 2 doubles][means: entries * 2 doubles][sq: entries doubles][pooled levels]
// [gradients of the pooled levels].  Entries are the (map, level) pairs in (map, level) order; a map's pooled levels follow each other.
struct RegLayout {
    int64_t entries, pooled_floats;
    int max_levels;
    int64_t off_means() const { return entries * PJ_SLOTS * 4; }
    int64_t off_sq() const { return off_means() + entries * 4; }
    int64_t off_pooled() const { return off_sq() + entries * 2; }
    int64_t off_grads() const { return off_pooled() + pooled_floats; }
    int64_t total() const { return off_grads() + pooled_floats; }
};

// nullptr, or why the lists are refused.
static const char* reg_layout(int count, const int* batch, const int* size, RegLayout& lay) {
    lay = RegLayout{0, 0, 0};
    if (count < 0 || (count > 0 && (!batch || !size))) return refusal("null or negative list");
    for (int i = 0; i < count; ++i) {
        if (batch[i] < 1 || !pow2(size[i]))
            return refusal("map %d is [%d,1,%d,%d]: needs batch >= 1 and a power-of-two side", i, batch[i], size[i], size[i]);
        if ((int64_t)batch[i] * size[i] * size[i] > (1 << 30)) return refusal("map %d has more than 2^30 elements", i);
        const int levels = reg_levels(size[i]);
        lay.entries += levels;
        lay.max_levels = levels > lay.max_levels ? levels : lay.max_levels;
        for (int j = 1, s = size[i] >> 1; j < levels; ++j, s >>= 1) lay.pooled_floats += (int64_t)batch[i] * s * s;
    }
    if (lay.entries > (1 << 20)) return refusal("more than 2^20 (map, level) pairs");
    return nullptr;
}

// Every (map, level = `level`) of the lists, MT_MAXT per table: fill(tb, k, map, off, next) sets the pointers its kernel reads
// (src always; dst and aux only where the kernel at hand uses them: they stay null for the products and the means) from `off`, the
// offset of the level in the pooled slab (level 0: -1), and `next`, the offset of the map's next level (-1: this is its last), and
// returns the entry's units.  level < 0: every level.
template <class Fill, class Launch>
static int reg_for_each_table(int count, const int* batch, const int* size, int level, Fill fill, Launch launch) {
    RegTable tb{};
    int64_t units = 0, pooled = 0;
    int slot = 0;
    const auto flush = [&]() {
        if (tb.count == 0) return 0;
        tb.units = (int)units;
        const int rc = launch(tb);
        tb = RegTable{};
        units = 0;
        return rc;
    };
    for (int i = 0; i < count; ++i) {
        const int levels = reg_levels(size[i]);
        int s = size[i];
        for (int j = 0; j < levels; ++j, ++slot, s >>= 1) {
            const int64_t n = (int64_t)batch[i] * s * s;
            const int64_t off = j == 0 ? -1 : pooled;
            const int64_t next = j + 1 < levels ? (j == 0 ? pooled : pooled + n) : -1;
            if (j > 0) pooled += n;
            if (level >= 0 && j != level) continue;
            const int k = tb.count++;
            tb.s[k] = s, tb.n[k] = (int)n, tb.slot[k] = slot, tb.first[k] = (int)units;
            units += fill(tb, k, i, off, next);
            if (tb.count == MT_MAXT || units > (1 << 30))
                if (const int rc = flush()) return rc;
        }
    }
    return flush();
}

}  // namespace w2e

using namespace w2e;

extern "C" {

int w2e_noise_grad_slices(int64_t planes, int64_t pixels) {
    if (planes < 1 || pixels < 1) return 0;
    return noise_grad_slices(planes, pixels);
}

int w2e_noise_grad(const float* gpre, const float* noise_w, float* g_noise, int64_t planes, int64_t pixels, int accumulate,
                   void* stream) {
    W2E_REQUIRE(gpre && noise_w && g_noise, "noise_grad: null tensor");
    W2E_REQUIRE(planes >= 1 && pixels >= 1, "noise_grad: bad dims %lld planes, %lld pixels", (long long)planes, (long long)pixels);
    W2E_REQUIRE(planes <= INT32_MAX && pixels <= INT32_MAX, "noise_grad: more than 2^31 - 1 planes or pixels");
    // S from the dims alone, so that the order of the sums does not depend on an address: with pixels % 4 == 0 and an unaligned gpre the
    // one-pixel form runs with the S sized for a quarter of its threads -- more threads than the heuristic asked for, the same sums
    const int S = noise_grad_slices(planes, pixels);
    const bool vec = pixels % 4 == 0 && ((uintptr_t)gpre % 16) == 0 && ((uintptr_t)g_noise % 4) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        noise_grad_kernel<4><<<(unsigned)ceil_div(pixels / 4, 256 / S), 256, 0, st>>>(gpre, noise_w, g_noise, planes, pixels, pixels / 4, S, accumulate);
    else
        noise_grad_kernel<1><<<(unsigned)ceil_div(pixels, 256 / S), 256, 0, st>>>(gpre, noise_w, g_noise, planes, pixels, pixels, S, accumulate);
    W2E_LAUNCH_CHECK("noise_grad");
    return 0;
}

int w2e_noise_reg_workspace(int count, const int* batch, const int* size, int64_t* floats) {
    RegLayout lay;
    const char* why = reg_layout(count, batch, size, lay);
    W2E_REQUIRE(!why, "noise_reg_workspace: %s", why);
    W2E_REQUIRE(floats, "noise_reg_workspace: null floats");
    *floats = lay.total();
    return 0;
}

int w2e_noise_reg_fwd(int count, const float* const* maps, const int* batch, const int* size, float* workspace,
                      int64_t workspace_floats, float* loss, void* stream) {
    RegLayout lay;
    const char* why = reg_layout(count, batch, size, lay);
    W2E_REQUIRE(!why, "noise_reg_fwd: %s", why);
    W2E_REQUIRE(loss, "noise_reg_fwd: null loss");
    W2E_REQUIRE(count == 0 || maps, "noise_reg_fwd: null list");
    for (int i = 0; i < count; ++i) W2E_REQUIRE(maps[i], "noise_reg_fwd: map %d is null", i);
    W2E_REQUIRE(workspace && workspace_floats >= lay.total() && ((uintptr_t)workspace % 8) == 0,
                "noise_reg_fwd: the workspace needs %lld floats at an 8-byte aligned address (got %lld)", (long long)lay.total(),
                (long long)workspace_floats);
    hipStream_t st = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    double* means = reinterpret_cast<double*>(workspace + lay.off_means());
    double* sq = reinterpret_cast<double*>(workspace + lay.off_sq());
    float* pooled = workspace + lay.off_pooled();
    // the pyramid, one step per launch: every map that has level `level` + 1 pools its level `level`
    for (int level = 0; level + 1 < lay.max_levels; ++level) {
        const int rc = reg_for_each_table(
            count, batch, size, level,
            [&](RegTable& tb, int k, int i, int64_t off, int64_t next) -> int64_t {
                if (next < 0) {  // the map ends at this level: no entry
                    --tb.count;
                    return 0;
                }
                tb.src[k] = off < 0 ? maps[i] : pooled + off;
                tb.dst[k] = pooled + next;
                return ceil_div(tb.n[k] / 4, 256);
            },
            [&](const RegTable& tb) {
                reg_pool_kernel<<<(unsigned)tb.units, 256, 0, st>>>(tb);
                W2E_LAUNCH_CHECK("noise_reg_fwd (pool)");
                return 0;
            });
        if (rc) return rc;
    }
    // the products of every (map, level) and their means
    const int rc = reg_for_each_table(
        count, batch, size, -1,
        [&](RegTable& tb, int k, int i, int64_t off, int64_t) -> int64_t {
            tb.src[k] = off < 0 ? maps[i] : pooled + off;
            return blocks_of(tb.n[k]);
        },
        [&](const RegTable& tb) {
            reg_products_kernel<<<(unsigned)tb.units, 256, 0, st>>>(tb, partials);
            W2E_LAUNCH_CHECK("noise_reg_fwd (products)");
            reg_means_kernel<<<(unsigned)tb.count, 64, 0, st>>>(tb, partials, means, sq);
            W2E_LAUNCH_CHECK("noise_reg_fwd (means)");
            return 0;
        });
    if (rc) return rc;
    reg_loss_kernel<<<1, 64, 0, st>>>(sq, (int)lay.entries, loss);
    W2E_LAUNCH_CHECK("noise_reg_fwd (loss)");
    return 0;
}

int w2e_noise_reg_bwd(int count, const float* const* maps, const int* batch, const int* size, float* workspace,
                      int64_t workspace_floats, const float* gout, float* const* grads, int accumulate, void* stream) {
    RegLayout lay;
    const char* why = reg_layout(count, batch, size, lay);
    W2E_REQUIRE(!why, "noise_reg_bwd: %s", why);
    W2E_REQUIRE(gout, "noise_reg_bwd: null gout");
    W2E_REQUIRE(count == 0 || (maps && grads), "noise_reg_bwd: null list");
    for (int i = 0; i < count; ++i) W2E_REQUIRE(maps[i] && grads[i], "noise_reg_bwd: map or gradient %d is null", i);
    W2E_REQUIRE(workspace && workspace_floats >= lay.total() && ((uintptr_t)workspace % 8) == 0,
                "noise_reg_bwd: the workspace needs %lld floats at an 8-byte aligned address (got %lld)", (long long)lay.total(),
                (long long)workspace_floats);
    hipStream_t st = (hipStream_t)stream;
    const double* means = reinterpret_cast<const double*>(workspace + lay.off_means());
    const float* pooled = workspace + lay.off_pooled();
    float* gpool = workspace + lay.off_grads();
    // coarse to fine: level `level` of every map that has it reads the finished gradient of its level + 1
    for (int level = lay.max_levels - 1; level >= 0; --level) {
        const int acc = level == 0 ? accumulate : 0;
        const int rc = reg_for_each_table(
            count, batch, size, level,
            [&](RegTable& tb, int k, int i, int64_t off, int64_t next) -> int64_t {
                tb.src[k] = off < 0 ? maps[i] : pooled + off;
                tb.dst[k] = off < 0 ? grads[i] : gpool + off;
                tb.aux[k] = next < 0 ? nullptr : gpool + next;
                return ceil_div(tb.n[k], 256);
            },
            [&](const RegTable& tb) {
                reg_grad_kernel<<<(unsigned)tb.units, 256, 0, st>>>(tb, means, gout, acc);
                W2E_LAUNCH_CHECK("noise_reg_bwd");
                return 0;
            });
        if (rc) return rc;
    }
    return 0;
}

int w2e_noise_normalize(int count, float* const* maps, const int64_t* numel, float* workspace, int64_t workspace_floats, void* stream) {
    W2E_REQUIRE(count >= 0 && (count == 0 || (maps && numel)), "noise_normalize: null or negative list");
    for (int i = 0; i < count; ++i) {
        W2E_REQUIRE(maps[i], "noise_normalize: map %d is null", i);
        W2E_REQUIRE(numel[i] >= 2 && numel[i] <= (1 << 30), "noise_normalize: map %d has %lld elements (2 .. 2^30)", i, (long long)numel[i]);
    }
    W2E_REQUIRE(count == 0 || (workspace && workspace_floats >= (int64_t)count * PJ_SLOTS * 4 && ((uintptr_t)workspace % 8) == 0),
                "noise_normalize: the workspace needs %lld floats at an 8-byte aligned address (got %lld)",
                (long long)count * PJ_SLOTS * 4, (long long)workspace_floats);
    hipStream_t st = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    for (int at = 0; at < count;) {
        NormTable tb{};
        int64_t units = 0;
        for (; at < count && tb.count < MT_MAXT; ++at) {
            const int k = tb.count++;
            tb.p[k] = maps[at], tb.n[k] = (int)numel[at], tb.slot[k] = at, tb.first[k] = (int)units;
            units += blocks_of(numel[at]);
        }
        tb.units = (int)units;
        norm_moments_kernel<<<(unsigned)tb.units, 256, 0, st>>>(tb, partials);
        W2E_LAUNCH_CHECK("noise_normalize (moments)");
        norm_apply_kernel<<<(unsigned)tb.units, 256, 0, st>>>(tb, partials);
        W2E_LAUNCH_CHECK("noise_normalize (apply)");
    }
    return 0;
}

int w2e_proj_front_blocks(int64_t small_numel) {
    if (small_numel < 1) return 0;
    const int64_t b = ceil_div(small_numel, 1024);
    return (int)(b > W2E_PROJ_FRONT_PARTIALS ? W2E_PROJ_FRONT_PARTIALS : b);
}

static const char* front_dims(int batch, int channels, int height, int width, int f) {
    if (batch < 1 || channels < 1 || height < 1 || width < 1 || f < 1) return refusal("bad dims %d %d %d %d, f %d", batch, channels, height, width, f);
    if (height % f || width % f) return refusal("%d x %d is no multiple of f = %d", height, width, f);
    if ((int64_t)batch * channels * height * width > (1 << 30)) return refusal("more than 2^30 image elements");  // (32-bit grid strides)
    return nullptr;
}

int w2e_proj_front_fwd(const float* img, const float* target, int batch, int channels, int height, int width, int f, float* small,
                       double* partials, void* stream) {
    const char* why = front_dims(batch, channels, height, width, f);
    W2E_REQUIRE(!why, "proj_front_fwd: %s", why);
    W2E_REQUIRE(img && small, "proj_front_fwd: null tensor");
    W2E_REQUIRE(!target == !partials, "proj_front_fwd: target and partials go together");
    const int oh = height / f, ow = width / f;
    const int n_small = batch * channels * oh * ow;
    const unsigned grid = (unsigned)w2e_proj_front_blocks(n_small);
    hipStream_t st = (hipStream_t)stream;
    const float inv = 1.0f / (float)(f * f);
    const bool aligned = ((uintptr_t)img % 16) == 0;  // (width is a multiple of f: every box row then starts on an f-float boundary)
    if (f == 4 && aligned) front_fwd_kernel<4><<<grid, 256, 0, st>>>(img, target, small, partials, n_small, oh, ow, width, f, inv);
    else if (f == 2 && aligned) front_fwd_kernel<2><<<grid, 256, 0, st>>>(img, target, small, partials, n_small, oh, ow, width, f, inv);
    else front_fwd_kernel<0><<<grid, 256, 0, st>>>(img, target, small, partials, n_small, oh, ow, width, f, inv);
    W2E_LAUNCH_CHECK("proj_front_fwd");
    return 0;
}

int w2e_proj_front_bwd(const float* g_small, const float* small, const float* target, const float* g_mse, float coef, int batch,
                       int channels, int height, int width, int f, float* g_img, void* stream) {
    const char* why = front_dims(batch, channels, height, width, f);
    W2E_REQUIRE(!why, "proj_front_bwd: %s", why);
    W2E_REQUIRE(g_img, "proj_front_bwd: null g_img");
    W2E_REQUIRE(!g_mse || (small && target), "proj_front_bwd: the MSE term needs small and target");
    const int n_img = batch * channels * height * width;
    hipStream_t st = (hipStream_t)stream;
    const float inv = 1.0f / (float)(f * f);
    if (width % 4 == 0 && ((uintptr_t)g_img % 16) == 0)
        front_bwd_kernel<4><<<stream_grid(n_img / 4, 256), 256, 0, st>>>(g_small, small, target, g_mse, coef, g_img, n_img / 4, height, width, f, inv);
    else
        front_bwd_kernel<1><<<stream_grid(n_img, 256), 256, 0, st>>>(g_small, small, target, g_mse, coef, g_img, n_img, height, width, f, inv);
    W2E_LAUNCH_CHECK("proj_front_bwd");
    return 0;
}

}  // extern "C"
