// K12e: the style branch of the region-attention net (attention/run_attention.py:811-828, FullSpaceMapperFEATClusterLinStyle_Net): per
// S-space code c below mapper_layer
//     x_text_hidden = mapper_text_c(x_text)            2 x EqualLinear(fused_lrelu): E -> (E+512)/2 -> 512
//     x_c_hidden    = mapper_c(x_c)                    EqualLinear(d_c, d_c)
//     x_c_new       = x_c + alpha * (mapper_all_c(x_c_hidden || x_text_hidden) - x_c),   loss_delta += mean_b ||x_c_new - x_c|| / mapper_layer
// on B <= 16 rows: as stock ops about 20 launches per code forward and twice that backward.  Here one layer of ALL codes is one launch
// per direction.  A "group" is one EqualLinear: out [B, n] from one or two row-major sources ([B, k0] with row stride ld0, [B, k1]
// with row stride ld1) contracted as if concatenated, against the weight AS STORED ([n, k0 + k1], row o = output feature o).  Every
// pointer of a group travels in the kernel arguments (RsGroups, by value), so groups of one launch may belong to different module
// families, read a shared source, or point into packed buffers.
//
// fp32 FMA, fp32 accumulation; every sum has one fixed order, no atomics: the same bits on every run.  The kernels are bound by one
// pass over the weights (forward, input gradient) or over the weight gradients (weight gradient): 16-byte accesses where every
// width is a multiple of 4 and every pointer 16-byte aligned (the production shapes), one float per lane otherwise.
#include "common.h"
#include "device.h"

namespace w2e {

constexpr int RS_MAXG = 32, RS_MAXB = 16, RS_MAXDIM = 4096;
constexpr float RS_SLOPE = 0.2f, RS_GAIN = 1.4142135623730951f;

struct RsGroups {
    int groups, batch;
    const float* a0[RS_MAXG];   // forward / weight gradient: the sources.  Input gradient: gy [B, n] and y [B, n] (the layer's output)
    const float* a1[RS_MAXG];
    const float* w[RS_MAXG];    // [n, k0 + k1]
    const float* bias[RS_MAXG]; // forward: [n] or null.  Weight gradient: gy [B, n]
    const float* y[RS_MAXG];    // weight gradient: y [B, n] (null where act = 0)
    float* o0[RS_MAXG];         // forward: out [B, n].  Input gradient: gx of source 0 / 1 (null = not wanted).  Weight gradient: gw, gb
    float* o1[RS_MAXG];
    int k0[RS_MAXG], k1[RS_MAXG], n[RS_MAXG], ld0[RS_MAXG], ld1[RS_MAXG], act[RS_MAXG];
    float w_scale[RS_MAXG];
};

__device__ __forceinline__ float rs_act(float v, int act) { return act ? (v > 0.f ? v : v * RS_SLOPE) * RS_GAIN : v; }
// d act / d pre, from the OUTPUT y (its sign is the pre-activation's; y == 0 takes the negative side, as fused_leaky_relu's backward does)
__device__ __forceinline__ float rs_dact(float y, int act) { return act ? (y > 0.f ? RS_GAIN : RS_GAIN * RS_SLOPE) : 1.f; }

// Forward:  out[m, o] = act(w_scale * sum_k a[m, k] W[o, k] + b_scale * bias[o]).  One wave per output feature o (4 per workgroup; grid
// (ceil(max n / 4), groups): 1792 workgroups at 14 codes of width 512).  The lanes split k -- VEC: lane l holds k = 4l .. 4l+3 of every
// 256-wide slab, one coalesced 16-byte read of the weight row per slab --, all MB rows accumulate in registers against that one read,
// and a butterfly finishes each row.
template <int MB, bool VEC>
__global__ __launch_bounds__(256) void rs_fwd_kernel(RsGroups g, float b_scale) {
    const int c = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o = blockIdx.x * 4 + wave;
    if (o >= g.n[c]) return;
    const int k0 = g.k0[c], k1 = g.k1[c], K = k0 + k1, ld0 = g.ld0[c], ld1 = g.ld1[c], batch = g.batch;
    const float* __restrict__ wr = g.w[c] + (int64_t)o * K;
    const float* __restrict__ s0 = g.a0[c];
    const float* __restrict__ s1 = g.a1[c];
    float acc[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) acc[m] = 0.f;
    if constexpr (VEC) {
        for (int k = 4 * lane; k < K; k += 256) {
            const float4 wv = *reinterpret_cast<const float4*>(wr + k);
            const float* ap = k < k0 ? s0 + k : s1 + (k - k0);
            const int ld = k < k0 ? ld0 : ld1;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (m < batch) {
                    const float4 av = *reinterpret_cast<const float4*>(ap + (int64_t)m * ld);
                    acc[m] += av.x * wv.x, acc[m] += av.y * wv.y, acc[m] += av.z * wv.z, acc[m] += av.w * wv.w;
                }
            }
        }
    } else {
        for (int k = lane; k < K; k += 64) {
            const float wv = wr[k];
            const float* ap = k < k0 ? s0 + k : s1 + (k - k0);
            const int ld = k < k0 ? ld0 : ld1;
#pragma unroll
            for (int m = 0; m < MB; ++m)
                if (m < batch) acc[m] += ap[(int64_t)m * ld] * wv;
        }
    }
    const float bs = g.bias[c] ? g.bias[c][o] * b_scale : 0.f;
    const int n = g.n[c], act = g.act[c];
    const float ws = g.w_scale[c];
    float* __restrict__ out = g.o0[c];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        if (m < batch) {
            const float s = wave_sum(acc[m]);
            if (lane == 0) out[(int64_t)m * n + o] = rs_act(s * ws + bs, act);
        }
    }
}

// Input gradient:  gx[m, i] = w_scale * sum_o gpre[m, o] W[o, i],  gpre = gy .* act'(y), written per source (a null gx is skipped by the
// host choosing the i range: a workgroup whose 64 columns all belong to unwanted sources returns at once).  A workgroup owns 64
// consecutive columns i of one group; gpre of the group is staged in LDS.  VEC: thread (q, l) = (tid / 16, tid % 16) owns columns
// i0 + 4l .. + 3 and the rows o = q, q + 16, ...: a wave reads four 256-byte row segments per step.  Scalar: thread (q, l) =
// (tid / 64, tid % 64) owns column i0 + l and the rows o = q, q + 4, ....  The partial sums of a column are joined in a fixed order: the
// four row classes of a wave by two butterfly steps (VEC), then the four waves in ascending order through LDS.
constexpr int RS_IT = 64;  // columns per workgroup
template <int MB, bool VEC>
__global__ __launch_bounds__(256) void rs_dgrad_kernel(RsGroups g) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];  // gpre [batch][n], then part [4][MB][RS_IT]
    const int c = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const int k0 = g.k0[c], k1 = g.k1[c], K = k0 + k1, n = g.n[c], batch = g.batch, act = g.act[c];
    const int i0 = blockIdx.x * RS_IT;
    if (i0 >= K) return;
    {   // nothing wanted in [i0, i0 + RS_IT)?
        const int i1 = i0 + RS_IT < K ? i0 + RS_IT : K;
        const bool want0 = g.o0[c] && i0 < k0, want1 = g.o1[c] && i1 > k0;
        if (!want0 && !want1) return;
    }
    float* gp = rs_lds;
    float* part = rs_lds + ((batch * n + 3) & ~3);
    const float* __restrict__ gy = g.a0[c];
    const float* __restrict__ y = g.a1[c];
    for (int e = tid; e < batch * n; e += 256) gp[e] = gy[e] * rs_dact(act ? y[e] : 1.f, act);
    __syncthreads();
    const float* __restrict__ W = g.w[c];
    constexpr int CW = VEC ? 4 : 1;                  // columns per thread
    const int l = VEC ? (tid & 15) : (tid & 63), q = VEC ? (tid >> 4) : (tid >> 6), QS = VEC ? 16 : 4;
    const int i = i0 + CW * l;
    float acc[MB][CW];
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int j = 0; j < CW; ++j) acc[m][j] = 0.f;
    if (i < K) {
        for (int o = q; o < n; o += QS) {
            float wv[CW];
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(W + (int64_t)o * K + i);
                wv[0] = t.x, wv[1] = t.y, wv[2] = t.z, wv[3] = t.w;
            } else {
                wv[0] = W[(int64_t)o * K + i];
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                if (m < batch) {
                    const float gv = gp[m * n + o];
#pragma unroll
                    for (int j = 0; j < CW; ++j) acc[m][j] += gv * wv[j];
                }
            }
        }
    }
    if constexpr (VEC) {  // the four row classes of this wave: lanes l, l + 16, l + 32, l + 48
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int j = 0; j < CW; ++j) {
                float v = acc[m][j];
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                acc[m][j] = v;
            }
    }
    if (!VEC || (tid & 63) < 16) {
#pragma unroll
        for (int m = 0; m < MB; ++m)
#pragma unroll
            for (int j = 0; j < CW; ++j) part[(wave * MB + m) * RS_IT + CW * l + j] = acc[m][j];
    }
    __syncthreads();
    const float ws = g.w_scale[c];
    for (int e = tid; e < MB * RS_IT; e += 256) {
        const int m = e / RS_IT, col = e - m * RS_IT, ii = i0 + col;
        if (m >= batch || ii >= K) continue;
        const float v = ((part[(0 * MB + m) * RS_IT + col] + part[(1 * MB + m) * RS_IT + col]) + part[(2 * MB + m) * RS_IT + col]) +
                        part[(3 * MB + m) * RS_IT + col];
        if (ii < k0) {
            if (g.o0[c]) g.o0[c][(int64_t)m * k0 + ii] = v * ws;
        } else if (g.o1[c]) {
            g.o1[c][(int64_t)m * k1 + (ii - k0)] = v * ws;
        }
    }
}

// Weight and bias gradient:  gW[o, i] = w_scale * sum_m gpre[m, o] a[m, i],  gb[o] = b_scale * sum_m gpre[m, o],  gpre = gy .* act'(y);
// WRITTEN, rows m in ascending order.  A thread owns (o, 4 consecutive i) (VEC: one 16-byte store; the write of gW is the traffic of
// this kernel) or one (o, i).
template <bool VEC>
__global__ __launch_bounds__(256) void rs_wgrad_kernel(RsGroups g, float b_scale) {
    const int c = blockIdx.y;
    const int k0 = g.k0[c], k1 = g.k1[c], K = k0 + k1, n = g.n[c], batch = g.batch, act = g.act[c];
    constexpr int CW = VEC ? 4 : 1;
    const int per_row = (K + CW - 1) / CW;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * per_row) return;
    const int o = (int)(e / per_row), i = (int)(e - (int64_t)o * per_row) * CW;
    const float* __restrict__ gy = g.bias[c];
    const float* __restrict__ y = g.y[c];
    const float* ap = i < k0 ? g.a0[c] + i : g.a1[c] + (i - k0);
    const int ld = i < k0 ? g.ld0[c] : g.ld1[c];
    float s[CW], sb = 0.f;
#pragma unroll
    for (int j = 0; j < CW; ++j) s[j] = 0.f;
    for (int m = 0; m < batch; ++m) {
        const float gv = gy[(int64_t)m * n + o] * rs_dact(act ? y[(int64_t)m * n + o] : 1.f, act);
        sb += gv;
        if constexpr (VEC) {
            const float4 av = *reinterpret_cast<const float4*>(ap + (int64_t)m * ld);
            s[0] += gv * av.x, s[1] += gv * av.y, s[2] += gv * av.z, s[3] += gv * av.w;
        } else {
            s[0] += gv * ap[(int64_t)m * ld];
        }
    }
    const float ws = g.w_scale[c];
    float* gw = g.o0[c] + (int64_t)o * K + i;
    if constexpr (VEC) *reinterpret_cast<float4*>(gw) = make_float4(s[0] * ws, s[1] * ws, s[2] * ws, s[3] * ws);
    else *gw = s[0] * ws;
    if (i == 0 && g.o1[c]) g.o1[c][o] = sb * b_scale;
}

// The finish.  Per code c and row m (one wave each):  diff = alpha * (y - x),  x_new = x + diff,  norm[c * B + m] = ||diff||_2 (lane-strided
// partial sums joined by the butterfly: one fixed order).  x is read in place out of the caller's [B, 1, E + d] rows (row stride ldx).
struct RsFinish {
    int groups, batch;
    const float* x[RS_MAXG];   // [B, d] with row stride ldx
    const float* y[RS_MAXG];   // [B, d] mapper_all's output
    const float* go[RS_MAXG];  // backward: the gradient of x_new [B, d] (null = zeros)
    float* out[RS_MAXG];       // forward: x_new [B, d];  backward: gy [B, d]
    int d[RS_MAXG], ldx[RS_MAXG];
};

__global__ __launch_bounds__(256) void rs_finish_fwd_kernel(RsFinish f, float alpha, float* __restrict__ norms) {
    const int c = blockIdx.y, lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= f.batch) return;
    const int d = f.d[c];
    const float* __restrict__ x = f.x[c] + (int64_t)m * f.ldx[c];
    const float* __restrict__ y = f.y[c] + (int64_t)m * d;
    float* __restrict__ out = f.out[c] + (int64_t)m * d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float diff = alpha * (y[j] - x[j]);
        out[j] = x[j] + diff;
        s += diff * diff;
    }
    s = wave_sum(s);
    if (lane == 0) norms[c * f.batch + m] = sqrtf(s);
}

// loss_delta = sum_c (sum_m norm[c, m] / B) / layers: one wave, lane-strided over the groups * batch norms, then the butterfly
__global__ __launch_bounds__(64) void rs_loss_kernel(const float* __restrict__ norms, int count, float scale, float* __restrict__ loss) {
    float s = 0.f;
    for (int e = threadIdx.x; e < count; e += 64) s += norms[e];
    s = wave_sum(s);
    if (threadIdx.x == 0) *loss = s * scale;
}

// gy[m, j] = alpha * (g_out[m, j] + g_loss * diff[m, j] / norm[c, m] * scale),  scale = 1 / (B * layers); the norm term is 0 where
// norm == 0 (torch's norm backward masks that row; never NaN)
__global__ __launch_bounds__(256) void rs_finish_bwd_kernel(RsFinish f, float alpha, float scale, const float* __restrict__ norms,
                                                           const float* __restrict__ g_loss) {
    const int c = blockIdx.y, d = f.d[c];
    const float gl = g_loss ? *g_loss * scale : 0.f;
    const float* __restrict__ go = f.go[c];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < f.batch * d; e += gridDim.x * 256) {
        const int m = e / d, j = e - m * d;
        const float nrm = norms[c * f.batch + m];
        float v = go ? go[e] : 0.f;
        if (nrm > 0.f && gl != 0.f) {
            const float diff = alpha * (f.y[c][e] - f.x[c][(int64_t)m * f.ldx[c] + j]);
            v += gl * (diff / nrm);
        }
        f.out[c][e] = alpha * v;
    }
}

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace w2e

using namespace w2e;

#define RS_BATCH_DISPATCH(batch, CALL) \
    do {                               \
        if ((batch) <= 1) { CALL(1); } \
        else if ((batch) <= 2) { CALL(2); } \
        else if ((batch) <= 4) { CALL(4); } \
        else if ((batch) <= 8) { CALL(8); } \
        else { CALL(16); }             \
    } while (0)

static int rs_check_dims(const char* who, int groups, int batch, const int* k0, const int* k1, const int* n) {
    W2E_REQUIRE(groups >= 1 && groups <= RS_MAXG, "%s: %d groups (1 .. %d)", who, groups, RS_MAXG);
    W2E_REQUIRE(batch >= 1 && batch <= RS_MAXB, "%s: batch %d (1 .. %d)", who, batch, RS_MAXB);
    W2E_REQUIRE(k0 && k1 && n, "%s: null dimension array", who);
    for (int c = 0; c < groups; ++c)
        W2E_REQUIRE(k0[c] >= 1 && k1[c] >= 0 && n[c] >= 1 && k0[c] + k1[c] <= RS_MAXDIM && n[c] <= RS_MAXDIM,
                    "%s: group %d: k0 %d (>= 1), k1 %d (>= 0), n %d (>= 1), k0 + k1 and n at most %d", who, c, k0[c], k1[c], n[c], RS_MAXDIM);
    return 0;
}

extern "C" int w2e_rstyle_linear_fwd(int groups, int batch, const float* const* src0, const float* const* src1, const int* k0,
                                     const int* k1, const int* ld0, const int* ld1, const float* const* w, const float* const* bias,
                                     float* const* out, const int* n, const float* w_scale, float b_scale, const int* act, void* stream) {
    if (rs_check_dims("rstyle_linear_fwd", groups, batch, k0, k1, n)) return 1;
    W2E_REQUIRE(src0 && src1 && ld0 && ld1 && w && out && w_scale && act, "rstyle_linear_fwd: null argument");
    RsGroups g{};
    g.groups = groups, g.batch = batch;
    bool vec = true;
    int nmax = 0;
    for (int c = 0; c < groups; ++c) {
        W2E_REQUIRE(src0[c] && w[c] && out[c] && (k1[c] == 0 || src1[c]), "rstyle_linear_fwd: group %d has a null pointer", c);
        W2E_REQUIRE(ld0[c] >= k0[c] && (k1[c] == 0 || ld1[c] >= k1[c]), "rstyle_linear_fwd: group %d: a row stride is shorter than its row", c);
        g.a0[c] = src0[c], g.a1[c] = k1[c] ? src1[c] : src0[c], g.w[c] = w[c], g.bias[c] = bias ? bias[c] : nullptr, g.o0[c] = out[c];
        g.k0[c] = k0[c], g.k1[c] = k1[c], g.n[c] = n[c], g.ld0[c] = ld0[c], g.ld1[c] = k1[c] ? ld1[c] : 0, g.act[c] = act[c] != 0;
        g.w_scale[c] = w_scale[c];
        vec = vec && !(k0[c] & 3) && !(k1[c] & 3) && !(ld0[c] & 3) && !(g.ld1[c] & 3) && al16(src0[c]) && al16(g.a1[c]) && al16(w[c]);
        nmax = n[c] > nmax ? n[c] : nmax;
    }
    const dim3 grid((unsigned)ceil_div(nmax, 4), (unsigned)groups);
#define RS_FWD(MB)                                                                                \
    if (vec) rs_fwd_kernel<MB, true><<<grid, 256, 0, (hipStream_t)stream>>>(g, b_scale);           \
    else rs_fwd_kernel<MB, false><<<grid, 256, 0, (hipStream_t)stream>>>(g, b_scale)
    RS_BATCH_DISPATCH(batch, RS_FWD);
#undef RS_FWD
    W2E_LAUNCH_CHECK("rstyle_linear_fwd");
    return 0;
}

extern "C" int w2e_rstyle_linear_dgrad(int groups, int batch, const float* const* gy, const float* const* y, const float* const* w,
                                       float* const* gx0, float* const* gx1, const int* k0, const int* k1, const int* n,
                                       const float* w_scale, const int* act, void* stream) {
    if (rs_check_dims("rstyle_linear_dgrad", groups, batch, k0, k1, n)) return 1;
    W2E_REQUIRE(gy && y && w && gx0 && gx1 && w_scale && act, "rstyle_linear_dgrad: null argument");
    RsGroups g{};
    g.groups = groups, g.batch = batch;
    bool vec = true;
    int kmax = 0, nmax = 0;
    for (int c = 0; c < groups; ++c) {
        W2E_REQUIRE(gy[c] && w[c] && (!act[c] || y[c]), "rstyle_linear_dgrad: group %d has a null pointer", c);
        W2E_REQUIRE(gx0[c] || (k1[c] && gx1[c]), "rstyle_linear_dgrad: group %d asks for no gradient", c);
        g.a0[c] = gy[c], g.a1[c] = act[c] ? y[c] : gy[c], g.w[c] = w[c], g.o0[c] = gx0[c], g.o1[c] = k1[c] ? gx1[c] : nullptr;
        g.k0[c] = k0[c], g.k1[c] = k1[c], g.n[c] = n[c], g.act[c] = act[c] != 0, g.w_scale[c] = w_scale[c];
        vec = vec && !((k0[c] + k1[c]) & 3) && al16(w[c]);
        kmax = k0[c] + k1[c] > kmax ? k0[c] + k1[c] : kmax;
        nmax = n[c] > nmax ? n[c] : nmax;
    }
    const dim3 grid((unsigned)ceil_div(kmax, RS_IT), (unsigned)groups);
#define RS_DG(MB)                                                                                                      \
    {                                                                                                                  \
        const size_t lds = sizeof(float) * (size_t)(((batch * nmax + 3) & ~3) + 4 * MB * RS_IT);                       \
        W2E_REQUIRE(lds <= 64 * 1024, "rstyle_linear_dgrad: batch %d x width %d does not fit the staged gradient", batch, nmax); \
        if (vec) rs_dgrad_kernel<MB, true><<<grid, 256, lds, (hipStream_t)stream>>>(g);                                 \
        else rs_dgrad_kernel<MB, false><<<grid, 256, lds, (hipStream_t)stream>>>(g);                                    \
    }
    RS_BATCH_DISPATCH(batch, RS_DG);
#undef RS_DG
    W2E_LAUNCH_CHECK("rstyle_linear_dgrad");
    return 0;
}

extern "C" int w2e_rstyle_linear_wgrad(int groups, int batch, const float* const* gy, const float* const* y, const float* const* src0,
                                       const float* const* src1, const int* k0, const int* k1, const int* ld0, const int* ld1,
                                       float* const* gw, float* const* gb, const int* n, const float* w_scale, float b_scale,
                                       const int* act, void* stream) {
    if (rs_check_dims("rstyle_linear_wgrad", groups, batch, k0, k1, n)) return 1;
    W2E_REQUIRE(gy && y && src0 && src1 && ld0 && ld1 && gw && w_scale && act, "rstyle_linear_wgrad: null argument");
    RsGroups g{};
    g.groups = groups, g.batch = batch;
    bool vec = true;
    int64_t work = 0;
    for (int c = 0; c < groups; ++c) {
        W2E_REQUIRE(gy[c] && src0[c] && gw[c] && (k1[c] == 0 || src1[c]) && (!act[c] || y[c]), "rstyle_linear_wgrad: group %d has a null pointer", c);
        W2E_REQUIRE(ld0[c] >= k0[c] && (k1[c] == 0 || ld1[c] >= k1[c]), "rstyle_linear_wgrad: group %d: a row stride is shorter than its row", c);
        g.bias[c] = gy[c], g.y[c] = act[c] ? y[c] : gy[c], g.a0[c] = src0[c], g.a1[c] = k1[c] ? src1[c] : src0[c];
        g.o0[c] = gw[c], g.o1[c] = gb ? gb[c] : nullptr;
        g.k0[c] = k0[c], g.k1[c] = k1[c], g.n[c] = n[c], g.ld0[c] = ld0[c], g.ld1[c] = k1[c] ? ld1[c] : 0, g.act[c] = act[c] != 0;
        g.w_scale[c] = w_scale[c];
        vec = vec && !(k0[c] & 3) && !(k1[c] & 3) && !(ld0[c] & 3) && !(g.ld1[c] & 3) && al16(src0[c]) && al16(g.a1[c]) && al16(gw[c]);
    }
    for (int c = 0; c < groups; ++c) {
        const int64_t mine = (int64_t)n[c] * ceil_div(k0[c] + k1[c], vec ? 4 : 1);
        work = mine > work ? mine : work;
    }
    const dim3 grid((unsigned)ceil_div(work, 256), (unsigned)groups);
    if (vec) rs_wgrad_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(g, b_scale);
    else rs_wgrad_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(g, b_scale);
    W2E_LAUNCH_CHECK("rstyle_linear_wgrad");
    return 0;
}

static int rs_fill_finish(const char* who, RsFinish& f, int groups, int batch, const float* const* x, const int* ldx, const float* const* y,
                          float* const* out, const int* dims) {
    W2E_REQUIRE(groups >= 1 && groups <= RS_MAXG, "%s: %d groups (1 .. %d)", who, groups, RS_MAXG);
    W2E_REQUIRE(batch >= 1 && batch <= RS_MAXB, "%s: batch %d (1 .. %d)", who, batch, RS_MAXB);
    W2E_REQUIRE(x && ldx && y && out && dims, "%s: null argument", who);
    f.groups = groups, f.batch = batch;
    for (int c = 0; c < groups; ++c) {
        W2E_REQUIRE(dims[c] >= 1 && dims[c] <= RS_MAXDIM && ldx[c] >= dims[c], "%s: group %d: width %d (1 .. %d), row stride %d", who, c, dims[c],
                    RS_MAXDIM, ldx[c]);
        W2E_REQUIRE(x[c] && y[c] && out[c], "%s: group %d has a null pointer", who, c);
        f.x[c] = x[c], f.y[c] = y[c], f.out[c] = out[c], f.go[c] = nullptr, f.d[c] = dims[c], f.ldx[c] = ldx[c];
    }
    return 0;
}

extern "C" int w2e_rstyle_finish_fwd(int groups, int batch, const float* const* x, const int* ldx, const float* const* y, float* const* x_new,
                                     const int* dims, float alpha, int layers, float* norms, float* loss_delta, void* stream) {
    RsFinish f{};
    if (rs_fill_finish("rstyle_finish_fwd", f, groups, batch, x, ldx, y, x_new, dims)) return 1;
    W2E_REQUIRE(norms && loss_delta && layers >= 1, "rstyle_finish_fwd: norms, loss_delta and layers >= 1 are required");
    rs_finish_fwd_kernel<<<dim3((unsigned)ceil_div(batch, 4), (unsigned)groups), 256, 0, (hipStream_t)stream>>>(f, alpha, norms);
    W2E_LAUNCH_CHECK("rstyle_finish_fwd");
    rs_loss_kernel<<<1, 64, 0, (hipStream_t)stream>>>(norms, groups * batch, 1.f / ((float)batch * (float)layers), loss_delta);
    W2E_LAUNCH_CHECK("rstyle_finish_fwd (loss)");
    return 0;
}

extern "C" int w2e_rstyle_finish_bwd(int groups, int batch, const float* const* x, const int* ldx, const float* const* y,
                                     const float* const* g_out, const float* norms, const float* g_loss, float* const* gy, const int* dims,
                                     float alpha, int layers, void* stream) {
    RsFinish f{};
    if (rs_fill_finish("rstyle_finish_bwd", f, groups, batch, x, ldx, y, gy, dims)) return 1;
    W2E_REQUIRE(norms && g_out && layers >= 1, "rstyle_finish_bwd: norms, g_out and layers >= 1 are required");
    int dmax = 0;
    for (int c = 0; c < groups; ++c) f.go[c] = g_out[c], dmax = dims[c] > dmax ? dims[c] : dmax;
    rs_finish_bwd_kernel<<<dim3((unsigned)ceil_div((int64_t)batch * dmax, 256), (unsigned)groups), 256, 0, (hipStream_t)stream>>>(
        f, alpha, 1.f / ((float)batch * (float)layers), norms, g_loss);
    W2E_LAUNCH_CHECK("rstyle_finish_bwd");
    return 0;
}
