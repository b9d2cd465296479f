// Device-side helpers shared by the kernels of libw2e.so: the wave / quad reductions and the v_mfma_f32_32x32x2_f32 attention building
// blocks of the CLIP towers (vit2.hip, text.hip).  Each rule that several kernels must agree on -- the accumulator layout, the
// packed-operand index, the slab order of the QKV loader -- is written here once.
// (Not here on purpose: the one-wave-per-row slab sum and LayerNorm arithmetic of vit.hip / vit2.hip / text.hip.  Behind a helper the
// compiler contracts the other product of each x*x + y*y pair, which changes the last bit of the variance: DESIGN.md, K8-K10.)
#pragma once
#include "common.h"

namespace w2e {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------ wave and quad reductions
// 64-lane xor butterfly: every lane ends with the reduction of all 64, in one fixed order.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the same butterfly on counters: integer addition commutes, so the order is no concern here
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
    return v;
}
// inclusive prefix sum over the 64 lanes (lane 63 ends with the wave's sum): six shift-and-add steps
__device__ __forceinline__ unsigned wave_scan_inclusive(unsigned v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// Four adjacent lanes: two DPP quad permutes instead of ds_bpermute steps.
__device__ __forceinline__ float quad_xor1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
}
__device__ __forceinline__ float quad_xor2(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
}
__device__ __forceinline__ float quad_sum(float v) {
    v += quad_xor1(v);
    return v + quad_xor2(v);
}
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, quad_xor1(v));
    return fmaxf(v, quad_xor2(v));
}

__device__ __forceinline__ float4 add4(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// F.interpolate(mode='nearest') source index, as torch computes it: in fp32, with scale = (float)in / (float)out.  The exact-integer
// floor(dst * in / out) reads a neighbouring pixel at some ratios that are no power of two (26 -> 22: destination 11).  Used by the
// mask blend (elementwise.hip) and by every gather of the region-attention mask kernels (attention.hip, attention_bwd.hip).
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) {
    // torch nearest: min(floor(dst * (in/out)), in-1)  (attention_model.py:548 uses the default mode)
    const int s = (int)floorf(dst * scale);
    return s < in_size - 1 ? s : in_size - 1;
}

__device__ __forceinline__ float quick_gelu(float x) { return x / (1.f + __expf(-1.702f * x)); }
__device__ __forceinline__ float quick_gelu_grad(float x) {
    const float s = 1.f / (1.f + __expf(-1.702f * x));
    return s * (1.f + 1.702f * x * (1.f - s));
}

// ------------------------------------------------------------------------------------------ attention on MFMA
// Every contraction runs on v_mfma_f32_32x32x2_f32 over LDS matrices whose rows are SA / SB floats apart; a wave owns one 32x32
// output block.  k-slot convention (same for both operands): lane-half h, group g, component c <-> k = 8g + 4h + c.
// Accumulator register r of lane (half, j) is row acc_row(r, half), column j of the block.
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// Element (m, n) of a matrix stored K-quad-major with mpad rows, P[n / 4][m][n % 4]: the operand packing of w2e_gemm_pk (vit3.hip).
__device__ __forceinline__ int64_t kq_index(int64_t m, int n, int mpad) { return ((int64_t)(n >> 2) * mpad + m) * 4 + (n & 3); }

__device__ __forceinline__ void acc_zero(f32x16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}
// scatter a wave's 32x32 accumulator block, scaled, into an LDS matrix with rows of S floats
template <int S>
__device__ __forceinline__ void acc_to_lds(const f32x16& a, float* M, int i0, int j0, int j, int half, float scale) {
#pragma unroll
    for (int r = 0; r < 16; ++r) M[(i0 + acc_row(r, half)) * S + j0 + j] = a[r] * scale;
}

// acc += A_rows . B_rows^T over 64 k: out[i][j] = sum_k A[i][k] B[j][k]   (both operands row-major, k along the row: b128 fetches)
template <int SA, int SB>
__device__ __forceinline__ void mm_rows_rows(f32x16& acc, const float* A, const float* B, int i0, int j0, int j, int half) {
    const float4* ar = reinterpret_cast<const float4*>(A + (i0 + j) * SA) + half;
    const float4* br = reinterpret_cast<const float4*>(B + (j0 + j) * SB) + half;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const float4 a4 = ar[2 * g], b4 = br[2 * g];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
    }
}
// acc += A . B over k < 8 * groups: out[i][n] = sum_k A[i][k] B[k][n]   (A row-major b128; B read down its rows, lanes along n).
// G > 0: the group count at compile time (fully unrolled); G = 0: the runtime bound `groups` (the causal tower's live columns).
template <int SA, int SB, int G = 0>
__device__ __forceinline__ void mm_rows_cols(f32x16& acc, const float* A, const float* B, int i0, int n0, int j, int half, int groups = G) {
    const float4* ar = reinterpret_cast<const float4*>(A + (i0 + j) * SA) + half;
    const float* bc = B + n0 + j;
    const auto group = [&](int g) {
        const float4 a4 = ar[2 * g];
        const int k = 8 * g + 4 * half;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, bc[(k + 0) * SB], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, bc[(k + 1) * SB], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, bc[(k + 2) * SB], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, bc[(k + 3) * SB], acc, 0, 0, 0);
    };
    if constexpr (G > 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) group(g);
    } else {
        for (int g = 0; g < groups; ++g) group(g);
    }
}
// acc += A^T . B : out[m][n] = sum_k A[k][m] B[k][n]   (both read down their rows)
template <int SA, int SB>
__device__ __forceinline__ void mm_cols_cols(f32x16& acc, const float* A, const float* B, int m0, int n0, int j, int half) {
    const float* ac = A + m0 + j;
    const float* bc = B + n0 + j;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const int k = 8 * g + 4 * half;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[(k + c) * SA], bc[(k + c) * SB], acc, 0, 0, 0);
    }
}

// NH heads' worth of [L x 64] blocks (column offsets col[0..NH-1]) of a [B*L, ld] matrix given as nsplit slabs (+ bias) -> LDS
// [4 * ROW_STEP][STRIDE] images dst[0..NH-1], zero rows >= L.  A workgroup of 16 * ROW_STEP threads: thread = columns d..d+3, rows
// t0 + ROW_STEP * q.  Loop order: slab outermost (ascending, as in every consumer of split-K slabs), the thread's 4*NH float4s inside, CH slabs per
// pass -- all 4*NH*CH loads of a pass are issued before the first add (a per-element slab loop would chain nsplit*4*NH load
// latencies: measured 18 us of the 22 us the visual kernel took).
template <int NH, int CH, int ROW_STEP, int STRIDE>
__device__ __forceinline__ void load_heads(const float* src, int nsplit, int64_t slab, const float* bias, int64_t row0, int ld,
                                           const int (&col)[NH], int L, float* const (&dst)[NH]) {
    float4 v[NH][4];
    const int d = (threadIdx.x & 15) * 4, t0 = threadIdx.x >> 4;
#pragma unroll
    for (int a = 0; a < NH; ++a)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[a][q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = 0; base < nsplit; base += CH) {
        float4 w[CH][NH][4];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int a = 0; a < NH; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int t = t0 + ROW_STEP * q;
                    w[c][a][q] = (base + c < nsplit && t < L)
                                     ? *reinterpret_cast<const float4*>(src + (base + c) * slab + (row0 + t) * ld + col[a] + d)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int a = 0; a < NH; ++a)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[a][q] = add4(v[a][q], w[c][a][q]);
    }
#pragma unroll
    for (int a = 0; a < NH; ++a) {
        const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + col[a] + d) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = t0 + ROW_STEP * q;
            *reinterpret_cast<float4*>(dst[a] + t * STRIDE + d) = t < L ? add4(v[a][q], bv) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

}  // namespace w2e
