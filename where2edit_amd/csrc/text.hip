// The CLIP text tower around the third-generation block kernels (include/w2e_vit.h): the tower itself reuses w2e_gemm_pk,
// w2e_reduce_ln_fwd and w2e_reduce_gelu (vit2.hip, vit3.hip); this file adds what a causal, token-fed tower needs on top.
//   text_embed      x[b*L + l] = E[tokens[b, l]] + P[l]      (int32 or int64 tokens read in place; an id outside the table -> NaN row)
//   attn_causal     softmax(QK^T/8 + triu(-inf, 1)) V per (batch, head), L <= 96, on v_mfma_f32_32x32x2_f32
//   text_pool       the EOT row (first argmax of the tokens) of the last block's output, summed from its slabs, through ln_final
// No atomics, no memsets: every output element is written by exactly one lane, sums run in a fixed order.
#include "device.h"
#include "../../include/w2e_vit.h"

namespace w2e {
namespace text {

__device__ __forceinline__ int64_t token_at(const void* tokens, int token_bytes, int64_t i) {
    return token_bytes == 8 ? reinterpret_cast<const int64_t*>(tokens)[i] : (int64_t)reinterpret_cast<const int32_t*>(tokens)[i];
}

// ------------------------------------------------------------------------------------------ token embedding
__global__ void text_embed_kernel(const void* __restrict__ tokens, int token_bytes, const float* __restrict__ table, int64_t vocab,
                                  const float* __restrict__ pos, float* __restrict__ out, int seq, int dim4, int64_t total4) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += step) {
        const int64_t row = q / dim4;
        const int c = (int)(q - row * dim4);
        const int64_t tok = token_at(tokens, token_bytes, row);
        float4 v;
        if (tok < 0 || tok >= vocab) {  // checked before the table is touched: a bad id never reads outside it
            const float nan = __builtin_nanf("");
            v = make_float4(nan, nan, nan, nan);
        } else {
            const int l = (int)(row % seq);
            v = add4(reinterpret_cast<const float4*>(table)[tok * dim4 + c], reinterpret_cast<const float4*>(pos)[(int64_t)l * dim4 + c]);
        }
        reinterpret_cast<float4*>(out)[q] = v;
    }
}

// ------------------------------------------------------------------------------------------ causal attention on MFMA
// One workgroup (6 waves) per (batch, head); L <= 96 tokens padded to 96, head dim 64.  Q, K, V live in LDS as [96][CS] rows,
// CS = 68 floats, the probabilities P as [96][PS] rows, PS = 100 (16-B aligned rows whose starts fall in 16 different 4-bank
// groups over any 16 consecutive rows: the b128 operand fetches are conflict-free).  S = QK^T has a 3x3 grid of 32x32 blocks of which
// the six on and below the diagonal are live: wave w owns one of them; the three above it are never computed.  O = PV has
// 3x2 blocks of 32x32: wave w owns block (w>>1, w&1) and contracts only over the columns j < 32*(row block + 1).  k-slot
// convention of device.h: lane-half h, group g, component c <-> k = 8g + 4h + c.  Thread t of the 384 stages columns 4*(t&15) .. +3 of
// rows (t>>4) + 24q (load_heads<3, 2, 24, CS>); the softmax runs four adjacent lanes per row, as vit2.hip's softmax_rows.
constexpr int CL = 96, CS = 68, PS = 100, CT = 384;

__global__ __launch_bounds__(CT) void attn_causal_fwd_kernel(const float* __restrict__ qkv, int nsplit, int64_t slab,
                                                             const float* __restrict__ bias, float* __restrict__ out, int L, int H,
                                                             int out_mpad) {
    extern __shared__ __attribute__((aligned(16))) float tsm_[];
    float* q = tsm_;
    float* k = q + CL * CS;
    float* v = k + CL * CS;
    float* p = v + CL * CS;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, j = lane & 31;
    const int ld = 3 * H * 64;
    {
        const int cols[3] = {h * 64, (H + h) * 64, (2 * H + h) * 64};
        float* const dsts[3] = {q, k, v};
        load_heads<3, 2, 24, CS>(qkv, nsplit, slab, bias, (int64_t)b * L, ld, cols, L, dsts);
    }
    __syncthreads();
    // S: live block (bi, bj), bj <= bi, of the lower triangle; a block row at or past L has no row to produce
    {
        const int bi = wave == 0 ? 0 : (wave < 3 ? 1 : 2);
        const int bj = wave - bi * (bi + 1) / 2;
        if (bi * 32 < L) {
            f32x16 acc;
            acc_zero(acc);
            mm_rows_rows<CS, CS>(acc, q, k, bi * 32, bj * 32, j, half);
            acc_to_lds<PS>(acc, p, bi * 32, bj * 32, j, half, 0.125f);
        }
    }
    __syncthreads();
    // softmax of row i over j <= i; P[i][j] = 0 for i < j < 32*(i/32 + 1), the rest of the row's contraction range
    {
        const int i = threadIdx.x >> 2, c = threadIdx.x & 3;
        if (i < L) {  // (uniform over a quad: the DPP reductions stay inside active quads)
            float x[CL / 4];
            float mx = -3.0e38f;
#pragma unroll
            for (int u = 0; u < CL / 4; ++u) {
                const int jj = 4 * u + c;
                x[u] = jj <= i ? p[i * PS + jj] : -3.0e38f;
                mx = fmaxf(mx, x[u]);
            }
            mx = quad_max(mx);
            float sum = 0.f;
#pragma unroll
            for (int u = 0; u < CL / 4; ++u) {
                x[u] = (4 * u + c <= i) ? __expf(x[u] - mx) : 0.f;
                sum += x[u];
            }
            const float inv = 1.f / quad_sum(sum);
            const int width = 32 * (i / 32 + 1);
#pragma unroll
            for (int u = 0; u < CL / 4; ++u)
                if (4 * u + c < width) p[i * PS + 4 * u + c] = x[u] * inv;
        }
    }
    __syncthreads();
    // O block (bi, dj): O[i][d] = sum_{j < 32(bi+1)} P[i][j] V[j][d]
    const int bi = wave >> 1, dj = wave & 1;
    if (bi * 32 >= L) return;
    f32x16 acc;
    acc_zero(acc);
    mm_rows_cols<PS, CS>(acc, p, v, bi * 32, dj * 32, j, half, 4 * (bi + 1));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = bi * 32 + acc_row(r, half);
        if (i >= L) continue;
        const int64_t m = (int64_t)b * L + i;
        const int n = h * 64 + dj * 32 + j;
        if (out_mpad > 0) out[kq_index(m, n, out_mpad)] = acc[r];  // K-quad-major: the out-projection's A operand
        else out[m * (H * 64) + n] = acc[r];
    }
}

// ------------------------------------------------------------------------------------------ EOT pooling + ln_final
// One wave per sequence: the first index of the largest token (torch.argmax), then that row only: sum of the slabs (ascending)
// + bias + residual, LayerNorm, out[b].  dim = 256 * T4.
template <int T4>
__global__ __launch_bounds__(64) void text_pool_kernel(const float* __restrict__ part, int nsplit, int64_t slab, const float* __restrict__ bias,
                                                       const float* __restrict__ residual, const void* __restrict__ tokens, int token_bytes,
                                                       int L, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       float* __restrict__ out, int dim) {
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    int64_t best = INT64_MIN;
    int idx = L;
    for (int l = lane; l < L; l += 64) {
        const int64_t t = token_at(tokens, token_bytes, (int64_t)b * L + l);
        if (t > best) best = t, idx = l;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (ob > best || (ob == best && oi < idx)) best = ob, idx = oi;
    }
    const int64_t row = (int64_t)b * L + idx;  // idx < L: lane 0 always holds position 0
    float4 v[T4];
#pragma unroll
    for (int t = 0; t < T4; ++t) v[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int base = 0; base < nsplit; base += 4) {
        float4 w[4][T4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int t = 0; t < T4; ++t)
                w[c][t] = base + c < nsplit ? reinterpret_cast<const float4*>(part + (base + c) * slab + row * dim)[lane + 64 * t]
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int t = 0; t < T4; ++t) v[t] = add4(v[t], w[c][t]);
    }
    if (bias)
#pragma unroll
        for (int t = 0; t < T4; ++t) v[t] = add4(v[t], reinterpret_cast<const float4*>(bias)[lane + 64 * t]);
    if (residual)
#pragma unroll
        for (int t = 0; t < T4; ++t) v[t] = add4(v[t], reinterpret_cast<const float4*>(residual + row * dim)[lane + 64 * t]);
    float sm = 0.f;
#pragma unroll
    for (int t = 0; t < T4; ++t) sm += (v[t].x + v[t].y) + (v[t].z + v[t].w);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sm += __shfl_xor(sm, off, 64);
    const float mean = sm / dim;
    float sq = 0.f;
#pragma unroll
    for (int t = 0; t < T4; ++t) {
        v[t].x -= mean, v[t].y -= mean, v[t].z -= mean, v[t].w -= mean;
        sq += (v[t].x * v[t].x + v[t].y * v[t].y) + (v[t].z * v[t].z + v[t].w * v[t].w);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
    const float rstd = rsqrtf(sq / dim + eps);
#pragma unroll
    for (int t = 0; t < T4; ++t) {
        const float4 g = reinterpret_cast<const float4*>(gamma)[lane + 64 * t], bt = reinterpret_cast<const float4*>(beta)[lane + 64 * t];
        reinterpret_cast<float4*>(out + (int64_t)b * dim)[lane + 64 * t] =
            make_float4(v[t].x * rstd * g.x + bt.x, v[t].y * rstd * g.y + bt.y, v[t].z * rstd * g.z + bt.z, v[t].w * rstd * g.w + bt.w);
    }
}

}  // namespace text
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_text_embed(const void* tokens, int token_bytes, const float* token_embedding, int64_t vocab, const float* positional,
                              float* out, int batch, int seq, int dim, void* stream) {
    W2E_REQUIRE(tokens && token_embedding && positional && out, "text_embed: null tensor");
    W2E_REQUIRE(token_bytes == 4 || token_bytes == 8, "text_embed: token_bytes %d (4 or 8)", token_bytes);
    W2E_REQUIRE(seq >= 1 && seq <= text::CL && batch >= 0, "text_embed: seq %d (1 .. %d), batch %d", seq, text::CL, batch);
    W2E_REQUIRE(dim == 512 || dim == 768 || dim == 1024, "text_embed: dim %d unsupported (512, 768, 1024)", dim);
    W2E_REQUIRE(vocab >= 1, "text_embed: vocab %lld", (long long)vocab);
    const int64_t total4 = (int64_t)batch * seq * (dim / 4);
    if (total4 == 0) return 0;
    text::text_embed_kernel<<<stream_grid(total4, 256), 256, 0, (hipStream_t)stream>>>(tokens, token_bytes, token_embedding, vocab,
                                                                                      positional, out, seq, dim / 4, total4);
    W2E_LAUNCH_CHECK("text_embed");
    return 0;
}

extern "C" int w2e_attn_causal_fwd(const float* qkv, int nsplit, int64_t slab, const float* bias, float* out, int batch, int seq,
                                   int heads, int out_packed_rows, void* stream) {
    W2E_REQUIRE(qkv && out && nsplit >= 1, "attn_causal_fwd: null tensor / bad split count");
    W2E_REQUIRE(seq >= 1 && seq <= text::CL && batch >= 0, "attn_causal_fwd: seq %d (1 .. %d), batch %d", seq, text::CL, batch);
    W2E_REQUIRE(heads == 8 || heads == 12 || heads == 16, "attn_causal_fwd: width heads*64 = %d unsupported (512, 768, 1024)", heads * 64);
    W2E_REQUIRE(out_packed_rows == 0 || (int64_t)out_packed_rows >= (int64_t)batch * seq, "attn_causal_fwd: out_packed_rows %d for %lld rows",
                out_packed_rows, (long long)batch * seq);
    if (batch == 0) return 0;
    const size_t lds = sizeof(float) * text::CL * (3 * text::CS + text::PS);
    static unsigned done = 0;
    W2E_REQUIRE(big_lds_once((const void*)text::attn_causal_fwd_kernel, &done), "attn_causal_fwd: cannot raise the dynamic LDS limit to %zu B", lds);
    text::attn_causal_fwd_kernel<<<batch * heads, text::CT, lds, (hipStream_t)stream>>>(qkv, nsplit, slab, bias, out, seq, heads, out_packed_rows);
    W2E_LAUNCH_CHECK("attn_causal_fwd");
    return 0;
}

extern "C" int w2e_text_pool(const float* part, int nsplit, int64_t slab, const float* bias, const float* residual, const void* tokens,
                             int token_bytes, int batch, int seq, const float* gamma, const float* beta, float eps, float* out, int dim,
                             void* stream) {
    W2E_REQUIRE(part && tokens && gamma && beta && out && nsplit >= 1, "text_pool: null tensor / bad split count");
    W2E_REQUIRE(token_bytes == 4 || token_bytes == 8, "text_pool: token_bytes %d (4 or 8)", token_bytes);
    W2E_REQUIRE(seq >= 1 && seq <= text::CL && batch >= 0, "text_pool: seq %d (1 .. %d), batch %d", seq, text::CL, batch);
    W2E_REQUIRE(dim == 512 || dim == 768 || dim == 1024, "text_pool: dim %d unsupported (512, 768, 1024)", dim);
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
#define W2E_TPOOL(T) text::text_pool_kernel<T><<<batch, 64, 0, s>>>(part, nsplit, slab, bias, residual, tokens, token_bytes, seq, gamma, beta, eps, out, dim)
    if (dim == 512) W2E_TPOOL(2);
    else if (dim == 768) W2E_TPOOL(3);
    else W2E_TPOOL(4);
#undef W2E_TPOOL
    W2E_LAUNCH_CHECK("text_pool");
    return 0;
}
