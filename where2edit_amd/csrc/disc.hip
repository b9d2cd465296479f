// K8: the two layers of the StyleGAN2 Discriminator that do not run on the conv engine (models/stylegan2/model.py:577-705).
//   fromRGB    ConvLayer(3, C, 1) = EqualConv2d(3, C, 1, bias=False) + FusedLeakyReLU(C) (model.py:614-647, 665): a 1x1 conv with
//              K = 3, which does not fit the engine's 8-channel groups; bound by its C-channel output writes.
//   mbstd      the minibatch-stddev channel (model.py:690-698): one extra channel per sample, the mean over C*H*W of
//              sqrt(var over the group + 1e-8), appended behind the C channels (torch.cat([out, stddev], 1)).
// R1 (the gradient penalty, disc_hip.r1_penalty) adds the forward-mode halves of both -- the fromRGB tangent, the minibatch-stddev
// JVP and the Hessian-vector product of its stddev channel -- and the per-sample sum of squares of the input gradient.
// No atomics, no memsets: every reduction runs in a fixed order, so every result is bit-reproducible and capturable.
#include "device.h"

namespace w2e {

namespace {

constexpr float kSqrt2 = 1.41421356237309504880f;
constexpr int FR_PPT = 4;                  // pixels per thread of the fromRGB backward
constexpr int FR_PPB = 256 * FR_PPT;       // pixels per workgroup (one partial row per workgroup)
constexpr int FR_MAX_C = 512;

// y[b,o,p] = lrelu(scale * sum_i w[o,i] x[b,i,p] + bias[o], 0.2) * sqrt2; one thread per pixel, every output channel.
__global__ __launch_bounds__(256) void fromrgb_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ y, int64_t n, int64_t hw,
                                                          int c, float scale) {
    __shared__ float wl[FR_MAX_C * 4];
    for (int e = threadIdx.x; e < c; e += 256) {
        wl[4 * e + 0] = w[3 * e + 0] * scale;
        wl[4 * e + 1] = w[3 * e + 1] * scale;
        wl[4 * e + 2] = w[3 * e + 2] * scale;
        wl[4 * e + 3] = bias ? bias[e] : 0.f;
    }
    __syncthreads();
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
        const int64_t b = q / hw, p = q - b * hw;
        const float* xb = x + b * 3 * hw + p;
        const float x0 = xb[0], x1 = xb[hw], x2 = xb[2 * hw];
        float* yb = y + b * c * hw + p;
        for (int o = 0; o < c; ++o) {
            float v = ((wl[4 * o] * x0 + wl[4 * o + 1] * x1) + wl[4 * o + 2] * x2) + wl[4 * o + 3];
            v = (v > 0.f ? v : 0.2f * v) * kSqrt2;
            yb[(int64_t)o * hw] = v;
        }
    }
}

// gpre = gy * sqrt2 * (y > 0 ? 1 : 0.2);  gx[b,i,p] = scale * sum_o w[o,i] gpre[b,o,p] (gx may be NULL);
// part[blk][o] = (sum gpre*x0, sum gpre*x1, sum gpre*x2, sum gpre) over the workgroup's FR_PPB pixels (part may be NULL).
__global__ __launch_bounds__(256) void fromrgb_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ y,
                                                          const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ gx,
                                                          float4* __restrict__ part, int64_t n, int64_t hw, int c, float scale) {
    __shared__ float wl[FR_MAX_C * 3];
    __shared__ float4 red[4][FR_MAX_C];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int e = tid; e < 3 * c; e += 256) wl[e] = w[e];
    __syncthreads();
    int64_t off[FR_PPT];
    float xv[FR_PPT][3], ga[FR_PPT][3];
    bool ok[FR_PPT];
#pragma unroll
    for (int j = 0; j < FR_PPT; ++j) {
        const int64_t q = (int64_t)blockIdx.x * FR_PPB + j * 256 + tid;
        ok[j] = q < n;
        const int64_t b = ok[j] ? q / hw : 0, p = ok[j] ? q - b * hw : 0;
        off[j] = b * c * hw + p;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xv[j][i] = ok[j] ? x[b * 3 * hw + i * hw + p] : 0.f;
            ga[j][i] = 0.f;
        }
    }
    for (int o = 0; o < c; ++o) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int j = 0; j < FR_PPT; ++j) {
            if (!ok[j]) continue;
            const int64_t e = off[j] + (int64_t)o * hw;
            const float g = gy[e] * kSqrt2 * (y[e] > 0.f ? 1.f : 0.2f);
            ga[j][0] += wl[3 * o] * g;
            ga[j][1] += wl[3 * o + 1] * g;
            ga[j][2] += wl[3 * o + 2] * g;
            s0 += g * xv[j][0];
            s1 += g * xv[j][1];
            s2 += g * xv[j][2];
            s3 += g;
        }
        if (part) {
            s0 = wave_sum(s0);
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            s3 = wave_sum(s3);
            if (lane == 0) red[wv][o] = make_float4(s0, s1, s2, s3);
        }
    }
    if (gx) {
#pragma unroll
        for (int j = 0; j < FR_PPT; ++j) {
            if (!ok[j]) continue;
            const int64_t q = (int64_t)blockIdx.x * FR_PPB + j * 256 + tid;
            const int64_t b = q / hw, p = q - b * hw;
#pragma unroll
            for (int i = 0; i < 3; ++i) gx[b * 3 * hw + i * hw + p] = scale * ga[j][i];
        }
    }
    if (!part) return;
    __syncthreads();
    for (int o = tid; o < c; o += 256) {
        const float4 a = red[0][o], b4 = red[1][o], c4 = red[2][o], d4 = red[3][o];
        part[(int64_t)blockIdx.x * c + o] = make_float4(((a.x + b4.x) + c4.x) + d4.x, ((a.y + b4.y) + c4.y) + d4.y,
                                                        ((a.z + b4.z) + c4.z) + d4.z, ((a.w + b4.w) + c4.w) + d4.w);
    }
}

// One workgroup per output channel: the partial rows summed in a fixed order -> dw[o,0..2] = scale * ..., db[o] (either may be NULL).
__global__ __launch_bounds__(256) void fromrgb_finish_kernel(const float4* __restrict__ part, int rows, int c, float scale,
                                                             float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float4 red[256];
    const int o = blockIdx.x, tid = threadIdx.x;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = tid; r < rows; r += 256) {
        const float4 v = part[(int64_t)r * c + o];
        a.x += v.x, a.y += v.y, a.z += v.z, a.w += v.w;
    }
    red[tid] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            float4 u = red[tid];
            const float4 v = red[tid + s];
            u.x += v.x, u.y += v.y, u.z += v.z, u.w += v.w;
            red[tid] = u;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float4 r = red[0];
        if (dw) {
            dw[3 * o] = scale * r.x;
            dw[3 * o + 1] = scale * r.y;
            dw[3 * o + 2] = scale * r.z;
        }
        if (db) db[o] = r.w;
    }
}

__device__ float block_sum_256(float v, float* red) {
    const int tid = threadIdx.x;
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup per group member m: samples b = g*M + m (g < group) share one stddev value (view(group, -1, ...), var(0)).
__global__ __launch_bounds__(256) void mbstd_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int group, int m_count,
                                                        int c, int hw) {
    __shared__ float red[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int64_t n = (int64_t)c * hw;
    float acc = 0.f;
    for (int64_t e = tid; e < n; e += 256) {
        float v[4], mean = 0.f;
        for (int g = 0; g < group; ++g) {
            const int64_t b = (int64_t)g * m_count + m;
            v[g] = x[b * n + e];
            y[b * (n + hw) + e] = v[g];
            mean += v[g];
        }
        mean /= (float)group;
        float var = 0.f;
        for (int g = 0; g < group; ++g) var += (v[g] - mean) * (v[g] - mean);
        acc += sqrtf(var / (float)group + 1e-8f);
    }
    const float s = block_sum_256(acc, red) / (float)n;
    for (int e = tid; e < group * hw; e += 256) {
        const int g = e / hw, p = e - g * hw;
        y[((int64_t)g * m_count + m) * (n + hw) + n + p] = s;
    }
}

// gx[b,:C] = gy[b,:C] + gs[m] * (x - mean) / (group * C*H*W * sd),  gs[m] = sum over the group's samples and pixels of gy[b,C].
__global__ __launch_bounds__(256) void mbstd_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ x, float* __restrict__ gx,
                                                        int group, int m_count, int c, int hw) {
    __shared__ float red[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int64_t n = (int64_t)c * hw;
    float gsum = 0.f;
    for (int e = tid; e < group * hw; e += 256) {
        const int g = e / hw, p = e - g * hw;
        gsum += gy[((int64_t)g * m_count + m) * (n + hw) + n + p];
    }
    const float coef = block_sum_256(gsum, red) / ((float)group * (float)n);
    for (int64_t e = tid; e < n; e += 256) {
        float v[4], mean = 0.f;
        for (int g = 0; g < group; ++g) {
            v[g] = x[((int64_t)g * m_count + m) * n + e];
            mean += v[g];
        }
        mean /= (float)group;
        float var = 0.f;
        for (int g = 0; g < group; ++g) var += (v[g] - mean) * (v[g] - mean);
        const float k = coef / sqrtf(var / (float)group + 1e-8f);
        for (int g = 0; g < group; ++g) {
            const int64_t b = (int64_t)g * m_count + m;
            gx[b * n + e] = gy[b * (n + hw) + e] + k * (v[g] - mean);
        }
    }
}

// The tangent of fromrgb_fwd_kernel along dx, from the saved OUTPUT y (its sign is the pre-activation's): no bias, the slope as a mask.
// t[b,o,p] = sqrt2 * (y > 0 ? 1 : 0.2) * scale * sum_i w[o,i] dx[b,i,p]: the C-channel tensor is read once and written once.
__global__ __launch_bounds__(256) void fromrgb_jvp_kernel(const float* __restrict__ dx, const float* __restrict__ y,
                                                          const float* __restrict__ w, float* __restrict__ t, int64_t n, int64_t hw, int c,
                                                          float scale) {
    __shared__ float wl[FR_MAX_C * 3];
    for (int e = threadIdx.x; e < 3 * c; e += 256) wl[e] = w[e] * scale;
    __syncthreads();
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < n; q += (int64_t)gridDim.x * 256) {
        const int64_t b = q / hw, p = q - b * hw;
        const float* xb = dx + b * 3 * hw + p;
        const float x0 = xb[0], x1 = xb[hw], x2 = xb[2 * hw];
        const int64_t base = b * c * hw + p;
        for (int o = 0; o < c; ++o) {
            const int64_t e = base + (int64_t)o * hw;
            const float v = (wl[3 * o] * x0 + wl[3 * o + 1] * x1) + wl[3 * o + 2] * x2;
            t[e] = v * (y[e] > 0.f ? kSqrt2 : 0.2f * kSqrt2);
        }
    }
}

// The tangent of mbstd_fwd_kernel along dx: y[b,:C] = dx[b]; y[b,C,:] = the mean over C*hw of sum_g (x_g - mean)(dx_g) / (group * sd).
__global__ __launch_bounds__(256) void mbstd_jvp_kernel(const float* __restrict__ x, const float* __restrict__ dx, float* __restrict__ y,
                                                        int group, int m_count, int c, int hw) {
    __shared__ float red[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int64_t n = (int64_t)c * hw;
    float acc = 0.f;
    for (int64_t e = tid; e < n; e += 256) {
        float v[4], d[4], mean = 0.f;
        for (int g = 0; g < group; ++g) {
            const int64_t b = (int64_t)g * m_count + m;
            v[g] = x[b * n + e];
            d[g] = dx[b * n + e];
            y[b * (n + hw) + e] = d[g];
            mean += v[g];
        }
        mean /= (float)group;
        float var = 0.f, dot = 0.f;
        for (int g = 0; g < group; ++g) {
            var += (v[g] - mean) * (v[g] - mean);
            dot += (v[g] - mean) * d[g];
        }
        acc += dot / ((float)group * sqrtf(var / (float)group + 1e-8f));
    }
    const float s = block_sum_256(acc, red) / (float)n;
    for (int e = tid; e < group * hw; e += 256) {
        const int g = e / hw, p = e - g * hw;
        y[((int64_t)g * m_count + m) * (n + hw) + n + p] = s;
    }
}

// mu[b] = d/dx[b] of <gy[:, C], stddev tangent(x, dx)>: with k = gs[m] / (group * C*hw) (gs as in mbstd_bwd_kernel), c_g = x_g - mean,
// P = sum_g c_g dx_g:  mu_g = k * ((dx_g - mean(dx)) / sd - P c_g / (group * sd^3)).
__global__ __launch_bounds__(256) void mbstd_hvp_kernel(const float* __restrict__ gy, const float* __restrict__ x,
                                                        const float* __restrict__ dx, float* __restrict__ mu, int group, int m_count, int c,
                                                        int hw) {
    __shared__ float red[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int64_t n = (int64_t)c * hw;
    float gsum = 0.f;
    for (int e = tid; e < group * hw; e += 256) {
        const int g = e / hw, p = e - g * hw;
        gsum += gy[((int64_t)g * m_count + m) * (n + hw) + n + p];
    }
    const float coef = block_sum_256(gsum, red) / ((float)group * (float)n);
    for (int64_t e = tid; e < n; e += 256) {
        float v[4], d[4], mean = 0.f, dmean = 0.f;
        for (int g = 0; g < group; ++g) {
            const int64_t b = (int64_t)g * m_count + m;
            v[g] = x[b * n + e];
            d[g] = dx[b * n + e];
            mean += v[g];
            dmean += d[g];
        }
        mean /= (float)group;
        dmean /= (float)group;
        float var = 0.f, dot = 0.f;
        for (int g = 0; g < group; ++g) {
            var += (v[g] - mean) * (v[g] - mean);
            dot += (v[g] - mean) * (d[g] - dmean);
        }
        const float sd2 = var / (float)group + 1e-8f;
        const float k1 = coef / sqrtf(sd2), k2 = k1 * dot / ((float)group * sd2);
        for (int g = 0; g < group; ++g) mu[((int64_t)g * m_count + m) * n + e] = k1 * (d[g] - dmean) - k2 * (v[g] - mean);
    }
}

constexpr int SQ_PER_THREAD = 16;
constexpr int SQ_CHUNK = 256 * SQ_PER_THREAD;  // elements per workgroup of the first stage

// Stage 1: part[b][k] = sum of x^2 over chunk k of row b (thread-strided, then the wave / workgroup tree: one fixed order).
__global__ __launch_bounds__(256) void sumsq_part_kernel(const float* __restrict__ x, float* __restrict__ part, int64_t n, int chunks) {
    __shared__ float red[4];
    const int64_t row = blockIdx.y, first = (int64_t)blockIdx.x * SQ_CHUNK;
    const float* xr = x + row * n;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < SQ_PER_THREAD; ++j) {
        const int64_t e = first + j * 256 + threadIdx.x;
        const float v = e < n ? xr[e] : 0.f;
        acc += v * v;
    }
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[row * chunks + blockIdx.x] = s;
}

// Stage 2: one workgroup per row sums its partials in a fixed order.
__global__ __launch_bounds__(256) void sumsq_finish_kernel(const float* __restrict__ part, float* __restrict__ out, int chunks) {
    __shared__ float red[4];
    const float* pr = part + (int64_t)blockIdx.x * chunks;
    float acc = 0.f;
    for (int k = threadIdx.x; k < chunks; k += 256) acc += pr[k];
    const float s = block_sum_256(acc, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

int mbstd_group(int batch) { return batch < 4 ? batch : 4; }

}  // namespace

}  // namespace w2e

using namespace w2e;

extern "C" {

int w2e_fromrgb_fwd(const float* x, const float* weight, const float* bias, float* y, int batch, int channels, int64_t hw, float scale,
                    void* stream) {
    W2E_REQUIRE(x && weight && y, "fromrgb_fwd: null tensor");
    W2E_REQUIRE(batch >= 0 && channels > 0 && channels <= FR_MAX_C && hw > 0, "fromrgb_fwd: bad dims (channels <= %d)", FR_MAX_C);
    const int64_t n = (int64_t)batch * hw;
    if (n == 0) return 0;
    fromrgb_fwd_kernel<<<stream_grid(n, 256), 256, 0, (hipStream_t)stream>>>(x, weight, bias, y, n, hw, channels, scale);
    W2E_LAUNCH_CHECK("fromrgb_fwd");
    return 0;
}

int w2e_fromrgb_bwd_rows(int batch, int64_t hw) { return (int)ceil_div((int64_t)batch * hw, FR_PPB); }

int w2e_fromrgb_bwd(const float* gy, const float* y, const float* x, const float* weight, float* gx, float* part, float* dw, float* db,
                    int batch, int channels, int64_t hw, float scale, void* stream) {
    W2E_REQUIRE(gy && y && x && weight, "fromrgb_bwd: null tensor");
    W2E_REQUIRE(batch > 0 && channels > 0 && channels <= FR_MAX_C && hw > 0, "fromrgb_bwd: bad dims (channels <= %d)", FR_MAX_C);
    W2E_REQUIRE(!(dw || db) || part, "fromrgb_bwd: dw / db need the partials workspace");
    const int64_t rows = ceil_div((int64_t)batch * hw, FR_PPB);
    W2E_REQUIRE(rows < (1ll << 31), "fromrgb_bwd: too large");
    hipStream_t st = (hipStream_t)stream;
    float4* p4 = (dw || db) ? reinterpret_cast<float4*>(part) : nullptr;
    W2E_REQUIRE(!p4 || ((uintptr_t)part & 15) == 0, "fromrgb_bwd: part must be 16-byte aligned");
    if (!gx && !p4) return 0;
    fromrgb_bwd_kernel<<<(unsigned)rows, 256, 0, st>>>(gy, y, x, weight, gx, p4, (int64_t)batch * hw, hw, channels, scale);
    W2E_LAUNCH_CHECK("fromrgb_bwd");
    if (p4) {
        fromrgb_finish_kernel<<<(unsigned)channels, 256, 0, st>>>(p4, (int)rows, channels, scale, dw, db);
        W2E_LAUNCH_CHECK("fromrgb_bwd (finish)");
    }
    return 0;
}

int w2e_mbstd_fwd(const float* x, float* y, int batch, int channels, int hw, void* stream) {
    W2E_REQUIRE(x && y, "mbstd_fwd: null tensor");
    W2E_REQUIRE(batch > 0 && channels > 0 && hw > 0 && (int64_t)channels * hw < (1ll << 31), "mbstd_fwd: bad dims");
    const int group = mbstd_group(batch);
    W2E_REQUIRE(batch % group == 0, "mbstd_fwd: batch %d is not a multiple of the stddev group min(batch, 4) = %d", batch, group);
    mbstd_fwd_kernel<<<(unsigned)(batch / group), 256, 0, (hipStream_t)stream>>>(x, y, group, batch / group, channels, hw);
    W2E_LAUNCH_CHECK("mbstd_fwd");
    return 0;
}

int w2e_mbstd_bwd(const float* gy, const float* x, float* gx, int batch, int channels, int hw, void* stream) {
    W2E_REQUIRE(gy && x && gx, "mbstd_bwd: null tensor");
    W2E_REQUIRE(batch > 0 && channels > 0 && hw > 0 && (int64_t)channels * hw < (1ll << 31), "mbstd_bwd: bad dims");
    const int group = mbstd_group(batch);
    W2E_REQUIRE(batch % group == 0, "mbstd_bwd: batch %d is not a multiple of the stddev group min(batch, 4) = %d", batch, group);
    mbstd_bwd_kernel<<<(unsigned)(batch / group), 256, 0, (hipStream_t)stream>>>(gy, x, gx, group, batch / group, channels, hw);
    W2E_LAUNCH_CHECK("mbstd_bwd");
    return 0;
}

int w2e_fromrgb_jvp(const float* dx, const float* y, const float* weight, float* t, int batch, int channels, int64_t hw, float scale,
                    void* stream) {
    W2E_REQUIRE(dx && y && weight && t, "fromrgb_jvp: null tensor");
    W2E_REQUIRE(batch > 0 && channels > 0 && channels <= FR_MAX_C && hw > 0, "fromrgb_jvp: bad dims (channels <= %d)", FR_MAX_C);
    const int64_t n = (int64_t)batch * hw;
    fromrgb_jvp_kernel<<<stream_grid(n, 256), 256, 0, (hipStream_t)stream>>>(dx, y, weight, t, n, hw, channels, scale);
    W2E_LAUNCH_CHECK("fromrgb_jvp");
    return 0;
}

int w2e_mbstd_jvp(const float* x, const float* dx, float* y, int batch, int channels, int hw, void* stream) {
    W2E_REQUIRE(x && dx && y, "mbstd_jvp: null tensor");
    W2E_REQUIRE(batch > 0 && channels > 0 && hw > 0 && (int64_t)channels * hw < (1ll << 31), "mbstd_jvp: bad dims");
    const int group = mbstd_group(batch);
    W2E_REQUIRE(batch % group == 0, "mbstd_jvp: batch %d is not a multiple of the stddev group min(batch, 4) = %d", batch, group);
    mbstd_jvp_kernel<<<(unsigned)(batch / group), 256, 0, (hipStream_t)stream>>>(x, dx, y, group, batch / group, channels, hw);
    W2E_LAUNCH_CHECK("mbstd_jvp");
    return 0;
}

int w2e_mbstd_hvp(const float* gy, const float* x, const float* dx, float* mu, int batch, int channels, int hw, void* stream) {
    W2E_REQUIRE(gy && x && dx && mu, "mbstd_hvp: null tensor");
    W2E_REQUIRE(batch > 0 && channels > 0 && hw > 0 && (int64_t)channels * hw < (1ll << 31), "mbstd_hvp: bad dims");
    const int group = mbstd_group(batch);
    W2E_REQUIRE(batch % group == 0, "mbstd_hvp: batch %d is not a multiple of the stddev group min(batch, 4) = %d", batch, group);
    mbstd_hvp_kernel<<<(unsigned)(batch / group), 256, 0, (hipStream_t)stream>>>(gy, x, dx, mu, group, batch / group, channels, hw);
    W2E_LAUNCH_CHECK("mbstd_hvp");
    return 0;
}

int w2e_sumsq_rows_parts(int64_t n) { return n > 0 && n < (int64_t)SQ_CHUNK * 65535 ? (int)ceil_div(n, SQ_CHUNK) : 0; }

int w2e_sumsq_rows(const float* x, float* part, float* out, int batch, int64_t n, void* stream) {
    W2E_REQUIRE(x && part && out, "sumsq_rows: null tensor");
    W2E_REQUIRE(batch > 0 && batch <= 65535 && n > 0, "sumsq_rows: bad dims (0 < batch <= 65535, n > 0)");
    const int chunks = w2e_sumsq_rows_parts(n);
    W2E_REQUIRE(chunks > 0, "sumsq_rows: row too long");
    hipStream_t st = (hipStream_t)stream;
    sumsq_part_kernel<<<dim3((unsigned)chunks, (unsigned)batch), 256, 0, st>>>(x, part, n, chunks);
    W2E_LAUNCH_CHECK("sumsq_rows");
    sumsq_finish_kernel<<<(unsigned)batch, 256, 0, st>>>(part, out, chunks);
    W2E_LAUNCH_CHECK("sumsq_rows (finish)");
    return 0;
}

}  // extern "C"
