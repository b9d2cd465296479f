// The kernels of the VGG16 perceptual loss (criteria/perceptual_loss.py) that the IR-SE50 set does not already cover
// (include/w2e_irse.h): 2x2 max-pooling forward, its backward with the preceding ReLU folded in, and the MSE loss head
// with relu2_2's ReLU mask folded into its gradient.  All three are memory-bound; the 3x3 convolutions run on
// w2e_conv3x3 (modconv.hip / the Winograd forms).
#include "../../include/w2e_irse.h"
#include "device.h"

namespace w2e {

// PyTorch's max_pool2d rule: scan the window in row-major order and take a value when it is greater than the running
// maximum or NaN -- the first of equal maxima wins, a NaN propagates (the last NaN of the window is the arg-max).
__device__ __forceinline__ void max_take(float v, int i, float& m, int& idx) {
    if (v > m || v != v) m = v, idx = i;
}

__device__ __forceinline__ int window_argmax(float a, float b, float c, float d, float& m) {
    int idx = 0;
    m = a;
    max_take(b, 1, m, idx);
    max_take(c, 2, m, idx);
    max_take(d, 3, m, idx);
    return idx;
}

// W % 4 == 0: one thread per (plane, output row, pair of output columns): two float4 loads (one per input row), one float2 store.
__global__ void maxpool2x2_fwd_vec_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int OH, int64_t items) {
    const int quads = W >> 2, OW = W >> 1;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += step) {
        const int q = (int)(it % quads);
        const int64_t pr = it / quads;  // plane * OH + output row
        const int r = (int)(pr % OH);
        const int64_t plane = pr / OH;
        const float* row0 = x + (plane * H + 2 * r) * (int64_t)W;
        const float4 u = reinterpret_cast<const float4*>(row0)[q];
        const float4 v = reinterpret_cast<const float4*>(row0 + W)[q];
        float2 o;
        window_argmax(u.x, u.y, v.x, v.y, o.x);
        window_argmax(u.z, u.w, v.z, v.w, o.y);
        reinterpret_cast<float2*>(y + pr * OW)[q] = o;
    }
}

// Any W: one thread per output element.
__global__ void maxpool2x2_fwd_scalar_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int OH, int OW,
                                             int64_t total) {
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const int ox = (int)(e % OW);
        const int64_t pr = e / OW;
        const int r = (int)(pr % OH);
        const int64_t plane = pr / OH;
        const float* p = x + (plane * H + 2 * r) * (int64_t)W + 2 * ox;
        float m;
        window_argmax(p[0], p[1], p[W], p[W + 1], m);
        y[e] = m;
    }
}

// gx = [relu: y > 0] * (position is its window's arg-max ? g : 0); the row / column dropped by flooring get 0.
// W % 4 == 0: one thread per (plane, input row pair, 4 input columns) -- ceil(H/2) row pairs, the last one of an odd H is the
// dropped row (zeros) -- two float4 loads of y, one float2 load of g, two float4 stores.
__global__ void maxpool2x2_bwd_vec_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ gx, int H, int W,
                                          int OH, int relu, int64_t items) {
    const int quads = W >> 2, OW = W >> 1, RP = (H + 1) >> 1;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += step) {
        const int q = (int)(it % quads);
        const int64_t pr = it / quads;
        const int r = (int)(pr % RP);
        const int64_t plane = pr / RP;
        const int64_t off0 = (plane * H + 2 * r) * (int64_t)W;
        if (r >= OH) {  // the dropped last row of an odd H
            reinterpret_cast<float4*>(gx + off0)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        const float4 u = reinterpret_cast<const float4*>(y + off0)[q];
        const float4 v = reinterpret_cast<const float4*>(y + off0 + W)[q];
        const float2 gg = reinterpret_cast<const float2*>(g + (plane * OH + r) * (int64_t)OW)[q];
        float m;
        const int i0 = window_argmax(u.x, u.y, v.x, v.y, m);
        const int i1 = window_argmax(u.z, u.w, v.z, v.w, m);
        float4 a = make_float4(i0 == 0 ? gg.x : 0.f, i0 == 1 ? gg.x : 0.f, i1 == 0 ? gg.y : 0.f, i1 == 1 ? gg.y : 0.f);
        float4 b = make_float4(i0 == 2 ? gg.x : 0.f, i0 == 3 ? gg.x : 0.f, i1 == 2 ? gg.y : 0.f, i1 == 3 ? gg.y : 0.f);
        if (relu) {
            a.x = u.x > 0.f ? a.x : 0.f, a.y = u.y > 0.f ? a.y : 0.f, a.z = u.z > 0.f ? a.z : 0.f, a.w = u.w > 0.f ? a.w : 0.f;
            b.x = v.x > 0.f ? b.x : 0.f, b.y = v.y > 0.f ? b.y : 0.f, b.z = v.z > 0.f ? b.z : 0.f, b.w = v.w > 0.f ? b.w : 0.f;
        }
        reinterpret_cast<float4*>(gx + off0)[q] = a;
        if (2 * r + 1 < H) reinterpret_cast<float4*>(gx + off0 + W)[q] = b;
    }
}

// Any W: one thread per 2x2 window of the ceil(H/2) x ceil(W/2) cover; windows past the floor write zeros to what they hold.
__global__ void maxpool2x2_bwd_scalar_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ gx, int H, int W,
                                             int OH, int OW, int relu, int64_t total) {
    const int CH = (H + 1) >> 1, CW = (W + 1) >> 1;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const int cx = (int)(e % CW);
        const int64_t pr = e / CW;
        const int r = (int)(pr % CH);
        const int64_t plane = pr / CH;
        const int64_t off = (plane * H + 2 * r) * (int64_t)W + 2 * cx;
        if (r >= OH || cx >= OW) {
            gx[off] = 0.f;
            if (2 * cx + 1 < W) gx[off + 1] = 0.f;
            if (2 * r + 1 < H) {
                gx[off + W] = 0.f;
                if (2 * cx + 1 < W) gx[off + W + 1] = 0.f;
            }
            continue;
        }
        const float v0 = y[off], v1 = y[off + 1], v2 = y[off + W], v3 = y[off + W + 1];
        float m;
        const int i = window_argmax(v0, v1, v2, v3, m);
        const float gv = g[(plane * OH + r) * (int64_t)OW + cx];
        float o0 = i == 0 ? gv : 0.f, o1 = i == 1 ? gv : 0.f, o2 = i == 2 ? gv : 0.f, o3 = i == 3 ? gv : 0.f;
        if (relu) {
            o0 = v0 > 0.f ? o0 : 0.f, o1 = v1 > 0.f ? o1 : 0.f, o2 = v2 > 0.f ? o2 : 0.f, o3 = v3 > 0.f ? o3 : 0.f;
        }
        gx[off] = o0, gx[off + 1] = o1, gx[off + W] = o2, gx[off + W + 1] = o3;
    }
}

constexpr int MSE_BLOCK = 256;

// Fixed-order block sum (wave shuffles, then wave 0 over the 4 wave sums); the result is valid in thread 0.
__device__ __forceinline__ float block_sum_vgg(float v, float* sm) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sm[wave] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    return r;
}

// Pass 1: every block strides the float4 groups of f1 (per_sample % 4 == 0, so a group never straddles two samples and the
// broadcast target is read at e % per_sample) and leaves its sum of squared differences in partials[block]; with gpre1 /
// gpre2 it also writes the two sides' gradients (the ReLU mask of the side they belong to folded in).
__global__ __launch_bounds__(MSE_BLOCK) void mse_relu_vec_kernel(const float* __restrict__ f1, const float* __restrict__ f2,
                                                                  int64_t per4, int bcast, float scale, float* __restrict__ gpre1,
                                                                  float* __restrict__ gpre2, float* __restrict__ partials, int64_t total4) {
    __shared__ float sm[MSE_BLOCK / 64];
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    float acc = 0.f;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4; q += step) {
        const float4 a = reinterpret_cast<const float4*>(f1)[q];
        const float4 b = reinterpret_cast<const float4*>(f2)[bcast ? q % per4 : q];
        const float4 d = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
        acc += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        if (gpre1) {
            reinterpret_cast<float4*>(gpre1)[q] = make_float4(a.x > 0.f ? scale * d.x : 0.f, a.y > 0.f ? scale * d.y : 0.f,
                                                              a.z > 0.f ? scale * d.z : 0.f, a.w > 0.f ? scale * d.w : 0.f);
        }
        if (gpre2) {
            reinterpret_cast<float4*>(gpre2)[q] = make_float4(b.x > 0.f ? -scale * d.x : 0.f, b.y > 0.f ? -scale * d.y : 0.f,
                                                              b.z > 0.f ? -scale * d.z : 0.f, b.w > 0.f ? -scale * d.w : 0.f);
        }
    }
    const float s = block_sum_vgg(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(MSE_BLOCK) void mse_relu_scalar_kernel(const float* __restrict__ f1, const float* __restrict__ f2,
                                                                     int64_t per, int bcast, float scale, float* __restrict__ gpre1,
                                                                     float* __restrict__ gpre2, float* __restrict__ partials,
                                                                     int64_t total) {
    __shared__ float sm[MSE_BLOCK / 64];
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    float acc = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const float a = f1[e], b = f2[bcast ? e % per : e];
        const float d = a - b;
        acc += d * d;
        if (gpre1) gpre1[e] = a > 0.f ? scale * d : 0.f;
        if (gpre2) gpre2[e] = b > 0.f ? -scale * d : 0.f;
    }
    const float s = block_sum_vgg(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// Pass 2: one block sums the partials in a fixed order and writes loss = sum * inv_n.
__global__ __launch_bounds__(MSE_BLOCK) void mse_final_kernel(const float* __restrict__ partials, int n, float inv_n,
                                                               float* __restrict__ loss) {
    __shared__ float sm[MSE_BLOCK / 64];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += MSE_BLOCK) acc += partials[i];
    const float s = block_sum_vgg(acc, sm);
    if (threadIdx.x == 0) loss[0] = s * inv_n;
}

}  // namespace w2e

using namespace w2e;

extern "C" int w2e_maxpool2x2_fwd(const float* x, float* y, int64_t planes, int height, int width, void* stream) {
    W2E_REQUIRE(x && y, "maxpool2x2_fwd: null tensor");
    W2E_REQUIRE(planes >= 0, "maxpool2x2_fwd: planes %lld < 0", (long long)planes);
    W2E_REQUIRE(height >= 2 && width >= 2, "maxpool2x2_fwd: a %dx%d image has no 2x2 window", height, width);
    const int oh = height / 2, ow = width / 2;
    if (planes == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    if ((width & 3) == 0) {
        const int64_t items = planes * oh * (width / 4);
        maxpool2x2_fwd_vec_kernel<<<stream_grid(items, 256), 256, 0, s>>>(x, y, height, width, oh, items);
    } else {
        const int64_t total = planes * oh * ow;
        maxpool2x2_fwd_scalar_kernel<<<stream_grid(total, 256), 256, 0, s>>>(x, y, height, width, oh, ow, total);
    }
    W2E_LAUNCH_CHECK("maxpool2x2_fwd");
    return 0;
}

extern "C" int w2e_maxpool2x2_relu_bwd(const float* g, const float* y, float* gx, int64_t planes, int height, int width, int relu,
                                       void* stream) {
    W2E_REQUIRE(g && y && gx, "maxpool2x2_relu_bwd: null tensor");
    W2E_REQUIRE(planes >= 0, "maxpool2x2_relu_bwd: planes %lld < 0", (long long)planes);
    W2E_REQUIRE(height >= 2 && width >= 2, "maxpool2x2_relu_bwd: a %dx%d image has no 2x2 window", height, width);
    if (planes == 0) return 0;
    const int oh = height / 2, ow = width / 2;
    hipStream_t s = (hipStream_t)stream;
    if ((width & 3) == 0) {
        const int64_t items = planes * ((height + 1) / 2) * (width / 4);
        maxpool2x2_bwd_vec_kernel<<<stream_grid(items, 256), 256, 0, s>>>(g, y, gx, height, width, oh, relu ? 1 : 0, items);
    } else {
        const int64_t total = planes * ((height + 1) / 2) * ((width + 1) / 2);
        maxpool2x2_bwd_scalar_kernel<<<stream_grid(total, 256), 256, 0, s>>>(g, y, gx, height, width, oh, ow, relu ? 1 : 0, total);
    }
    W2E_LAUNCH_CHECK("maxpool2x2_relu_bwd");
    return 0;
}

extern "C" int w2e_mse_relu_fwd(const float* f1, const float* f2, int batch, int batch2, int64_t per_sample, float* gpre1, float* gpre2,
                                float* partials, int n_partials, float* loss, void* stream) {
    W2E_REQUIRE(f1 && f2 && partials && loss, "mse_relu_fwd: null tensor");
    W2E_REQUIRE(batch >= 1 && per_sample >= 1, "mse_relu_fwd: bad size (batch %d, per_sample %lld)", batch, (long long)per_sample);
    W2E_REQUIRE(batch2 == batch || batch2 == 1, "mse_relu_fwd: target batch %d is neither %d nor 1", batch2, batch);
    W2E_REQUIRE(!(gpre2 && batch2 != batch), "mse_relu_fwd: gpre2 (the target's gradient) needs equal batches");
    W2E_REQUIRE(n_partials >= W2E_MSE_PARTIALS, "mse_relu_fwd: the partials slab holds %d floats, needs %d", n_partials, W2E_MSE_PARTIALS);
    const int64_t total = (int64_t)batch * per_sample;
    const int bcast = (batch2 == 1 && batch > 1) ? 1 : 0;
    // (2/N and 1/N in double on the host, one rounding each)
    const float scale = (float)(2.0 / (double)total), inv_n = (float)(1.0 / (double)total);
    hipStream_t s = (hipStream_t)stream;
    // the grid depends on the size only, so the partials (and the loss) are the same bits on every call
    int blocks;
    if ((per_sample & 3) == 0) {
        const int64_t total4 = total / 4;
        blocks = (int)std::min<int64_t>(ceil_div(total4, 4 * MSE_BLOCK), W2E_MSE_PARTIALS);
        mse_relu_vec_kernel<<<blocks, MSE_BLOCK, 0, s>>>(f1, f2, per_sample / 4, bcast, scale, gpre1, gpre2, partials, total4);
    } else {
        blocks = (int)std::min<int64_t>(ceil_div(total, 4 * MSE_BLOCK), W2E_MSE_PARTIALS);
        mse_relu_scalar_kernel<<<blocks, MSE_BLOCK, 0, s>>>(f1, f2, per_sample, bcast, scale, gpre1, gpre2, partials, total);
    }
    W2E_LAUNCH_CHECK("mse_relu_fwd");
    mse_final_kernel<<<1, MSE_BLOCK, 0, s>>>(partials, blocks, inv_n, loss);
    W2E_LAUNCH_CHECK("mse_relu_fwd (final sum)");
    return 0;
}
