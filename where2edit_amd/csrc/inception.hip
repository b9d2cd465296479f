// Inception-v3 feature extractor (include/w2e_inception.h): the implicit-GEMM convolution with folded BatchNorm + ReLU that covers
// all nine geometric forms of the network's 94 convolutions and its fully connected head, the three 3x3 pools, and the input resize.
#include "../../include/w2e_inception.h"
#include "device.h"

namespace w2e {
namespace {

constexpr unsigned OOB = 0xfffffff0u;  // past every descriptor below (each tensor is held under 2 GiB): such a load returns 0

struct ConvP {
    const float *x, *w, *scale, *shift;
    float* y;
    int B, Cin, H, W, N, KH, KW, stride, ph, pw, OH, OW, relu, ych, yoff;
    int K, M;    // GEMM K = Cin*KH*KW, M = B*OH*OW
    int table;   // the (k -> input offset, tap) table is in dynamic LDS (K int2 entries)
};

// Output tile: TO = 32*WO output channels (accumulator rows) x TP = 32*WP positions of the flattened [B, OH, OW] (accumulator columns,
// so a lane's stores run along a row of y).  Four waves, one 32x32 accumulator block each; K in chunks of 32 through LDS, the next
// chunk's global loads in flight during a chunk's MFMAs.  out[o][p] = sum_k Ws[o][k] * Xs[k][p] through device.h's mm_rows_cols: the
// weight tile row-major (b128 in from global memory when K % 4 == 0, b128 to LDS, b128 out), the gathered input tile read down its
// rows with lanes along p.  Every output is summed by one wave in one accumulator, over k in mm_rows_cols' fixed order.
template <int WO, int WP>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const ConvP p) {
    static_assert(WO * WP == 4, "four waves");
    constexpr int TO = 32 * WO, TP = 32 * WP, KC = 32, SW = KC + 4;  // (rows of 36 floats: 16-byte aligned, b128 reads conflict free)
    constexpr int XK = 256 / TP, XE = KC / XK;  // X tile: XK rows of k per pass, XE passes
    constexpr int WV = TO / 32;                 // W tile: a float4 of k per thread and pass, 8 threads per row, 32 rows per pass
    __shared__ __attribute__((aligned(16))) float Ws[TO * SW];
    __shared__ float Xs[KC * TP];
    extern __shared__ int2 ktab[];
    const int t = threadIdx.x, lane = t & 63, j = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wo = (wave % WO) * 32, wp = (wave / WO) * 32;
    const int o0 = blockIdx.y * TO, p0 = blockIdx.x * TP;
    const int HW = p.H * p.W, KHW = p.KH * p.KW, OHW = p.OH * p.OW;
    // k -> (offset of its tap inside a sample of x, index of the tap)
    const auto kdecode = [&](int k) -> int2 {
        const int c = k / KHW, tap = k - c * KHW, kh = tap / p.KW;
        return make_int2(c * HW + kh * p.W + (tap - kh * p.KW), tap);
    };
    if (p.table) {
        for (int k = t; k < p.K; k += 256) ktab[k] = kdecode(k);
        __syncthreads();
    }
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x), (short)0, (int)((unsigned)p.B * p.Cin * HW * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), (short)0, (int)((unsigned)p.N * p.K * 4u), 0x00020000);
    // this thread's column of the X tile: one output position, fixed over the whole K loop; bit `tap` of tapmask: that tap of its
    // window lies inside the image (at most 49 taps; bit 63 stays clear and stands for "k past K")
    const int xp = t % TP, xk = t / TP;
    const int pos = p0 + xp;
    const bool pvalid = pos < p.M;
    const int pb = pvalid ? pos / OHW : 0, psp = pvalid ? pos - pb * OHW : 0;
    const int poh = psp / p.OW, pow_ = psp - poh * p.OW;
    const int ih0 = poh * p.stride - p.ph, iw0 = pow_ * p.stride - p.pw;
    const int xbase = pb * p.Cin * HW + ih0 * p.W + iw0;  // may be negative; only used with an in-bounds tap added
    unsigned long long tapmask = 0;
    if (pvalid)
        for (int kh = 0; kh < p.KH; ++kh)
            for (int kw = 0; kw < p.KW; ++kw)
                if ((unsigned)(ih0 + kh) < (unsigned)p.H && (unsigned)(iw0 + kw) < (unsigned)p.W) tapmask |= 1ull << (kh * p.KW + kw);
    const int wq = (t & 7) * 4, wrow = t >> 3;
    const bool wvec = (p.K & 3) == 0;  // rows of wt start 16-byte aligned relative to each other and no float4 straddles K
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    float xr[XE];
    f32x4 wr[WV];
    const auto gload = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < XE; ++i) {
            const int k = k0 + xk + XK * i;
            int2 e = make_int2(0, 63);
            if (k < p.K) e = p.table ? ktab[k] : (KHW == 1 ? make_int2(k * HW, 0) : kdecode(k));
            const unsigned off = ((tapmask >> e.y) & 1ull) ? (unsigned)(xbase + e.x) * 4u : OOB;
            xr[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, off, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < WV; ++i) {
            const int o = o0 + wrow + 32 * i, k = k0 + wq;
            const unsigned row = (unsigned)o * p.K * 4u;
            if (wvec) {
                wr[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (o < p.N && k < p.K) ? row + k * 4u : OOB, 0, 0));
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    wr[i][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, (o < p.N && k + c < p.K) ? row + (k + c) * 4u : OOB, 0, 0));
            }
        }
    };
    f32x16 acc;
    acc_zero(acc);
    gload(0);
    for (int k0 = 0; k0 < p.K; k0 += KC) {
#pragma unroll
        for (int i = 0; i < XE; ++i) Xs[(xk + XK * i) * TP + xp] = xr[i];
#pragma unroll
        for (int i = 0; i < WV; ++i) *reinterpret_cast<f32x4*>(Ws + (wrow + 32 * i) * SW + wq) = wr[i];
        __syncthreads();
        if (k0 + KC < p.K) gload(k0 + KC);
        mm_rows_cols<SW, TP, KC / 8>(acc, Ws, Xs, wo, wp, j, half);
        __syncthreads();
    }
    // epilogue: register r of lane (half, j) is output channel o0 + wo + acc_row(r, half), position p0 + wp + j
    const int opos = p0 + wp + j;
    if (opos >= p.M) return;
    const int ob = opos / OHW, osp = opos - ob * OHW;
    float* yb = p.y + ((int64_t)ob * p.ych + p.yoff) * OHW + osp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = o0 + wo + acc_row(r, half);
        if (o < p.N) {
            const float a = p.scale ? p.scale[o] : 1.f, b = p.shift ? p.shift[o] : 0.f;
            float v = a * acc[r] + b;
            if (p.relu) v = v > 0.f ? v : (v != v ? v : 0.f);  // relu keeps a NaN, as torch's does
            yb[(int64_t)o * OHW] = v;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void pool3x3_kernel(const float* __restrict__ x, float* __restrict__ y, int C, int H, int W, int OH,
                                                      int OW, int ych, int yoff, int64_t total) {
    constexpr int S = MODE == W2E_POOL_MAX_S2 ? 2 : 1, P = MODE == W2E_POOL_MAX_S2 ? 0 : 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ow = (int)(i % OW);
        const int64_t q = i / OW;
        const int oh = (int)(q % OH);
        const int64_t plane = q / OH;  // b * C + c
        const int c = (int)(plane % C);
        const int64_t b = plane / C;
        const float* xp = x + plane * H * W;
        float m = -INFINITY, sum = 0.f;
        int count = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = oh * S - P + dy;
            if (iy < 0 || iy >= H) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = ow * S - P + dx;
                if (ix < 0 || ix >= W) continue;
                const float v = xp[(int64_t)iy * W + ix];
                if (MODE == W2E_POOL_AVG_S1P1) {
                    sum += v;
                    ++count;
                } else if (v > m || v != v) {  // PyTorch: a later NaN replaces, a tie keeps the first
                    m = v;
                }
            }
        }
        y[((b * ych + yoff + c) * OH + oh) * (int64_t)OW + ow] = MODE == W2E_POOL_AVG_S1P1 ? sum / (float)count : m;
    }
}

__global__ __launch_bounds__(256) void inception_resize_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, int in_h,
                                                               int in_w, int64_t total) {
    constexpr int S = W2E_INCEPTION_SIZE;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % S);
        const int64_t q = i / S;
        const int oy = (int)(q % S);
        const int64_t bc = q / S;
        const int c = (int)(bc % 3);
        const int64_t b = bc / 3;
        const int ny = oy * in_h, nx = ox * in_w;  // < 299 * 16384
        const int y0 = ny / S, x0 = nx / S;
        const float ty = (float)(ny - y0 * S) / (float)S, tx = (float)(nx - x0 * S) / (float)S;
        const int y1 = y0 + 1 < in_h ? y0 + 1 : in_h - 1, x1 = x0 + 1 < in_w ? x0 + 1 : in_w - 1;
        const uint8_t* im = src + b * in_h * in_w * 3 + c;
        const float tl = im[((int64_t)y0 * in_w + x0) * 3], tr = im[((int64_t)y0 * in_w + x1) * 3];
        const float bl = im[((int64_t)y1 * in_w + x0) * 3], br = im[((int64_t)y1 * in_w + x1) * 3];
        const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
        const float v = top + (bot - top) * ty;
        dst[i] = (v - 128.f) / 128.f;
    }
}

bool kernel_size_ok(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_conv2d_bn_relu(const float* x, const float* wt, const float* scale, const float* shift, float* y, int batch, int cin,
                                  int h, int w, int n, int kh, int kw, int stride, int ph, int pw, int relu, int y_channels, int y_ch_off,
                                  void* stream) {
    W2E_REQUIRE(x && wt && y, "conv2d_bn_relu: null tensor");
    W2E_REQUIRE(batch >= 0 && cin >= 1 && h >= 1 && w >= 1 && n >= 1, "conv2d_bn_relu: bad shape (batch %d, cin %d, %dx%d, n %d)", batch,
                cin, h, w, n);
    W2E_REQUIRE(kernel_size_ok(kh) && kernel_size_ok(kw), "conv2d_bn_relu: kernel %dx%d: each side is 1, 3, 5 or 7", kh, kw);
    W2E_REQUIRE(stride == 1 || stride == 2, "conv2d_bn_relu: stride %d is neither 1 nor 2", stride);
    W2E_REQUIRE(ph >= 0 && ph < kh && pw >= 0 && pw < kw, "conv2d_bn_relu: padding (%d, %d) for a %dx%d kernel", ph, pw, kh, kw);
    W2E_REQUIRE(h + 2 * ph >= kh && w + 2 * pw >= kw, "conv2d_bn_relu: a %dx%d image (padding %d, %d) holds no %dx%d window", h, w, ph, pw,
                kh, kw);
    W2E_REQUIRE(y_ch_off >= 0 && y_ch_off + (int64_t)n <= y_channels, "conv2d_bn_relu: channels [%d, %d) do not lie in an output of %d",
                y_ch_off, y_ch_off + n, y_channels);
    const int oh = (h + 2 * ph - kh) / stride + 1, ow = (w + 2 * pw - kw) / stride + 1;
    const int64_t K = (int64_t)cin * kh * kw, M = (int64_t)batch * oh * ow;
    const int64_t lim = (int64_t)1 << 29;  // floats in 2 GiB
    W2E_REQUIRE((int64_t)batch * cin * h * w < lim && (int64_t)n * K < lim && (int64_t)batch * y_channels * oh * ow < lim,
                "conv2d_bn_relu: a tensor of 2 GiB or more (x, wt and y are addressed with 32-bit offsets)");
    if (batch == 0) return 0;
    ConvP p{x, wt, scale, shift, y, batch, cin, h, w, n, kh, kw, stride, ph, pw, oh, ow, relu, y_channels, y_ch_off, (int)K, (int)M, 0};
    p.table = kh * kw > 1 && K <= 4608;  // 36 KB of dynamic LDS beside 20 KB of tiles; beyond, the taps are divided out per load
    const size_t lds = p.table ? (size_t)K * sizeof(int2) : 0;
    hipStream_t s = (hipStream_t)stream;
    // Four waves share a tile of 8192 outputs: 32 channels x 128 positions wherever that pads N less than 64 x 64 does (N = 32, 96,
    // 192 -> 0 instead of 32 idle rows).  (Measured and not kept: one wave per workgroup with K chunks of 64 for the layers that fill
    // fewer than eight waves per CU -- 17^2 and 8^2 at a small batch; without the operand sharing of a four-wave tile every one of
    // them ran slower, 11.3 ms against 8.8 ms over the network's 94 convolutions at batch 8.)
    if ((n + 31) / 32 * 32 < (n + 63) / 64 * 64) {
        dim3 grid((unsigned)ceil_div(M, 128), (unsigned)ceil_div(n, 32));
        conv_igemm_kernel<1, 4><<<grid, 256, lds, s>>>(p);
    } else {
        dim3 grid((unsigned)ceil_div(M, 64), (unsigned)ceil_div(n, 64));
        conv_igemm_kernel<2, 2><<<grid, 256, lds, s>>>(p);
    }
    W2E_LAUNCH_CHECK("conv2d_bn_relu");
    return 0;
}

extern "C" int w2e_pool3x3(const float* x, float* y, int batch, int channels, int h, int w, int mode, int y_channels, int y_ch_off,
                           void* stream) {
    W2E_REQUIRE(x && y, "pool3x3: null tensor");
    W2E_REQUIRE(mode == W2E_POOL_MAX_S2 || mode == W2E_POOL_AVG_S1P1 || mode == W2E_POOL_MAX_S1P1, "pool3x3: unknown mode %d", mode);
    W2E_REQUIRE(batch >= 0 && channels >= 1 && h >= 1 && w >= 1, "pool3x3: bad shape (batch %d, channels %d, %dx%d)", batch, channels, h, w);
    W2E_REQUIRE(mode != W2E_POOL_MAX_S2 || (h >= 3 && w >= 3), "pool3x3: a %dx%d image holds no unpadded 3x3 window", h, w);
    W2E_REQUIRE(y_ch_off >= 0 && y_ch_off + (int64_t)channels <= y_channels, "pool3x3: channels [%d, %d) do not lie in an output of %d",
                y_ch_off, y_ch_off + channels, y_channels);
    const int oh = mode == W2E_POOL_MAX_S2 ? (h - 3) / 2 + 1 : h, ow = mode == W2E_POOL_MAX_S2 ? (w - 3) / 2 + 1 : w;
    const int64_t total = (int64_t)batch * channels * oh * ow;
    if (total == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int grid = stream_grid(total, 256);
    if (mode == W2E_POOL_MAX_S2)
        pool3x3_kernel<W2E_POOL_MAX_S2><<<grid, 256, 0, s>>>(x, y, channels, h, w, oh, ow, y_channels, y_ch_off, total);
    else if (mode == W2E_POOL_AVG_S1P1)
        pool3x3_kernel<W2E_POOL_AVG_S1P1><<<grid, 256, 0, s>>>(x, y, channels, h, w, oh, ow, y_channels, y_ch_off, total);
    else
        pool3x3_kernel<W2E_POOL_MAX_S1P1><<<grid, 256, 0, s>>>(x, y, channels, h, w, oh, ow, y_channels, y_ch_off, total);
    W2E_LAUNCH_CHECK("pool3x3");
    return 0;
}

extern "C" int w2e_inception_resize(const uint8_t* src, float* dst, int batch, int in_h, int in_w, void* stream) {
    W2E_REQUIRE(src && dst, "inception_resize: null tensor");
    W2E_REQUIRE(batch >= 0 && in_h >= 1 && in_w >= 1 && in_h <= 16384 && in_w <= 16384, "inception_resize: bad shape (batch %d, %dx%d)",
                batch, in_h, in_w);
    const int64_t total = (int64_t)batch * 3 * W2E_INCEPTION_SIZE * W2E_INCEPTION_SIZE;
    if (total == 0) return 0;
    inception_resize_kernel<<<stream_grid(total, 256), 256, 0, (hipStream_t)stream>>>(src, dst, in_h, in_w, total);
    W2E_LAUNCH_CHECK("inception_resize");
    return 0;
}
