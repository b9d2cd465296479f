// Image I/O (include/w2e_image.h): Pillow's 8-bit resize + ToTensor / Normalize on the way in, torchvision's make_grid / save_image
// quantisation on the way out.  The arithmetic is the specification (DESIGN.md "Image I/O"): integer coefficient tables made on the
// host, int32 accumulation, a byte between the two passes; separately rounded fp32 operations in the quantiser.
//
// Resize, fused form.  A 256-thread workgroup owns TH x TW output pixels of one image.
//   1. stage: the input rows x columns under the tile go to LDS as 16-byte chunks at their ABSOLUTE 16-byte alignment (a row keeps
//      its address modulo 16 in LDS, so every chunk is one aligned global load and one ds_write_b128); a chunk that is not wholly
//      inside the source buffer is read byte by byte, each byte bounds-checked.  The tile's slices of the coefficient tables and the
//      normalisation table go to LDS in the same phase.
//   2. horizontal pass, LDS -> LDS bytes: a wave takes a staged row, its lanes the row's TW * C intermediate bytes.
//   3. vertical pass from the byte tile, then the table look-up (fp32 NCHW: a wave takes a (row, channel) pair, lanes run along x, so
//      a store instruction covers one contiguous run of floats) or the byte store (uint8 NHWC: a lane makes 4 consecutive bytes and
//      stores them as one word where the address allows).
// An axis that is not passed is the one-tap identity (K = 2^22 at the pixel's own index: (2^21 + v * 2^22) >> 22 == v), so that
// there is one kernel, not four.  The span a tile needs grows with in / out; when it does not fit in 64 KB the plan takes the
// two-launch form: one thread per output byte, taps read from global memory, the intermediate image in a caller's workspace.
#include "../../include/w2e_image.h"
#include "device.h"

#include <math.h>

namespace w2e {
namespace {

constexpr int IMG_THREADS = 256;
constexpr int IMG_WAVES = IMG_THREADS / 64;
constexpr int ONE = 1 << W2E_IMAGE_PRECISION_BITS;
constexpr int HALF = 1 << (W2E_IMAGE_PRECISION_BITS - 1);
constexpr int64_t IMG_LDS_LIMIT = 64 * 1024;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int to_byte(int acc) { return clampi(acc >> W2E_IMAGE_PRECISION_BITS, 0, 255); }

// ---- the plan (host) ----

struct AxisPlan {
    int passed, ksize;
    double scale, support;
};

AxisPlan axis_plan(int in, int out) {
    AxisPlan a;
    a.passed = in != out;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 1.0 * fs;
    a.ksize = a.passed ? (int)ceil(a.support) * 2 + 1 : 0;
    return a;
}

// Input samples under `t` consecutive outputs of an axis, at most: the first window starts at centre_0 - support, the last ends at
// centre_{t-1} + support, both rounded to integers (+2); NEAREST's single tap lies inside the BILINEAR window.
int span_cap(const AxisPlan& a, int t, int in) {
    if (!a.passed) return t;
    const double s = (t - 1) * a.scale + 2.0 * a.support;
    const int64_t cap = (int64_t)ceil(s) + 2;
    return (int)(cap < in ? cap : in);
}

struct FusedGeom {
    int th, tw, cap_rows, cap_cols, pitch_in, pitch_mid, ksx, ksy;
    int off_kx, off_bx, off_ky, off_by, off_in, off_mid;  // byte offsets into the dynamic LDS (the lut comes first)
    int64_t lds;
};

int round_up(int64_t v, int m) { return (int)((v + m - 1) / m * m); }

// LDS of the fused form for a th x tw tile (tw a power of two), or more than IMG_LDS_LIMIT.  ksx / ksy: the row length of the tables
// (>= 1; 1 for an axis that is not passed).
FusedGeom fused_geom(int channels, int in_h, int in_w, int out_h, int out_w, int th, int tw, int ksx, int ksy) {
    FusedGeom g;
    const AxisPlan ax = axis_plan(in_w, out_w), ay = axis_plan(in_h, out_h);
    g.th = th, g.tw = tw, g.ksx = ksx, g.ksy = ksy;
    const int tw_eff = tw < out_w ? tw : out_w, th_eff = th < out_h ? th : out_h;
    g.cap_cols = span_cap(ax, tw_eff, in_w);
    g.cap_rows = span_cap(ay, th_eff, in_h);
    g.pitch_in = round_up((int64_t)g.cap_cols * channels + 15, 16);  // + the row's address modulo 16
    g.pitch_mid = round_up((int64_t)tw * channels, 4);
    int64_t o = (int64_t)channels * 256 * 4;
    g.off_kx = (int)o, o += (int64_t)tw * ksx * 4;
    g.off_bx = (int)o, o += (int64_t)tw * 8;
    g.off_ky = (int)o, o += (int64_t)th * ksy * 4;
    g.off_by = (int)o, o += (int64_t)th * 8;
    o = (o + 15) / 16 * 16;
    g.off_in = (int)(o < (1 << 30) ? o : (1 << 30)), o += (int64_t)g.cap_rows * g.pitch_in;
    o = (o + 15) / 16 * 16;
    g.off_mid = (int)(o < (1 << 30) ? o : (1 << 30)), o += (int64_t)g.cap_rows * g.pitch_mid;
    g.lds = o;
    return g;
}

// The tiles tried, in this order; the first that fits is taken.  (Larger tiles re-read less halo: a tile of TH rows stages
// TH * scale + 2 * support of them.)
constexpr int TILES[3][2] = {{8, 64}, {8, 32}, {4, 32}};

// Fills `g` and returns true when a fused tile fits; ksx / ksy <= 0: the BILINEAR sizes.
bool pick_fused(int channels, int in_h, int in_w, int out_h, int out_w, int ksx, int ksy, FusedGeom* g) {
    const AxisPlan ax = axis_plan(in_w, out_w), ay = axis_plan(in_h, out_h);
    // the LDS is sized with the BILINEAR tables whatever is handed in: the form then depends on the sizes alone, as the plan says
    const int px = ax.passed ? ax.ksize : 1, py = ay.passed ? ay.ksize : 1;
    for (const auto& t : TILES) {
        const FusedGeom big = fused_geom(channels, in_h, in_w, out_h, out_w, t[0], t[1], px, py);
        if (big.lds > IMG_LDS_LIMIT) continue;
        *g = fused_geom(channels, in_h, in_w, out_h, out_w, t[0], t[1], ksx > 0 ? ksx : px, ksy > 0 ? ksy : py);
        return g->lds <= IMG_LDS_LIMIT;
    }
    return false;
}

const char* check_dims(const char* who, int batch, int channels, int in_h, int in_w, int out_h, int out_w) {
    if (batch < 0) return refusal("%s: batch %d < 0", who, batch);
    if (channels != 1 && channels != 3) return refusal("%s: channels must be 1 or 3 (got %d)", who, channels);
    const int v[4] = {in_h, in_w, out_h, out_w};
    for (int s : v)
        if (s < 1 || s > W2E_IMAGE_MAX_SIZE) return refusal("%s: every size must be in 1..%d (got %d x %d -> %d x %d)", who, W2E_IMAGE_MAX_SIZE, in_h, in_w, out_h, out_w);
    return nullptr;
}

// ---- the fused kernel ----

struct ResizeArgs {
    const uint8_t* src;
    const int32_t *kx, *bx, *ky, *by;  // NULL: the axis is not passed
    const float* lut;
    void* dst;
    int64_t src_bytes;
    int in_h, in_w, out_h, out_w, tiles_x, tiles_y;
    FusedGeom g;
};

template <int C, bool F32>
__global__ __launch_bounds__(IMG_THREADS) void image_resize_fused_kernel(const ResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    float* s_lut = reinterpret_cast<float*>(smem);
    int32_t* s_kx = reinterpret_cast<int32_t*>(smem + a.g.off_kx);
    int32_t* s_bx = reinterpret_cast<int32_t*>(smem + a.g.off_bx);
    int32_t* s_ky = reinterpret_cast<int32_t*>(smem + a.g.off_ky);
    int32_t* s_by = reinterpret_cast<int32_t*>(smem + a.g.off_by);
    uint8_t* s_in = smem + a.g.off_in;
    uint8_t* s_mid = smem + a.g.off_mid;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int ty = tl / a.tiles_x, tx = tl - ty * a.tiles_x;
    const int TH = a.g.th, TW = a.g.tw, ksx = a.g.ksx, ksy = a.g.ksy;
    const int tx0 = tx * TW, ty0 = ty * TH;
    const int tw = min(TW, a.out_w - tx0), th = min(TH, a.out_h - ty0);

    // the tile's input span, from the tables' first and last window; clamped to the image and to what the LDS was sized for
    int x0 = a.kx ? a.bx[2 * tx0] : tx0;
    int x1 = a.kx ? a.bx[2 * (tx0 + tw - 1)] + a.bx[2 * (tx0 + tw - 1) + 1] : tx0 + tw;
    int y0 = a.ky ? a.by[2 * ty0] : ty0;
    int y1 = a.ky ? a.by[2 * (ty0 + th - 1)] + a.by[2 * (ty0 + th - 1) + 1] : ty0 + th;
    x0 = clampi(x0, 0, a.in_w - 1), x1 = clampi(x1, x0 + 1, min(a.in_w, x0 + a.g.cap_cols));
    y0 = clampi(y0, 0, a.in_h - 1), y1 = clampi(y1, y0 + 1, min(a.in_h, y0 + a.g.cap_rows));
    const int rows = y1 - y0, span_bytes = (x1 - x0) * C;

    // 1. tables
    for (int i = tid; i < tw * ksx; i += IMG_THREADS) s_kx[i] = a.kx ? a.kx[(int64_t)tx0 * ksx + i] : ONE;
    for (int i = tid; i < tw; i += IMG_THREADS) {
        s_bx[2 * i] = a.kx ? a.bx[2 * (tx0 + i)] : tx0 + i;
        s_bx[2 * i + 1] = a.kx ? a.bx[2 * (tx0 + i) + 1] : 1;
    }
    for (int i = tid; i < th * ksy; i += IMG_THREADS) s_ky[i] = a.ky ? a.ky[(int64_t)ty0 * ksy + i] : ONE;
    for (int i = tid; i < th; i += IMG_THREADS) {
        s_by[2 * i] = a.ky ? a.by[2 * (ty0 + i)] : ty0 + i;
        s_by[2 * i + 1] = a.ky ? a.by[2 * (ty0 + i) + 1] : 1;
    }
    if constexpr (F32)
        for (int i = tid; i < C * 256; i += IMG_THREADS) s_lut[i] = a.lut[i];

    // 1. the input span: row r of the tile starts at src + row_off(r); its chunk i is the 16 bytes at (that address & ~15) + 16 i
    const uintptr_t lo = reinterpret_cast<uintptr_t>(a.src), hi = lo + (uintptr_t)a.src_bytes;
    const int chunks_cap = a.g.pitch_in / 16;
    for (int r = wave; r < rows; r += IMG_WAVES) {
        const uintptr_t start = lo + (uintptr_t)((((int64_t)b * a.in_h + y0 + r) * a.in_w + x0) * C);
        const uintptr_t base = start & ~(uintptr_t)15;
        const int chunks = min((int)((start - base + span_bytes + 15) / 16), chunks_cap);
        for (int i = lane; i < chunks; i += 64) {
            const uintptr_t g = base + 16 * (uintptr_t)i;
            uint4 v;
            if (g >= lo && g + 16 <= hi) {
                v = *reinterpret_cast<const uint4*>(g);
            } else {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uintptr_t p = g + j;
                    if (p >= lo && p < hi) w[j >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t*>(p)) << (8 * (j & 3));
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *reinterpret_cast<uint4*>(s_in + (int64_t)r * a.g.pitch_in + 16 * i) = v;
        }
    }
    __syncthreads();

    // 2. horizontal pass: s_in -> s_mid
    const int mid_w = tw * C;
    for (int r = wave; r < rows; r += IMG_WAVES) {
        const uintptr_t start = lo + (uintptr_t)((((int64_t)b * a.in_h + y0 + r) * a.in_w + x0) * C);
        const uint8_t* row = s_in + (int64_t)r * a.g.pitch_in + (int)(start & 15);
        for (int e = lane; e < mid_w; e += 64) {
            const int x = e / C, c = e - x * C;
            const int first = s_bx[2 * x], n = clampi(s_bx[2 * x + 1], 0, ksx);
            const int32_t* k = s_kx + x * ksx;
            int acc = HALF;
            for (int t = 0; t < n; ++t) acc += (int)row[(clampi(first + t, x0, x1 - 1) - x0) * C + c] * k[t];
            s_mid[r * a.g.pitch_mid + e] = (uint8_t)to_byte(acc);
        }
    }
    __syncthreads();

    // 3. vertical pass: s_mid -> dst
    if constexpr (F32) {
        float* dst = static_cast<float*>(a.dst);
        for (int q = wave; q < th * C; q += IMG_WAVES) {
            const int y = q / C, c = q - y * C;
            const int first = s_by[2 * y], n = clampi(s_by[2 * y + 1], 0, ksy);
            const int32_t* k = s_ky + y * ksy;
            float* out = dst + (((int64_t)b * C + c) * a.out_h + ty0 + y) * a.out_w + tx0;
            for (int x = lane; x < tw; x += 64) {
                int acc = HALF;
                for (int t = 0; t < n; ++t) acc += (int)s_mid[(clampi(first + t, y0, y1 - 1) - y0) * a.g.pitch_mid + x * C + c] * k[t];
                out[x] = s_lut[c * 256 + to_byte(acc)];
            }
        }
    } else {
        uint8_t* dst = static_cast<uint8_t*>(a.dst);
        const int words = (mid_w + 3) / 4;
        for (int y = wave; y < th; y += IMG_WAVES) {
            const int first = s_by[2 * y], n = clampi(s_by[2 * y + 1], 0, ksy);
            const int32_t* k = s_ky + y * ksy;
            uint8_t* out = dst + (((int64_t)b * a.out_h + ty0 + y) * a.out_w + tx0) * C;
            for (int u = lane; u < words; u += 64) {
                int acc[4] = {HALF, HALF, HALF, HALF};
                const int e0 = 4 * u;
                for (int t = 0; t < n; ++t) {
                    const uint8_t* m = s_mid + (clampi(first + t, y0, y1 - 1) - y0) * a.g.pitch_mid + e0;  // (pitch_mid % 4 == 0: in bounds)
                    const int kt = k[t];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += (int)m[j] * kt;
                }
                uint8_t* p = out + e0;
                if (e0 + 4 <= mid_w && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
                    *reinterpret_cast<uint32_t*>(p) = (uint32_t)to_byte(acc[0]) | (uint32_t)to_byte(acc[1]) << 8 | (uint32_t)to_byte(acc[2]) << 16 |
                                                      (uint32_t)to_byte(acc[3]) << 24;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (e0 + j < mid_w) p[j] = (uint8_t)to_byte(acc[j]);
                }
            }
        }
    }
}

// ---- the two-launch form: one axis per launch, one thread per output sample ----
// src [B, in_h, in_w, C] bytes -> [B, out_h, out_w, C] bytes (lut == NULL) or fp32 [B, C, out_h, out_w]; exactly one of the two axes
// changes size, or none (k == NULL: a copy through the table).
template <int C>
__global__ __launch_bounds__(IMG_THREADS) void image_resample_axis_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ k,
                                                                          const int32_t* __restrict__ bounds, int ksize, int vertical, int in_h,
                                                                          int in_w, int out_h, int out_w, const float* __restrict__ lut,
                                                                          void* __restrict__ dst, int64_t total) {
    const int64_t step = (int64_t)gridDim.x * IMG_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x; i < total; i += step) {
        const int c = (int)(i % C);
        int64_t q = i / C;
        const int x = (int)(q % out_w);
        q /= out_w;
        const int y = (int)(q % out_h);
        const int64_t b = q / out_h;
        const int o = vertical ? y : x, in = vertical ? in_h : in_w;
        const int first = k ? bounds[2 * o] : o, n = k ? clampi(bounds[2 * o + 1], 0, ksize) : 1;
        const int64_t stride = vertical ? (int64_t)in_w * C : C;
        const uint8_t* p = src + ((b * in_h + (vertical ? 0 : y)) * in_w + (vertical ? x : 0)) * C + c;
        int acc = HALF;
        for (int t = 0; t < n; ++t) acc += (int)p[clampi(first + t, 0, in - 1) * stride] * (k ? k[(int64_t)o * ksize + t] : ONE);
        const int v = to_byte(acc);
        if (lut) static_cast<float*>(dst)[((b * C + c) * out_h + y) * out_w + x] = lut[c * 256 + v];
        else static_cast<uint8_t*>(dst)[i] = (uint8_t)v;
    }
}

// ---- quantise ----

__device__ __forceinline__ uint32_t quantise_unit(float t) {  // trunc(clamp(t * 255 + 0.5, 0, 255)), NaN -> 0; no contraction
    const float q = __fadd_rn(__fmul_rn(t, 255.0f), 0.5f);
    if (!(q == q)) return 0u;
    return (uint32_t)(int)fminf(fmaxf(q, 0.0f), 255.0f);
}

struct QuantArgs {
    const float* src;
    uint8_t* dst;
    int64_t total;     // bytes of dst
    int64_t row_bytes;  // of dst
    int batch, channels, h, w, out_c, grid, xmaps, padding;
    float lo, neg_lo, hi, divisor;
    uint32_t pad_byte;
};

__device__ __forceinline__ uint32_t quantise_at(const QuantArgs& a, int64_t row, int col) {
    const int px = col / a.out_c, oc = col - px * a.out_c;
    int64_t k;
    int y, x;
    if (a.grid) {  // canvas cell (gy, gx) holds image gy * xmaps + gx at (padding, padding) of the cell
        const int cell_h = a.h + a.padding, cell_w = a.w + a.padding;
        const int gy = (int)(row / cell_h), gx = px / cell_w;
        y = (int)(row - (int64_t)gy * cell_h) - a.padding, x = px - gx * cell_w - a.padding;
        k = (int64_t)gy * a.xmaps + gx;
        if (y < 0 || x < 0 || gx >= a.xmaps || k >= a.batch) return a.pad_byte;
    } else {
        k = row / a.h, y = (int)(row - k * a.h), x = px;
    }
    const int c = a.channels == 1 ? 0 : oc;
    const float v = a.src[((k * a.channels + c) * a.h + y) * a.w + x];
    if (!(v == v)) return 0u;
    const float t = __fdiv_rn(__fadd_rn(fminf(fmaxf(v, a.lo), a.hi), a.neg_lo), a.divisor);
    return quantise_unit(t);
}

__global__ __launch_bounds__(IMG_THREADS) void image_quantize_kernel(const QuantArgs a) {
    const int64_t words = (a.total + 3) / 4, step = (int64_t)gridDim.x * IMG_THREADS;
    for (int64_t u = (int64_t)blockIdx.x * IMG_THREADS + threadIdx.x; u < words; u += step) {
        const int64_t i0 = 4 * u;
        int64_t row = i0 / a.row_bytes;
        int col = (int)(i0 - row * a.row_bytes);
        uint32_t word = 0;
        const int nb = a.total - i0 < 4 ? (int)(a.total - i0) : 4;
        for (int j = 0; j < nb; ++j) {
            word |= quantise_at(a, row, col) << (8 * j);
            if (++col == a.row_bytes) col = 0, ++row;
        }
        if (nb == 4) {
            *reinterpret_cast<uint32_t*>(a.dst + i0) = word;
        } else {
            for (int j = 0; j < nb; ++j) a.dst[i0 + j] = (uint8_t)(word >> (8 * j));
        }
    }
}

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_image_resize_plan(int batch, int channels, int in_h, int in_w, int out_h, int out_w, int64_t* plan) {
    W2E_REQUIRE(plan, "image_resize_plan: null plan");
    const char* why = check_dims("image_resize_plan", batch, channels, in_h, in_w, out_h, out_w);
    W2E_REQUIRE(!why, "%s", why);
    const AxisPlan ax = axis_plan(in_w, out_w), ay = axis_plan(in_h, out_h);
    for (int i = 0; i < 8; ++i) plan[i] = 0;
    plan[2] = ax.ksize, plan[3] = ay.ksize;
    FusedGeom g;
    if (pick_fused(channels, in_h, in_w, out_h, out_w, 0, 0, &g)) {
        plan[4] = g.th, plan[5] = g.tw, plan[6] = g.lds;
    } else {
        plan[0] = 1;
        plan[1] = ax.passed && ay.passed ? (int64_t)batch * in_h * out_w * channels : 0;
    }
    return 0;
}

extern "C" int w2e_image_resize(const uint8_t* src, int batch, int channels, int in_h, int in_w, int out_h, int out_w, const int32_t* kx,
                                const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, const float* lut,
                                void* dst, void* workspace, void* stream) {
    W2E_REQUIRE(src && dst, "image_resize: null tensor");
    const char* why = check_dims("image_resize", batch, channels, in_h, in_w, out_h, out_w);
    W2E_REQUIRE(!why, "%s", why);
    const AxisPlan ax = axis_plan(in_w, out_w), ay = axis_plan(in_h, out_h);
    if (!ax.passed) kx = nullptr, bx = nullptr, ksize_x = 1;
    if (!ay.passed) ky = nullptr, by = nullptr, ksize_y = 1;
    W2E_REQUIRE(!ax.passed || (kx && bx), "image_resize: null tables for the horizontal axis (%d -> %d)", in_w, out_w);
    W2E_REQUIRE(!ay.passed || (ky && by), "image_resize: null tables for the vertical axis (%d -> %d)", in_h, out_h);
    W2E_REQUIRE(!ax.passed || (ksize_x >= 1 && ksize_x <= ax.ksize), "image_resize: ksize_x %d is not in 1..%d", ksize_x, ax.ksize);
    W2E_REQUIRE(!ay.passed || (ksize_y >= 1 && ksize_y <= ay.ksize), "image_resize: ksize_y %d is not in 1..%d", ksize_y, ay.ksize);
    W2E_REQUIRE(!lut || (uintptr_t)lut % 4 == 0, "image_resize: lut must be 4-byte aligned");
    W2E_REQUIRE(!lut || (uintptr_t)dst % 4 == 0, "image_resize: an fp32 dst must be 4-byte aligned");
    W2E_REQUIRE(((uintptr_t)kx | (uintptr_t)bx | (uintptr_t)ky | (uintptr_t)by) % 4 == 0, "image_resize: the tables must be 4-byte aligned");
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    ResizeArgs a;
    if (pick_fused(channels, in_h, in_w, out_h, out_w, ksize_x, ksize_y, &a.g)) {
        a.src = src, a.kx = kx, a.bx = bx, a.ky = ky, a.by = by, a.lut = lut, a.dst = dst;
        a.src_bytes = (int64_t)batch * in_h * in_w * channels;
        a.in_h = in_h, a.in_w = in_w, a.out_h = out_h, a.out_w = out_w;
        a.tiles_x = (int)ceil_div(out_w, a.g.tw), a.tiles_y = (int)ceil_div(out_h, a.g.th);
        const int64_t grid = (int64_t)batch * a.tiles_x * a.tiles_y;
        W2E_REQUIRE(grid <= 0x7fffffff, "image_resize: %lld tiles in one call: split the batch", (long long)grid);
#define IMG_GO(C_, F_) image_resize_fused_kernel<C_, F_><<<(unsigned)grid, IMG_THREADS, (size_t)a.g.lds, s>>>(a)
        if (channels == 1) {
            if (lut) IMG_GO(1, true);
            else IMG_GO(1, false);
        } else {
            if (lut) IMG_GO(3, true);
            else IMG_GO(3, false);
        }
#undef IMG_GO
        W2E_LAUNCH_CHECK("image_resize (fused)");
        return 0;
    }
    const bool both = ax.passed && ay.passed;
    W2E_REQUIRE(!both || workspace, "image_resize: the two-launch form needs a workspace of %lld bytes (w2e_image_resize_plan)",
                (long long)batch * in_h * out_w * channels);
#define IMG_AXIS(src_, k_, b_, ks_, vert_, ih_, iw_, oh_, ow_, lut_, dst_)                                                              \
    do {                                                                                                                                \
        const int64_t total_ = (int64_t)batch * (oh_) * (ow_) * channels;                                                               \
        const int grid_ = stream_grid(total_, IMG_THREADS);                                                                             \
        if (channels == 1)                                                                                                              \
            image_resample_axis_kernel<1><<<grid_, IMG_THREADS, 0, s>>>(src_, k_, b_, ks_, vert_, ih_, iw_, oh_, ow_, lut_, dst_, total_); \
        else                                                                                                                            \
            image_resample_axis_kernel<3><<<grid_, IMG_THREADS, 0, s>>>(src_, k_, b_, ks_, vert_, ih_, iw_, oh_, ow_, lut_, dst_, total_); \
        W2E_LAUNCH_CHECK("image_resize (axis pass)");                                                                                   \
    } while (0)
    if (both) {
        IMG_AXIS(src, kx, bx, ksize_x, 0, in_h, in_w, in_h, out_w, (const float*)nullptr, workspace);
        IMG_AXIS((const uint8_t*)workspace, ky, by, ksize_y, 1, in_h, out_w, out_h, out_w, lut, dst);
    } else if (ay.passed) {
        IMG_AXIS(src, ky, by, ksize_y, 1, in_h, in_w, out_h, out_w, lut, dst);
    } else {
        IMG_AXIS(src, kx, bx, ksize_x, 0, in_h, in_w, out_h, out_w, lut, dst);
    }
#undef IMG_AXIS
    return 0;
}

extern "C" int w2e_image_quantize(const float* src, int batch, int channels, int h, int w, float lo, float hi, float divisor, int nrow,
                                  int padding, float pad_value, int grid, uint8_t* dst, void* stream) {
    W2E_REQUIRE(src && dst, "image_quantize: null tensor");
    const char* why = check_dims("image_quantize", batch, channels, h, w, h, w);
    W2E_REQUIRE(!why, "%s", why);
    W2E_REQUIRE(lo == lo && hi == hi && divisor == divisor, "image_quantize: the range or the divisor is NaN");
    W2E_REQUIRE(lo < hi && divisor > 0.0f, "image_quantize: need lo < hi and divisor > 0 (got %g, %g, %g)", lo, hi, divisor);
    W2E_REQUIRE((uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0, "image_quantize: src and dst must be 4-byte aligned");
    if (grid) {
        W2E_REQUIRE(nrow >= 1, "image_quantize: nrow %d < 1", nrow);
        W2E_REQUIRE(padding >= 0 && padding <= 1024, "image_quantize: padding %d is not in 0..1024", padding);
    }
    if (batch == 0) return 0;
    QuantArgs a;
    a.src = src, a.dst = dst, a.batch = batch, a.channels = channels, a.h = h, a.w = w;
    a.lo = lo, a.neg_lo = -lo, a.hi = hi, a.divisor = divisor;
    a.grid = grid != 0, a.xmaps = 1, a.padding = 0, a.pad_byte = 0;
    int64_t rows;
    if (!a.grid) {
        a.out_c = channels, rows = (int64_t)batch * h, a.row_bytes = (int64_t)w * channels;
    } else if (batch == 1) {  // make_grid returns a single image as it is (after the replication)
        a.out_c = 3, rows = h, a.row_bytes = (int64_t)w * 3;
    } else {
        a.out_c = 3, a.padding = padding;
        a.xmaps = nrow < batch ? nrow : batch;
        const int64_t ymaps = ceil_div(batch, a.xmaps);
        rows = ymaps * (h + padding) + padding, a.row_bytes = ((int64_t)a.xmaps * (w + padding) + padding) * 3;
        volatile float m = pad_value * 255.0f;  // (volatile: the product is rounded to fp32 before the add, as on the device)
        const float r = m + 0.5f;
        a.pad_byte = r == r ? (uint32_t)(int)fminf(fmaxf(r, 0.0f), 255.0f) : 0u;
    }
    W2E_REQUIRE(a.row_bytes <= 0x7fffffff, "image_quantize: a canvas row of %lld bytes", (long long)a.row_bytes);
    a.total = rows * a.row_bytes;
    image_quantize_kernel<<<stream_grid(ceil_div(a.total, 4), IMG_THREADS), IMG_THREADS, 0, (hipStream_t)stream>>>(a);
    W2E_LAUNCH_CHECK("image_quantize");
    return 0;
}
