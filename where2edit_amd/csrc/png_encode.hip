// PNG encoding on the device (include/w2e_png.h, "encoding"; DESIGN.md "K17e"): the row filter, the deflate kernel around
// csrc/png_deflate_core.h, and the gather that joins the chunks' slots into one zlib stream per image.
//
// Stage 1: one wave per row, four rows per workgroup.  Filtered byte (x, y) needs pixels (x, y), (x - 1, y), (x, y - 1) and
// (x - 1, y - 1) of the INPUT, so every row is independent: a first pass scores None, Sub, Up and Paeth (four wave reductions), a second
// writes the winner.  The row is read twice; the second read comes from the cache.
//
// Stage 2: one workgroup of ONE wave per chunk, the whole batch in one launch; then one workgroup per chunk again copies its slot to
// where the lengths of the slots before it put it.  No workgroup waits on another: the order comes from the launch boundary.
#include "../../include/w2e_image.h"
#include "../../include/w2e_png.h"
#include "common.h"
#include "png_core.h"
#include "png_deflate_core.h"

namespace w2e {
namespace {

constexpr int EW = 64;         // threads of the deflate kernel: one wave
constexpr int FILTER_ROWS = 4; // rows (waves) of a workgroup of the filter kernel
constexpr int GATHER = 256;    // threads of the gather kernel
static_assert(sizeof(pngenc::Shared) <= W2E_PNG_DEFLATE_LDS, "the header's bound of stage 2's LDS");
static_assert(W2E_PNG_SLOT % 4 == 0 && W2E_PNG_SLOT >= W2E_PNG_CHUNK + 10, "a slot holds the stored form, in whole words");

struct FilterArgs {
    const uint8_t* x;
    uint8_t* raw;
    int64_t raw_pitch;
    int h, w;
};

__device__ __forceinline__ uint32_t filter_cost(int v) { return (uint32_t)(v < 128 ? v : 256 - v); }

template <int C>
__global__ __launch_bounds__(64 * FILTER_ROWS) void png_filter_kernel(const FilterArgs a) {
    const int lane = threadIdx.x & 63, y = blockIdx.x * FILTER_ROWS + (threadIdx.x >> 6), b = blockIdx.y;
    if (y >= a.h) return;  // (no barrier below: a wave is on its own)
    const int rb = a.w * C;
    const uint8_t* cur = a.x + ((int64_t)b * a.h + y) * rb;
    const bool first = y == 0;
    const uint8_t* up = first ? cur : cur - rb;  // (never read on the first row, whose row above is all zero)
    uint32_t s_none = 0, s_sub = 0, s_up = 0, s_paeth = 0;
    for (int i = lane; i < rb; i += 64) {
        const int v = cur[i], l = i >= C ? cur[i - C] : 0, u = first ? 0 : up[i], ul = (first || i < C) ? 0 : up[i - C];
        s_none += filter_cost(v), s_sub += filter_cost((v - l) & 255), s_up += filter_cost((v - u) & 255);
        s_paeth += filter_cost((v - png::paeth(l, u, ul)) & 255);
    }
    for (int off = 32; off > 0; off >>= 1) {
        s_none += __shfl_xor(s_none, off, 64), s_sub += __shfl_xor(s_sub, off, 64);
        s_up += __shfl_xor(s_up, off, 64), s_paeth += __shfl_xor(s_paeth, off, 64);
    }
    // Pillow's order of trial: None, Up, Sub, Paeth; a later one needs a strictly smaller sum
    int filter = 0;
    uint32_t best = s_none;
    if (s_up < best) filter = 2, best = s_up;
    if (s_sub < best) filter = 1, best = s_sub;
    if (s_paeth < best) filter = 4, best = s_paeth;
    uint8_t* out = a.raw + b * a.raw_pitch + (int64_t)y * (rb + 1);
    if (lane == 0) out[0] = (uint8_t)filter;
    for (int i = lane; i < rb; i += 64) {
        const int v = cur[i], l = i >= C ? cur[i - C] : 0, u = first ? 0 : up[i], ul = (first || i < C) ? 0 : up[i - C];
        const int pred = filter == 0 ? 0 : filter == 1 ? l : filter == 2 ? u : png::paeth(l, u, ul);
        out[1 + i] = (uint8_t)(v - pred);
    }
}

struct DeflateArgs {
    const uint8_t* raw;
    const int64_t* sizes;
    uint8_t* out;
    int64_t* lengths;
    uint8_t* slots;    // [batch * chunks][W2E_PNG_SLOT]
    uint32_t* tokens;  // [batch * chunks][W2E_PNG_CHUNK]
    int32_t* meta;     // [batch * chunks][4]: the slot's bytes, the chunk's Adler sums s1 and s2, its length
    int64_t raw_pitch, out_pitch, max_size;
    int chunks;
};

__device__ __forceinline__ int64_t clamped_size(const DeflateArgs& a, int b) {
    const int64_t size = a.sizes[b];
    return size < 0 ? 0 : size > a.max_size ? a.max_size : size;
}

__global__ __launch_bounds__(EW) void png_deflate_kernel(const DeflateArgs a) {
    __shared__ pngenc::Shared sh;
    const int c = blockIdx.x, b = blockIdx.y;
    const int64_t size = clamped_size(a, b);
    const int chunks = pngenc::chunks_of(size);
    if (c >= chunks) return;  // (the gather never looks at this image's slots from `chunks` on)
    const int64_t g = (int64_t)b * a.chunks + c, at = (int64_t)c * pngenc::CHUNK;
    const int n = (int)(size - at < pngenc::CHUNK ? size - at : pngenc::CHUNK);
    pngenc::Deflate d(sh, pngenc::Lanes{(int)threadIdx.x, EW}, a.raw + b * a.raw_pitch + at, n, c == chunks - 1, a.tokens + g * pngenc::CHUNK,
                      reinterpret_cast<uint32_t*>(a.slots + g * W2E_PNG_SLOT));
    const int bytes = d.run();
    if (threadIdx.x == 0) {
        int32_t* m = a.meta + 4 * g;
        m[0] = bytes, m[1] = (int32_t)d.s1, m[2] = (int32_t)d.s2, m[3] = n;
    }
}

__global__ __launch_bounds__(GATHER) void png_gather_kernel(const DeflateArgs a) {
    __shared__ int64_t part[GATHER];
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int chunks = pngenc::chunks_of(clamped_size(a, b));
    if (c >= chunks) return;
    const int32_t* meta = a.meta + 4 * (int64_t)b * a.chunks;
    int64_t before = 0;  // the bytes of the slots before this one
    for (int j = tid; j < c; j += GATHER) before += meta[4 * j];
    part[tid] = before;
    __syncthreads();
    for (int off = GATHER / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] += part[tid + off];
        __syncthreads();
    }
    before = part[0];
    const int len = meta[4 * c];
    uint8_t* stream = a.out + b * a.out_pitch;
    uint8_t* dst = stream + 2 + before;
    const uint8_t* src = a.slots + ((int64_t)b * a.chunks + c) * W2E_PNG_SLOT;
    // bytes up to the destination's next word, whole words, the bytes that are left
    int lead = (int)((4 - ((uintptr_t)dst & 3)) & 3);
    if (lead > len) lead = len;
    const int words = (len - lead) / 4;
    if (tid < lead) dst[tid] = src[tid];
    for (int w = tid; w < words; w += GATHER) {
        const uint8_t* s = src + lead + 4 * w;
        *reinterpret_cast<uint32_t*>(dst + lead + 4 * w) = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
    }
    const int done = lead + 4 * words;
    if (tid < len - done) dst[done + tid] = src[done + tid];
    if (tid != 0) return;
    if (c == 0) stream[0] = pngenc::ZLIB_CMF, stream[1] = pngenc::ZLIB_FLG;
    if (c == chunks - 1) {
        uint32_t s1 = 1, s2 = 0;
        for (int j = 0; j < chunks; ++j) pngenc::adler_combine(s1, s2, (uint32_t)meta[4 * j + 1], (uint32_t)meta[4 * j + 2], (uint32_t)meta[4 * j + 3]);
        uint8_t* tail = dst + len;
        tail[0] = (uint8_t)(s2 >> 8), tail[1] = (uint8_t)s2, tail[2] = (uint8_t)(s1 >> 8), tail[3] = (uint8_t)s1;
        a.lengths[b] = 2 + before + len + 4;
    }
}

const char* check_encode(const char* who, int batch, int h, int w, int channels) {
    if (batch < 0 || batch > 65535) return refusal("%s: batch %d is not in 0..65535", who, batch);
    if (h < 1 || h > W2E_IMAGE_MAX_SIZE || w < 1 || w > W2E_IMAGE_MAX_SIZE) return refusal("%s: sizes are 1..%d (got %d x %d)", who, W2E_IMAGE_MAX_SIZE, h, w);
    if (channels < 1 || channels > 4) return refusal("%s: channels are 1 (L), 2 (LA), 3 (RGB) or 4 (RGBA) (got %d)", who, channels);
    return nullptr;
}

const char* check_deflate(const char* who, int batch, int64_t max_size) {
    if (batch < 0 || batch > 65535) return refusal("%s: batch %d is not in 0..65535", who, batch);
    if (max_size < 0 || max_size > 0x7fffffffLL) return refusal("%s: max_size %lld is not in 0..2^31-1", who, (long long)max_size);
    return nullptr;
}

void deflate_plan(int batch, int64_t max_size, int64_t* plan) {
    plan[0] = pngenc::chunks_of(max_size);
    plan[1] = W2E_PNG_SLOT;
    plan[2] = (int64_t)batch * plan[0] * (W2E_PNG_SLOT + 4 * (int64_t)W2E_PNG_CHUNK + 16);
    plan[3] = max_size + 10 * plan[0] + 6;
}

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_png_deflate_plan(int batch, int64_t max_size, int64_t* plan) {
    W2E_REQUIRE(plan, "png_deflate_plan: null plan");
    const char* why = check_deflate("png_deflate_plan", batch, max_size);
    W2E_REQUIRE(!why, "%s", why);
    deflate_plan(batch, max_size, plan);
    return 0;
}

extern "C" int w2e_png_encode_plan(int batch, int h, int w, int channels, int64_t* plan) {
    W2E_REQUIRE(plan, "png_encode_plan: null plan");
    const char* why = check_encode("png_encode_plan", batch, h, w, channels);
    W2E_REQUIRE(!why, "%s", why);
    plan[0] = 1 + (int64_t)w * channels;
    plan[1] = h * plan[0];
    plan[2] = (plan[1] + 3) / 4 * 4;
    deflate_plan(batch, plan[1], plan + 3);
    plan[7] = (plan[6] + 3) / 4 * 4;
    return 0;
}

extern "C" int w2e_png_filter(const uint8_t* x, int batch, int h, int w, int channels, uint8_t* raw, int64_t raw_pitch, void* stream) {
    W2E_REQUIRE(x && raw, "png_filter: null tensor");
    const char* why = check_encode("png_filter", batch, h, w, channels);
    W2E_REQUIRE(!why, "%s", why);
    const int64_t size = (int64_t)h * (1 + (int64_t)w * channels);
    W2E_REQUIRE(raw_pitch >= size, "png_filter: raw_pitch %lld is below the image's %lld bytes (w2e_png_encode_plan: plan[1])", (long long)raw_pitch,
                (long long)size);
    if (batch == 0) return 0;
    FilterArgs a;
    a.x = x, a.raw = raw, a.raw_pitch = raw_pitch, a.h = h, a.w = w;
    const dim3 grid((h + FILTER_ROWS - 1) / FILTER_ROWS, batch);
    hipStream_t s = (hipStream_t)stream;
    switch (channels) {
        case 1: png_filter_kernel<1><<<grid, 64 * FILTER_ROWS, 0, s>>>(a); break;
        case 2: png_filter_kernel<2><<<grid, 64 * FILTER_ROWS, 0, s>>>(a); break;
        case 3: png_filter_kernel<3><<<grid, 64 * FILTER_ROWS, 0, s>>>(a); break;
        default: png_filter_kernel<4><<<grid, 64 * FILTER_ROWS, 0, s>>>(a); break;
    }
    W2E_LAUNCH_CHECK("png_filter");
    return 0;
}

extern "C" int w2e_png_deflate(const uint8_t* raw, int64_t raw_pitch, const int64_t* sizes, int batch, int64_t max_size, uint8_t* out,
                               int64_t out_pitch, int64_t* lengths, uint8_t* work, int64_t work_bytes, void* stream) {
    W2E_REQUIRE(raw && sizes && out && lengths && work, "png_deflate: null tensor");
    const char* why = check_deflate("png_deflate", batch, max_size);
    W2E_REQUIRE(!why, "%s", why);
    int64_t plan[4];
    deflate_plan(batch, max_size, plan);
    W2E_REQUIRE(raw_pitch % 4 == 0 && raw_pitch >= max_size && raw_pitch > 0, "png_deflate: raw_pitch is a positive multiple of 4, at least max_size %lld (got %lld)",
                (long long)max_size, (long long)raw_pitch);
    W2E_REQUIRE(out_pitch % 4 == 0 && out_pitch >= plan[3], "png_deflate: out_pitch is a multiple of 4, at least the largest stream's %lld bytes (got %lld)",
                (long long)plan[3], (long long)out_pitch);
    W2E_REQUIRE(work_bytes >= plan[2], "png_deflate: the workspace has %lld bytes, w2e_png_deflate_plan asks for %lld", (long long)work_bytes, (long long)plan[2]);
    W2E_REQUIRE((uintptr_t)raw % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)sizes % 8 == 0 && (uintptr_t)lengths % 8 == 0 && (uintptr_t)work % 8 == 0,
                "png_deflate: raw and out must be 4-byte aligned, sizes, lengths and work 8-byte aligned");
    if (batch == 0) return 0;
    const int64_t slots = (int64_t)batch * plan[0];
    DeflateArgs a;
    a.raw = raw, a.sizes = sizes, a.out = out, a.lengths = lengths, a.raw_pitch = raw_pitch, a.out_pitch = out_pitch, a.max_size = max_size;
    a.chunks = (int)plan[0];
    a.slots = work;                                                                 // (W2E_PNG_SLOT is a multiple of 4: every part is aligned)
    a.tokens = reinterpret_cast<uint32_t*>(work + slots * W2E_PNG_SLOT);
    a.meta = reinterpret_cast<int32_t*>(work + slots * (W2E_PNG_SLOT + 4 * (int64_t)W2E_PNG_CHUNK));
    const dim3 grid((unsigned)plan[0], (unsigned)batch);
    png_deflate_kernel<<<grid, EW, 0, (hipStream_t)stream>>>(a);
    W2E_LAUNCH_CHECK("png_deflate");
    png_gather_kernel<<<grid, GATHER, 0, (hipStream_t)stream>>>(a);
    W2E_LAUNCH_CHECK("png_deflate (gather)");
    return 0;
}
