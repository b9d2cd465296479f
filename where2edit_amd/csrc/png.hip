// PNG decoding on the device (include/w2e_png.h; DESIGN.md "K17d"): the inflate kernel around csrc/png_core.h, and the kernel that
// undoes the row filters and writes the pixels.
//
// Stage 1: one workgroup of ONE wave per zlib stream, the whole batch in one launch.  Inflate is a serial chain, so all 64 lanes
// follow the same symbols (the reader's state is the same in every lane) and share only the work that is wide: filling the input
// window, building the tables of a block, copying a match, flushing the ring to memory in whole words.  No workgroup waits on another.
//
// Stage 2: one wave per image.  Byte (x, y) of a filtered row depends on (x - bpp, y), (x, y - 1) and (x - bpp, y - 1), so a wave takes
// a band of W2E_PNG_BAND rows, lane r on row y0 + r ONE pixel behind lane r - 1: what lane r - 1 produced at the step before is the
// pixel above, the value above at the step before that is the pixel above left.  Lane 0 reads the row above its band from memory,
// where the last lane of the band before has left it (in `raw`, in place), so the bands of an image run in sequence.  Pixels are
// loaded and stored in chunks of PX steps so that a chunk costs one memory latency, not PX.
#include "../../include/w2e_image.h"
#include "../../include/w2e_png.h"
#include "common.h"
#include "png_core.h"

namespace w2e {
namespace {

constexpr int PW = 64;  // threads of both kernels: one wave
constexpr int PX = 8;   // steps of stage 2 between two rounds of loads and stores
static_assert(PW == W2E_PNG_BAND, "a lane of stage 2 per row of a band");
static_assert(sizeof(png::Shared) <= W2E_PNG_INFLATE_LDS, "the header's bound of stage 1's LDS");
static_assert(png::FLUSH % 4 == 0 && png::FLUSH + 258 + 4 < png::RING, "the ring is flushed in words, long before it wraps onto itself");

struct InflateArgs {
    const uint8_t* streams;
    const int64_t* meta;
    const int64_t* sizes;
    int64_t stream_bytes, raw_pitch;
    uint8_t* raw;
    int32_t* status;
};

__global__ __launch_bounds__(PW) void png_inflate_kernel(const InflateArgs a) {
    __shared__ png::Shared sh;
    const int b = blockIdx.x;
    int64_t size = a.sizes[b];
    int st = 0;
    if (size < 0 || size > a.raw_pitch) size = size < 0 ? 0 : a.raw_pitch, st = W2E_PNG_STATUS_LONG;
    png::Inflate inf(sh, png::Lanes{(int)threadIdx.x, PW}, a.streams, a.stream_bytes, a.meta[2 * b], a.meta[2 * b + 1], a.raw + b * a.raw_pitch, size);
    st |= inf.run();
    if (threadIdx.x == 0) a.status[b] = st;
}

struct PixelArgs {
    uint8_t* raw;
    const uint32_t* palette;
    uint8_t* out;
    int32_t* status;
    int64_t raw_pitch;
    int h, w, row_bytes, units;  // bytes of a filtered row with its filter byte; filter units (pixels, or packed bytes below 8 bits) of a row
    int colour, depth, mode;
};

// The pixels of one filter unit, converted and stored.  v: the reconstructed bytes of the unit, the first in the low byte.
template <int BPP>
__device__ __forceinline__ void store_unit(const PixelArgs& a, const uint32_t* pal, uint8_t* out, int y, int x, uint32_t v) {
    if (a.depth < 8) {  // a palette below 8 bits: 8 / depth indices in the byte, the first in the high bits
        const int per = 8 / a.depth;
        for (int k = 0; k < per; ++k) {
            const int px = x * per + k;
            if (px >= a.w) break;
            const uint32_t idx = (v >> (8 - a.depth * (k + 1))) & ((1u << a.depth) - 1u);
            if (a.mode == W2E_PNG_MODE_RAW) {
                out[(int64_t)y * a.w + px] = (uint8_t)idx;
            } else {
                const uint32_t c = pal[idx];
                uint8_t* o = out + ((int64_t)y * a.w + px) * 3;
                o[0] = (uint8_t)c, o[1] = (uint8_t)(c >> 8), o[2] = (uint8_t)(c >> 16);
            }
        }
        return;
    }
    const int64_t at = (int64_t)y * a.w + x;
    if (a.mode == W2E_PNG_MODE_RAW) {
#pragma unroll
        for (int c = 0; c < BPP; ++c) out[at * BPP + c] = (uint8_t)(v >> (8 * c));
        return;
    }
    uint32_t c = v;                                                        // colours 2 and 6: R, G, B are the first three bytes
    if (a.colour == 0 || a.colour == 4) c = (v & 255u) * 0x010101u;        // grey: replicated
    if (a.colour == 3) c = pal[v & 255u];
    uint8_t* o = out + at * 3;
    o[0] = (uint8_t)c, o[1] = (uint8_t)(c >> 8), o[2] = (uint8_t)(c >> 16);
}

template <int BPP>
__global__ __launch_bounds__(PW) void png_pixels_kernel(const PixelArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    uint8_t* rows = a.raw + b * a.raw_pitch;
    const int out_channels = a.mode == W2E_PNG_MODE_RGB ? 3 : (a.depth < 8 ? 1 : BPP);
    uint8_t* out = a.out + (int64_t)b * a.h * a.w * out_channels;
    const uint32_t* pal = a.palette + (int64_t)b * 256;
    int bad = 0;
    for (int y0 = 0; y0 < a.h; y0 += PW) {
        __syncthreads();  // the last row of the band before is in memory, reconstructed
        const int y = y0 + lane;
        const bool live = y < a.h;
        uint8_t* row = rows + (int64_t)(live ? y : 0) * a.row_bytes;
        int filter = live ? row[0] : 0;
        if (filter > 4) filter = 0, bad = 1;
        const bool keep = live && lane == PW - 1 && y + 1 < a.h;  // the next band reads this row from memory
        const bool above = lane == 0 && y0 > 0;
        uint32_t left = 0, upleft = 0, last = 0;
        for (int t0 = 0; t0 < a.units + PW - 1; t0 += PX) {
            const int x0 = t0 - lane;
            uint32_t px[PX], upm[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const int x = x0 + j;
                const bool ok = live && x >= 0 && x < a.units;
                uint32_t v = 0, u = 0;
                if (ok) {
                    const uint8_t* p = row + 1 + (int64_t)x * BPP;
#pragma unroll
                    for (int c = 0; c < BPP; ++c) v |= (uint32_t)p[c] << (8 * c);
                    if (above) {
#pragma unroll
                        for (int c = 0; c < BPP; ++c) u |= (uint32_t)(p - a.row_bytes)[c] << (8 * c);
                    }
                }
                px[j] = v, upm[j] = u;
            }
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                uint32_t up = (uint32_t)__shfl_up((int)last, 1, 64);
                if (lane == 0) up = upm[j];
                if (x0 + j == 0) left = 0, upleft = 0;
                uint32_t cur = 0;
#pragma unroll
                for (int c = 0; c < BPP; ++c)
                    cur |= (uint32_t)png::unfilter(filter, (px[j] >> (8 * c)) & 255, (left >> (8 * c)) & 255, (up >> (8 * c)) & 255, (upleft >> (8 * c)) & 255)
                           << (8 * c);
                px[j] = cur;
                left = cur, upleft = up, last = cur;
            }
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const int x = x0 + j;
                if (live && x >= 0 && x < a.units) {
                    store_unit<BPP>(a, pal, out, y, x, px[j]);
                    if (keep) {
                        uint8_t* p = row + 1 + (int64_t)x * BPP;
#pragma unroll
                        for (int c = 0; c < BPP; ++c) p[c] = (uint8_t)(px[j] >> (8 * c));
                    }
                }
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
    if (lane == 0 && bad) a.status[b] |= W2E_PNG_STATUS_FILTER;
}

// bits per pixel of a colour type at a depth, or 0 when the pair is out of scope
int pixel_bits(int colour, int depth) {
    if (colour == 3) return (depth == 1 || depth == 2 || depth == 4 || depth == 8) ? depth : 0;
    if (depth != 8) return 0;
    return colour == 0 ? 8 : colour == 2 ? 24 : colour == 4 ? 16 : colour == 6 ? 32 : 0;
}

const char* check_png(const char* who, int batch, int h, int w, int colour, int depth, int mode) {
    if (batch < 0 || batch > 65535) return refusal("%s: batch %d is not in 0..65535", who, batch);
    if (h < 1 || h > W2E_IMAGE_MAX_SIZE || w < 1 || w > W2E_IMAGE_MAX_SIZE) return refusal("%s: sizes are 1..%d (got %d x %d)", who, W2E_IMAGE_MAX_SIZE, h, w);
    if (!pixel_bits(colour, depth))
        return refusal("%s: colour type %d at depth %d is out of scope (0, 2, 4, 6 at 8 bits; 3 at 1, 2, 4, 8 bits)", who, colour, depth);
    if (mode != W2E_PNG_MODE_RGB && mode != W2E_PNG_MODE_RAW) return refusal("%s: mode %d is neither W2E_PNG_MODE_RGB nor W2E_PNG_MODE_RAW", who, mode);
    return nullptr;
}

int64_t row_bytes(int w, int colour, int depth) { return 1 + ((int64_t)w * pixel_bits(colour, depth) + 7) / 8; }

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_png_plan(int batch, int h, int w, int colour, int depth, int mode, int64_t* plan) {
    W2E_REQUIRE(plan, "png_plan: null plan");
    const char* why = check_png("png_plan", batch, h, w, colour, depth, mode);
    W2E_REQUIRE(!why, "%s", why);
    const int bits = pixel_bits(colour, depth);
    plan[0] = row_bytes(w, colour, depth);
    plan[1] = h * plan[0];
    plan[2] = (plan[1] + 3) / 4 * 4;
    plan[3] = mode == W2E_PNG_MODE_RGB ? 3 : (colour == 3 ? 1 : bits / 8);
    plan[4] = (int64_t)h * w * plan[3];
    plan[5] = bits < 8 ? 1 : bits / 8;
    plan[6] = W2E_PNG_INFLATE_LDS;
    plan[7] = W2E_PNG_BAND;
    return 0;
}

extern "C" int w2e_png_inflate(const uint8_t* streams, const int64_t* meta, const int64_t* sizes, int64_t stream_bytes, int batch, uint8_t* raw,
                               int64_t raw_pitch, int32_t* status, void* stream) {
    W2E_REQUIRE(streams && meta && sizes && raw && status, "png_inflate: null tensor");
    W2E_REQUIRE(batch >= 0 && batch <= 65535, "png_inflate: batch %d is not in 0..65535", batch);
    W2E_REQUIRE(stream_bytes >= 0 && stream_bytes % 4 == 0, "png_inflate: stream_bytes is a multiple of 4 (got %lld)", (long long)stream_bytes);
    W2E_REQUIRE(raw_pitch > 0 && raw_pitch % 4 == 0, "png_inflate: raw_pitch is a positive multiple of 4 (got %lld)", (long long)raw_pitch);
    W2E_REQUIRE((uintptr_t)streams % 4 == 0 && (uintptr_t)raw % 4 == 0 && (uintptr_t)status % 4 == 0 && (uintptr_t)meta % 8 == 0 && (uintptr_t)sizes % 8 == 0,
                "png_inflate: streams, raw and status must be 4-byte aligned, meta and sizes 8-byte aligned");
    if (batch == 0) return 0;
    InflateArgs a;
    a.streams = streams, a.meta = meta, a.sizes = sizes, a.stream_bytes = stream_bytes, a.raw_pitch = raw_pitch, a.raw = raw, a.status = status;
    png_inflate_kernel<<<batch, PW, 0, (hipStream_t)stream>>>(a);
    W2E_LAUNCH_CHECK("png_inflate");
    return 0;
}

extern "C" int w2e_png_pixels(uint8_t* raw, int64_t raw_pitch, const uint32_t* palette, int batch, int h, int w, int colour, int depth, int mode,
                              uint8_t* out, int32_t* status, void* stream) {
    W2E_REQUIRE(raw && out && status, "png_pixels: null tensor");
    const char* why = check_png("png_pixels", batch, h, w, colour, depth, mode);
    W2E_REQUIRE(!why, "%s", why);
    W2E_REQUIRE(palette || colour != 3 || mode != W2E_PNG_MODE_RGB, "png_pixels: null palette for colour type 3 in RGB mode");
    W2E_REQUIRE((uintptr_t)palette % 4 == 0 && (uintptr_t)status % 4 == 0, "png_pixels: palette and status must be 4-byte aligned");
    const int64_t rb = row_bytes(w, colour, depth);
    W2E_REQUIRE(raw_pitch >= h * rb, "png_pixels: raw_pitch %lld is below the image's %lld bytes (w2e_png_plan: plan[1])", (long long)raw_pitch,
                (long long)(h * rb));
    if (batch == 0) return 0;
    PixelArgs a;
    a.raw = raw, a.palette = palette, a.out = out, a.status = status, a.raw_pitch = raw_pitch;
    a.h = h, a.w = w, a.row_bytes = (int)rb, a.colour = colour, a.depth = depth, a.mode = mode;
    const int bpp = pixel_bits(colour, depth) < 8 ? 1 : pixel_bits(colour, depth) / 8;
    a.units = (int)(rb - 1) / bpp;
    hipStream_t s = (hipStream_t)stream;
    switch (bpp) {
        case 1: png_pixels_kernel<1><<<batch, PW, 0, s>>>(a); break;
        case 2: png_pixels_kernel<2><<<batch, PW, 0, s>>>(a); break;
        case 3: png_pixels_kernel<3><<<batch, PW, 0, s>>>(a); break;
        default: png_pixels_kernel<4><<<batch, PW, 0, s>>>(a); break;
    }
    W2E_LAUNCH_CHECK("png_pixels");
    return 0;
}
