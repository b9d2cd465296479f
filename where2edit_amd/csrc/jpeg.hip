// Baseline JPEG on the device (include/w2e_jpeg.h): the bytes of Pillow's default JPEG for the same pixels.  The arithmetic is the
// specification (DESIGN.md "K17b"): 16.16 fixed-point colour conversion, libjpeg's accurate integer DCT (jfdctint), integer
// quantisation, the Annex K Huffman tables.  Nothing here rounds in floating point.
//
// Stage 1, pixels -> coefficients, one launch.  A 256-thread workgroup owns a strip of up to 8 MCUs of one MCU row (128 x 16 pixels):
//   1. stage: the strip's RGB bytes go to LDS as 16-byte chunks at their ABSOLUTE 16-byte alignment (as csrc/image.hip stages its
//      rows; a chunk that is not wholly inside the source buffer is read byte by byte, each byte bounds-checked);
//   2. convert: a thread takes 2 x 2 pixel cells: four Y samples, one Cb and one Cr sample (the down-sampling is in the cell), edges
//      repeated by clamping the coordinates the way libjpeg extends its planes;
//   3. row pass of the DCT: a thread takes one row of one block, planes -> int32 [block][8][9] (the pad keeps the column pass off
//      one bank);
//   4. column pass + quantisation: a thread takes one column of one block and writes int16 at the zigzag positions of an LDS image
//      of the strip's output; 5. the dummies take their DC; 6. the strip's 6 * 64 * mcus coefficients leave as one contiguous run.
// LDS map (bytes): raw 16 x 400 = 6400 | Y 16 x 128 = 2048 | Cb, Cr 2 x 8 x 64 = 1024 | mid 48 x 72 x 4 = 13824 | out 48 x 64 x 2 =
// 6144: 29440.
//
// Stage 2, coefficients -> segment, three launches, no atomics on global memory, the same bytes on every run.
//   a. code: ONE WAVE PER BLOCK, a lane per coefficient.  The walk over 64 coefficients is not a walk: the run of zeros before a
//      coefficient is a count of leading zeros on the wave's non-zero ballot, so every lane knows its own (run, size) code, its
//      0xF0 prefixes and its value bits (at most 3 * 11 + 16 + 10 = 59 bits) at once; lane 0 codes the DC difference, lane 63 the
//      end-of-block when the block ends in zeros.  A wave scan of the lengths gives each lane its bit offset; the fields are OR-ed
//      into the wave's 52-word LDS slot (they do not overlap, so the order of the ORs is no concern) and the words in use go to the
//      block's slot in the workspace, with the length.
//   b. scan: one workgroup per image walks its lengths in tiles of 1024 blocks, carry in 64 bits.
//   c. gather: every 32-bit word of the output finds the block that covers its first bit (binary search on the offsets) and
//      assembles itself from that block and the ones after it; the last word is filled with 1-bits.
#include "../../include/w2e_image.h"
#include "../../include/w2e_jpeg.h"
#include "device.h"

namespace w2e {
namespace {

constexpr int JT = 256;                        // threads of every workgroup here
constexpr int SM = W2E_JPEG_STRIP_MCUS;        // MCUs per strip
constexpr int RAW_PITCH = SM * 16 * 3 + 16;    // a staged row: 384 bytes + its address modulo 16
constexpr int MID_PITCH = 9;
constexpr int SLOT = W2E_JPEG_SLOT_WORDS;
constexpr int SLOT_BITS = SLOT * 32;
constexpr int TILE = W2E_JPEG_SCAN_TILE;
static_assert(TILE == JT * 4, "the scan takes four lengths per thread");

// Annex K base tables, natural order
const uint8_t LUMA_Q[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// ZZ_POS[natural index] = position in the zigzag scan
__constant__ uint8_t ZZ_POS[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                   10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

struct Geom {
    int mx, my;
    int64_t blocks;
};

Geom geom(int h, int w) {
    Geom g;
    g.mx = (w + 15) / 16, g.my = (h + 15) / 16;
    g.blocks = (int64_t)6 * g.mx * g.my;
    return g;
}

const char* check_dims(const char* who, int batch, int h, int w) {
    if (batch < 0) return refusal("%s: batch %d < 0", who, batch);
    if (h < 1 || h > W2E_IMAGE_MAX_SIZE || w < 1 || w > W2E_IMAGE_MAX_SIZE)
        return refusal("%s: every size must be in 1..%d (got %d x %d)", who, W2E_IMAGE_MAX_SIZE, h, w);
    return nullptr;
}

// ---- stage 1 ----

struct CoefArgs {
    const uint8_t* src;
    int16_t* coef;
    int64_t src_bytes, blocks;
    int h, w, mx, my, strips;
    uint8_t q[2][64];  // natural order
};

constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270, FIX_0_899976223 = 7373,
              FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137, FIX_1_961570560 = 16069, FIX_2_053119869 = 16819,
              FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of jfdctint over d[0..7] in place.  FIRST: the row pass (outputs 0 and 4 scaled up by 2 bits, the others descaled by 11);
// otherwise the column pass (2 and 15).
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(int (&d)[8]) {
    constexpr int N = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if constexpr (FIRST) {
        d[0] = (t10 + t11) << 2, d[4] = (t10 - t11) << 2;
    } else {
        d[0] = descale(t10 + t11, 2), d[4] = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * FIX_0_541196100;
    d[2] = descale(z1 + t13 * FIX_0_765366865, N);
    d[6] = descale(z1 - t12 * FIX_1_847759065, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    const int u4 = t4 * FIX_0_298631336, u5 = t5 * FIX_2_053119869, u6 = t6 * FIX_3_072711026, u7 = t7 * FIX_1_501321110;
    z1 *= -FIX_0_899976223, z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5, z4 = z4 * -FIX_0_390180644 + z5;
    d[7] = descale(u4 + z1 + z3, N), d[5] = descale(u5 + z2 + z4, N);
    d[3] = descale(u6 + z2 + z3, N), d[1] = descale(u7 + z1 + z4, N);
}

constexpr int FIX_Y_R = 19595, FIX_Y_G = 38470, FIX_Y_B = 7471;        // FIX(.299) FIX(.587) FIX(.114), FIX(x) = int(x * 65536 + .5)
constexpr int FIX_CB_R = 11059, FIX_CB_G = 21709, FIX_HALF = 32768;    // FIX(.16874) FIX(.33126) FIX(.5)
constexpr int FIX_CR_G = 27439, FIX_CR_B = 5329;                       // FIX(.41869) FIX(.08131)
constexpr int C_OFFSET = (128 << 16) + 32767;

__global__ __launch_bounds__(JT) void jpeg_coefficients_kernel(const CoefArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[16 * RAW_PITCH];
    __shared__ uint8_t s_y[16][SM * 16];
    __shared__ uint8_t s_c[2][8][SM * 8];
    __shared__ int s_mid[SM * 6 * 8 * MID_PITCH];
    __shared__ __attribute__((aligned(16))) int16_t s_out[SM * 6 * 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per_image = a.my * a.strips;
    const int b = blockIdx.x / per_image, rs = blockIdx.x - b * per_image;
    const int r = rs / a.strips, m0 = (rs - r * a.strips) * SM;
    const int nm = min(SM, a.mx - m0);           // MCUs of this strip
    const int y0 = 16 * r, x0 = 16 * m0;
    const int nr = min(16, a.h - y0);            // real pixel rows (>= 1)
    const int nc = min(16 * nm, a.w - x0);       // real pixel columns (>= 1)

    // 1. the strip's bytes
    const uintptr_t lo = reinterpret_cast<uintptr_t>(a.src), hi = lo + (uintptr_t)a.src_bytes;
    for (int rr = wave; rr < nr; rr += JT / 64) {
        const uintptr_t start = lo + (uintptr_t)((((int64_t)b * a.h + y0 + rr) * a.w + x0) * 3);
        const uintptr_t base = start & ~(uintptr_t)15;
        const int chunks = min((int)((start - base + (uintptr_t)nc * 3 + 15) / 16), RAW_PITCH / 16);
        for (int i = lane; i < chunks; i += 64) {
            const uintptr_t g = base + 16 * (uintptr_t)i;
            uint4 v;
            if (g >= lo && g + 16 <= hi) {
                v = *reinterpret_cast<const uint4*>(g);
            } else {
                uint32_t wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uintptr_t p = g + j;
                    if (p >= lo && p < hi) wd[j >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t*>(p)) << (8 * (j & 3));
                }
                v = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
            *reinterpret_cast<uint4*>(s_raw + rr * RAW_PITCH + 16 * i) = v;
        }
    }
    __syncthreads();

    // 2. colour conversion and down-sampling, a 2 x 2 cell per step.  Y repeats the last row / column (coordinates clamped).  Chroma
    // repeats the last COLUMN before the down-sampling, but of the rows only one, when h is odd; the rows below repeat the last
    // DOWN-SAMPLED row, so a cell below the image takes the chroma rows of the last cell inside it.
    const int cells_x = 8 * nm, last_cy = (nr + 1) / 2 - 1;
    for (int i = tid; i < 8 * cells_x; i += JT) {
        const int cy = i / cells_x, cx = i - cy * cells_x;
        const int pc[2] = {min(2 * cx, nc - 1), min(2 * cx + 1, nc - 1)};
        const int yr[2] = {min(2 * cy, nr - 1), min(2 * cy + 1, nr - 1)};
        const int ccy = min(cy, last_cy);
        const int cr[2] = {2 * ccy, min(2 * ccy + 1, nr - 1)};
        int cb_sum = 0, cr_sum = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const uintptr_t ys = lo + (uintptr_t)((((int64_t)b * a.h + y0 + yr[dy]) * a.w + x0) * 3);
            const uintptr_t cs = lo + (uintptr_t)((((int64_t)b * a.h + y0 + cr[dy]) * a.w + x0) * 3);
            const uint8_t* yrow = s_raw + yr[dy] * RAW_PITCH + (int)(ys & 15);
            const uint8_t* crow = s_raw + cr[dy] * RAW_PITCH + (int)(cs & 15);
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const uint8_t* p = yrow + 3 * pc[dx];
                s_y[2 * cy + dy][2 * cx + dx] = (uint8_t)((FIX_Y_R * p[0] + FIX_Y_G * p[1] + FIX_Y_B * p[2] + 32768) >> 16);
                const uint8_t* q = crow + 3 * pc[dx];
                const int R = q[0], G = q[1], B = q[2];
                cb_sum += (-FIX_CB_R * R - FIX_CB_G * G + FIX_HALF * B + C_OFFSET) >> 16;
                cr_sum += (FIX_HALF * R - FIX_CR_G * G - FIX_CR_B * B + C_OFFSET) >> 16;
            }
        }
        const int bias = 1 + (cx & 1);  // (8 * m0 is even: the strip's column parity is the image's)
        s_c[0][cy][cx] = (uint8_t)((cb_sum + bias) >> 2);
        s_c[1][cy][cx] = (uint8_t)((cr_sum + bias) >> 2);
    }
    __syncthreads();

    // 3. rows
    const int items = nm * 6 * 8;
    for (int i = tid; i < items; i += JT) {
        const int blk = i >> 3, row = i & 7, mcu = blk / 6, j = blk - mcu * 6;
        const uint8_t* p = j < 4 ? &s_y[(j >> 1) * 8 + row][mcu * 16 + (j & 1) * 8] : &s_c[j - 4][row][mcu * 8];
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)p[k] - 128;
        fdct_pass<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) s_mid[i * MID_PITCH + k] = d[k];
    }
    __syncthreads();

    // 4. columns, quantisation; a dummy is written as zeros
    const int rows_y = (a.h + 7) / 8, cols_y = (a.w + 7) / 8;
    for (int i = tid; i < items; i += JT) {
        const int blk = i >> 3, col = i & 7, mcu = blk / 6, j = blk - mcu * 6;
        const bool dummy = j < 4 && (2 * r + (j >> 1) >= rows_y || 2 * (m0 + mcu) + (j & 1) >= cols_y);
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = s_mid[(blk * 8 + k) * MID_PITCH + col];
        fdct_pass<false>(d);
        const uint8_t* q = a.q[j < 4 ? 0 : 1];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int n = 8 * k + col, div = 8 * (int)q[n];
            const int mag = (int)((unsigned)((d[k] < 0 ? -d[k] : d[k]) + (div >> 1)) / (unsigned)div);
            s_out[blk * 64 + ZZ_POS[n]] = dummy ? (int16_t)0 : (int16_t)(d[k] < 0 ? -mag : mag);
        }
    }
    __syncthreads();

    // 5. a dummy's DC is that of the previous Y block in scan order: always inside the MCU, since Y(0,0) is never a dummy
    if (tid < nm) {
        for (int j = 1; j < 4; ++j)
            if (2 * r + (j >> 1) >= rows_y || 2 * (m0 + tid) + (j & 1) >= cols_y) s_out[(tid * 6 + j) * 64] = s_out[(tid * 6 + j - 1) * 64];
    }
    __syncthreads();

    // 6. the strip's blocks are consecutive in the output
    uint4* dst = reinterpret_cast<uint4*>(a.coef + ((int64_t)b * a.blocks + ((int64_t)r * a.mx + m0) * 6) * 64);
    const uint4* from = reinterpret_cast<const uint4*>(s_out);
    for (int i = tid; i < nm * 6 * 8; i += JT) dst[i] = from[i];
}

// ---- stage 2a: a wave codes a block ----

__device__ __forceinline__ int bit_length(int v) { return 32 - __clz(v < 0 ? -v : v); }  // of the magnitude; 0 for 0

__global__ __launch_bounds__(JT) void jpeg_code_blocks_kernel(const int16_t* __restrict__ coef, const uint32_t* __restrict__ huff, int64_t total, int64_t mcus,
                                                              uint32_t* __restrict__ slots, uint32_t* __restrict__ lens) {
    __shared__ uint32_t s_huff[4 * 256];
    __shared__ uint32_t s_slot[JT / 64][SLOT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 4 * 256; i += JT) s_huff[i] = huff[i];

    for (int64_t base = (int64_t)blockIdx.x * (JT / 64); base < total; base += (int64_t)gridDim.x * (JT / 64)) {  // (uniform trip count)
        const int64_t gb = base + wave;
        const bool active = gb < total;
        if (lane < SLOT) s_slot[wave][lane] = 0u;
        __syncthreads();
        unsigned nbits = 0;
        if (active) {
            const int c = (int)(gb % 6);  // every image holds a multiple of 6 blocks
            const int v = coef[gb * 64 + lane];
            const uint32_t* dc = s_huff + (c < 4 ? 0 : 512);
            const uint32_t* ac = dc + 256;
            const uint64_t nz = __ballot(v != 0) | 1ull;  // (bit 0, the DC, ends every run below it)
            uint64_t field = 0;  // this lane's bits, right-aligned
            unsigned len = 0;
            if (lane == 0) {
                // the previous block of the component: the block before (Y inside an MCU), or the same slot / Y(1,1) of the MCU before
                const int64_t mcu_in_image = (gb / 6) % mcus;
                const int back = (c >= 1 && c <= 3) ? 1 : (c == 0 ? 3 : 6);
                const int pred = (c >= 1 && c <= 3) || mcu_in_image > 0 ? (int)coef[(gb - back) * 64] : 0;
                const int diff = v - pred, n = bit_length(diff);
                const uint32_t e = dc[n & 255];
                const uint32_t vb = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u);
                field = ((uint64_t)(e >> 5) << n) | vb;
                len = (e & 31u) + (unsigned)n;
            } else if (v != 0) {
                const int prev = 63 - __clzll((long long)(nz & ((1ull << lane) - 1ull)));
                const int run = lane - 1 - prev, n = bit_length(v);
                const uint32_t zrl = ac[0xF0], e = ac[(((run & 15) << 4) | n) & 255];
                for (int z = 0; z < (run >> 4); ++z) field = (field << (zrl & 31u)) | (zrl >> 5), len += zrl & 31u;
                field = (field << (e & 31u)) | (e >> 5), len += e & 31u;
                field = (field << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), len += (unsigned)n;
            } else if (lane == 63) {
                field = ac[0] >> 5, len = ac[0] & 31u;  // the block ends in zeros: end-of-block
            }
            const unsigned inc = wave_scan_inclusive(len);
            nbits = (unsigned)__shfl((int)inc, 63, 64);
            const unsigned off = inc - len;
            if (len) {  // at most 59 bits: three words
                const uint64_t top = field << (64 - len);
                const unsigned w0 = off >> 5, s = off & 31u;
                const uint32_t p0 = (uint32_t)(top >> 32) >> s, p1 = (uint32_t)(top >> s), p2 = s ? (uint32_t)(top << (32 - s)) : 0u;
                if (p0 && w0 < SLOT) atomicOr(&s_slot[wave][w0], p0);
                if (p1 && w0 + 1 < SLOT) atomicOr(&s_slot[wave][w0 + 1], p1);
                if (p2 && w0 + 2 < SLOT) atomicOr(&s_slot[wave][w0 + 2], p2);
            }
            nbits = nbits < (unsigned)SLOT_BITS ? nbits : (unsigned)SLOT_BITS;  // (coefficients no encoder makes: wrong bytes, no access outside a slot)
        }
        __syncthreads();
        if (active) {
            if (lane < (int)((nbits + 31u) >> 5)) slots[gb * SLOT + lane] = s_slot[wave][lane];
            if (lane == 0) lens[gb] = nbits;
        }
        __syncthreads();
    }
}

// ---- stage 2b: exclusive prefix sum of an image's lengths ----

__global__ __launch_bounds__(JT) void jpeg_scan_kernel(const uint32_t* __restrict__ lens, int64_t blocks, uint64_t* __restrict__ offs,
                                                       int64_t* __restrict__ lengths) {
    __shared__ unsigned s_wave[JT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* l = lens + (int64_t)blockIdx.x * blocks;
    uint64_t* o = offs + (int64_t)blockIdx.x * (blocks + 1);
    uint64_t carry = 0;
    for (int64_t t0 = 0; t0 < blocks; t0 += TILE) {
        const int64_t i = t0 + 4 * tid;
        unsigned v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i + k < blocks ? l[i + k] : 0u, sum += v[k];
        const unsigned inc = wave_scan_inclusive(sum);  // (a tile holds at most 1024 * 1664 bits: 32 bits are enough inside it)
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < JT / 64; ++k) before += k < wave ? s_wave[k] : 0u, tile += s_wave[k];
        uint64_t at = carry + before + (inc - sum);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < blocks) o[i + k] = at;
            at += v[k];
        }
        carry += tile;
        __syncthreads();
    }
    if (tid == 0) o[blocks] = carry, lengths[blockIdx.x] = (int64_t)((carry + 7) >> 3);
}

// ---- stage 2c: every output word assembles itself ----

__global__ __launch_bounds__(JT) void jpeg_gather_kernel(const uint32_t* __restrict__ slots, const uint64_t* __restrict__ offs, int64_t blocks,
                                                         uint8_t* __restrict__ out, int64_t out_stride) {
    const int b = blockIdx.y;
    const uint64_t* o = offs + (int64_t)b * (blocks + 1);
    const uint32_t* sl = slots + (int64_t)b * blocks * SLOT;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + (int64_t)b * out_stride);
    const uint64_t total = o[blocks];
    const int64_t words = (int64_t)((total + 31) >> 5);
    for (int64_t j = (int64_t)blockIdx.x * JT + threadIdx.x; j < words; j += (int64_t)gridDim.x * JT) {
        const uint64_t pos = (uint64_t)j << 5;
        int64_t lo = 0, hi = blocks - 1;  // the last block that starts at or before pos (o[0] = 0)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (o[mid] <= pos) lo = mid;
            else hi = mid - 1;
        }
        int64_t i = lo;
        uint32_t word = 0;
        int filled = 0;
        uint64_t start = o[i];
        while (filled < 32 && i < blocks) {
            const uint64_t end = o[i + 1], at = pos + (uint64_t)filled;
            const int avail = (int)(end - at);  // (at >= start; a block is at most 1664 bits)
            if (avail > 0) {
                const int rel = (int)(at - start), take = min(avail, 32 - filled);
                const int wi = rel >> 5, s = rel & 31;
                const uint32_t* w = sl + i * SLOT + wi;
                uint64_t comb = (uint64_t)w[0] << 32;
                if (s + take > 32) comb |= w[1];
                const uint32_t bits = (uint32_t)((comb << s) >> (64 - take));
                word |= bits << (32 - filled - take);
                filled += take;
                if (take < avail) break;
            }
            ++i, start = end;
        }
        if (filled < 32) word |= 0xffffffffu >> filled;  // after the last block: 1-bits
        dst[j] = __builtin_bswap32(word);                // the first bit of the stream is the top bit of byte 0
    }
}

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_jpeg_plan(int batch, int h, int w, int64_t* plan) {
    W2E_REQUIRE(plan, "jpeg_plan: null plan");
    const char* why = check_dims("jpeg_plan", batch, h, w);
    W2E_REQUIRE(!why, "%s", why);
    const Geom g = geom(h, w);
    plan[0] = g.blocks, plan[1] = g.mx, plan[2] = g.my;
    plan[3] = (int64_t)batch * ((g.blocks + 1) * 8 + g.blocks * SLOT * 4 + g.blocks * 4);
    plan[4] = g.blocks * SLOT * 4;
    plan[5] = g.blocks * 64;
    plan[6] = (int64_t)batch * g.my * ceil_div(g.mx, SM);
    plan[7] = TILE;
    return 0;
}

extern "C" int w2e_jpeg_coefficients(const uint8_t* src, int batch, int h, int w, int quality, int16_t* coef, void* stream) {
    W2E_REQUIRE(src && coef, "jpeg_coefficients: null tensor");
    const char* why = check_dims("jpeg_coefficients", batch, h, w);
    W2E_REQUIRE(!why, "%s", why);
    W2E_REQUIRE(quality >= 1 && quality <= 100, "jpeg_coefficients: quality %d is not in 1..100", quality);
    W2E_REQUIRE((uintptr_t)coef % 16 == 0, "jpeg_coefficients: coef must be 16-byte aligned");
    if (batch == 0) return 0;
    const Geom g = geom(h, w);
    CoefArgs a;
    a.src = src, a.coef = coef, a.src_bytes = (int64_t)batch * h * w * 3, a.blocks = g.blocks;
    a.h = h, a.w = w, a.mx = g.mx, a.my = g.my, a.strips = (int)ceil_div(g.mx, SM);
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;  // jpeg_quality_scaling
    for (int i = 0; i < 64; ++i) {
        const int l = (LUMA_Q[i] * scale + 50) / 100, c = (CHROMA_Q[i] * scale + 50) / 100;  // jpeg_add_quant_table, force_baseline
        a.q[0][i] = (uint8_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        a.q[1][i] = (uint8_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
    const int64_t grid = (int64_t)batch * g.my * a.strips;
    W2E_REQUIRE(grid <= 0x7fffffff, "jpeg_coefficients: %lld strips in one call: split the batch", (long long)grid);
    jpeg_coefficients_kernel<<<(unsigned)grid, JT, 0, (hipStream_t)stream>>>(a);
    W2E_LAUNCH_CHECK("jpeg_coefficients");
    return 0;
}

extern "C" int w2e_jpeg_entropy(const int16_t* coef, int batch, int h, int w, const uint32_t* huff, uint8_t* out, int64_t out_stride,
                                int64_t* lengths, void* workspace, void* stream) {
    W2E_REQUIRE(coef && huff && out && lengths, "jpeg_entropy: null tensor");
    W2E_REQUIRE(workspace, "jpeg_entropy: null workspace (w2e_jpeg_plan: plan[3] bytes)");
    const char* why = check_dims("jpeg_entropy", batch, h, w);
    W2E_REQUIRE(!why, "%s", why);
    const Geom g = geom(h, w);
    W2E_REQUIRE(out_stride >= g.blocks * SLOT * 4, "jpeg_entropy: out_stride %lld is below the largest segment, %lld bytes (w2e_jpeg_plan: plan[4])",
                (long long)out_stride, (long long)(g.blocks * SLOT * 4));
    W2E_REQUIRE((uintptr_t)out % 4 == 0 && out_stride % 4 == 0, "jpeg_entropy: out and out_stride must be multiples of 4");
    W2E_REQUIRE((uintptr_t)workspace % 8 == 0 && (uintptr_t)lengths % 8 == 0, "jpeg_entropy: workspace and lengths must be 8-byte aligned");
    W2E_REQUIRE((uintptr_t)coef % 2 == 0 && (uintptr_t)huff % 4 == 0, "jpeg_entropy: coef / huff are not aligned to their element");
    W2E_REQUIRE(batch <= 65535, "jpeg_entropy: batch %d > 65535: split it", batch);
    if (batch == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)batch * g.blocks;
    uint64_t* offs = static_cast<uint64_t*>(workspace);
    uint32_t* slots = reinterpret_cast<uint32_t*>(offs + (int64_t)batch * (g.blocks + 1));
    uint32_t* lens = slots + total * SLOT;
    const int64_t mcus = g.blocks / 6;
    int64_t code_grid = ceil_div(total, JT / 64);
    if (code_grid > 16384) code_grid = 16384;
    jpeg_code_blocks_kernel<<<dim3((unsigned)code_grid, 1, 1), JT, 0, s>>>(coef, huff, total, mcus, slots, lens);
    W2E_LAUNCH_CHECK("jpeg_entropy (code)");
    jpeg_scan_kernel<<<batch, JT, 0, s>>>(lens, g.blocks, offs, lengths);
    W2E_LAUNCH_CHECK("jpeg_entropy (scan)");
    int64_t gather_grid = ceil_div(g.blocks * SLOT, (int64_t)JT * 8);
    if (gather_grid > 1024) gather_grid = 1024;
    jpeg_gather_kernel<<<dim3((unsigned)gather_grid, (unsigned)batch, 1), JT, 0, s>>>(slots, offs, g.blocks, out, out_stride);
    W2E_LAUNCH_CHECK("jpeg_entropy (gather)");
    return 0;
}
