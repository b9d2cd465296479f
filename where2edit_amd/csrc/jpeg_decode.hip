// Baseline JPEG decoding on the device (include/w2e_jpeg.h): the pixels of Pillow's Image.open(...).convert("RGB") for the coded file.
// The arithmetic is the specification (DESIGN.md "K17c"): Huffman decoding, libjpeg's accurate integer inverse DCT (jidctint), its
// fancy 4:2:0 chroma up-sampling, 16.16 fixed-point colour conversion.  Nothing here rounds in floating point.
//
// Stage 1, scan -> coefficients.  A Huffman stream has no entry points; the decoder makes them by self-synchronisation.  An image's
// scan (byte stuffing removed by the host) is cut into subsequences of sub_bits bits, ONE THREAD PER SUBSEQUENCE.  A decoder state is
// (p, slot, k): the bit position of the next symbol, the block's position in its MCU, the next zigzag index (0: a DC code is next).
// walk<MODE>() is the one decoder all passes share; it is a total function of the state:
//   * it decodes every symbol that STARTS before the subsequence's end (and before the end of the scan), the last one whole;
//   * bits that begin no code of the table advance p by one bit and change nothing else; a run that carries k past 63 ends the block;
//   * bits past the end of the scan read as 1; every loop is bounded by sub_bits; every table index is masked.
// So a corrupt file yields wrong states and a nonzero status, never an access outside a buffer and never an unbounded loop.
//   sync   every subsequence but the first starts from the guess (i sub_bits, 0, 0).  A workgroup owns 256 consecutive subsequences
//          of one image and iterates entry[i + 1] = f_i(entry[i]) among them in LDS, recomputing only where entry[i] changed, until
//          nothing changes (at most 256 rounds).  What it hands to the NEXT workgroup travels through a pair of buffers that
//          alternate by launch, so no kernel reads what another workgroup of the same launch writes; when it differs from what the
//          neighbour was handed this launch, the workgroup ORs 1 into the launch's "changed" word.  The host launches until that word
//          is 0: at most ceil(n / 256) + 1 times, since launch g + 1 makes workgroup g exact.  From the second launch on a workgroup
//          whose first entry did not change has nothing to do.
//   count  each thread walks its subsequence from its final entry and counts the blocks it completes; an exclusive prefix sum per
//          image (one workgroup walks the counts in tiles of 1024) gives every subsequence its first block, and the status.
//   write  each thread walks again and stores every coefficient it passes -- a run's zeros, the value, an end-of-block's zeros, the
//          DC as its difference -- so every element is written exactly once, a block that straddles subsequences by several threads
//          at disjoint indices.  Blocks at or past the image's count are decoded and not stored.
//   dc     one workgroup per (image, component) turns differences into values by a prefix sum in scan order (int32, fixed order).
// Code tables (the host builds them from the file's DHT lists; W2E_JPEG_TABLE_WORDS 32-bit words each, one per block position's
// component and class, staged in LDS): a first-level look-up on the next 9 bits, uint16 (length << 8) | symbol, 0 when the code is
// longer; then libjpeg's walk over maxcode[10..16] and valoffset.  No global atomics but the "changed" OR.
//
// Stage 2, coefficients -> pixels, two launches through a planar workspace of one byte per sample.
//   planes  a 256-thread workgroup takes 48 consecutive blocks: their coefficients come in as 16-byte loads, a thread takes one
//           column of one block (dequantise, jidctint pass 1, int32 [block][8][9] in LDS: the pad keeps both passes off one bank),
//           then one row (pass 2, + 128, clamp) and stores its 8 samples as one 8-byte word at the block's place in its plane.
//   colour  a thread takes 4 pixels of a row: Y as one 4-byte load; for 4:2:0 the 2 x 4 chroma samples around them (h2v2 fancy
//           up-sampling on the REAL ceil(h/2) x ceil(w/2) plane, the edge sample repeated beyond it); three 4-byte stores when the
//           rows are 4-byte aligned (w % 4 == 0), bytes otherwise.
#include "../../include/w2e_image.h"
#include "../../include/w2e_jpeg.h"
#include "device.h"

namespace w2e {
namespace {

constexpr int JT = 256;                       // threads of every workgroup here; also the subsequences of a workgroup
constexpr int TW = W2E_JPEG_TABLE_WORDS;      // 32-bit words of one code table
constexpr int T_MAXCODE = 256, T_VALOFF = 274, T_VALS = 320;  // word offsets inside a table: lut[512] u16 | maxcode[18] | valoff[17] | vals[256] u8
constexpr int PB = 48;                        // blocks per workgroup of the plane kernel
constexpr int MID_PITCH = 9;
constexpr int TILE = JT * 4;
static_assert(T_VALS + 64 == TW, "the table's layout fills W2E_JPEG_TABLE_WORDS");
static_assert(JT == W2E_JPEG_DECODE_GROUP, "a workgroup owns W2E_JPEG_DECODE_GROUP subsequences");

struct Geom {
    int mcu, per, comps, mx, my;  // MCU edge in pixels, blocks per MCU, components
    int64_t blocks;
};

Geom geom(int h, int w, int sampling) {
    Geom g;
    g.mcu = sampling == W2E_JPEG_420 ? 16 : 8;
    g.per = sampling == W2E_JPEG_420 ? 6 : (sampling == W2E_JPEG_444 ? 3 : 1);
    g.comps = sampling == W2E_JPEG_GREY ? 1 : 3;
    g.mx = (w + g.mcu - 1) / g.mcu, g.my = (h + g.mcu - 1) / g.mcu;
    g.blocks = (int64_t)g.per * g.mx * g.my;
    return g;
}

const char* check_common(const char* who, int batch, int h, int w, int sampling) {
    if (batch < 0 || batch > 65535) return refusal("%s: batch %d is not in 0..65535", who, batch);
    if (h < 1 || h > W2E_IMAGE_MAX_SIZE || w < 1 || w > W2E_IMAGE_MAX_SIZE)
        return refusal("%s: every size must be in 1..%d (got %d x %d)", who, W2E_IMAGE_MAX_SIZE, h, w);
    if (sampling != W2E_JPEG_420 && sampling != W2E_JPEG_444 && sampling != W2E_JPEG_GREY)
        return refusal("%s: sampling %d is none of W2E_JPEG_420 (0), W2E_JPEG_444 (1), W2E_JPEG_GREY (2)", who, sampling);
    return nullptr;
}

const char* check_stream(const char* who, int64_t scan_bits, int sub_bits) {
    if (sub_bits < 32 || sub_bits > 4096 || sub_bits % 32) return refusal("%s: sub_bits %d is no multiple of 32 in 32..4096", who, sub_bits);
    if (scan_bits < 0 || scan_bits > W2E_JPEG_MAX_SCAN_BITS)
        return refusal("%s: scan_bits %lld is not in 0..%lld", who, (long long)scan_bits, (long long)W2E_JPEG_MAX_SCAN_BITS);
    return nullptr;
}

int64_t subsequences(int64_t scan_bits, int sub_bits) {
    const int64_t n = ceil_div(scan_bits, sub_bits);
    return n < 1 ? 1 : n;
}

// the block position's component: 4:2:0 Y Y Y Y Cb Cr, 4:4:4 Y Cb Cr, grey Y
__device__ __forceinline__ int slot_component(int slot, int per) { return per == 6 ? (slot < 4 ? 0 : slot - 3) : slot; }

// ---- stage 1 ----

struct State {
    int p, sk;  // sk = slot << 8 | k
};
__device__ __forceinline__ bool same(const State a, const State b) { return a.p == b.p && a.sk == b.sk; }

struct Scan {
    const uint32_t* words;  // the image's scan, 4-byte aligned
    int nwords;             // words that hold any of its bits
    int bits;               // 8 * its bytes
};

struct StreamArgs {
    const uint8_t* scan;
    const int64_t* meta;     // [batch][2]: byte offset of the image's scan (a multiple of 4), its length in bits
    const uint32_t* tables;  // [batch][6][TW]
    State* entry;            // [batch][nsub]
    State* hand;             // [2][batch][groups]
    uint32_t* info;          // [batch][nsub]: blocks completed | flags << 24
    uint32_t* first;         // [batch][nsub]: the first block of each subsequence
    int16_t* coef;
    int* status;
    int* changed;
    int64_t nsub, groups, blocks, scan_bytes;  // scan_bytes: the size of the whole scan buffer
    int sub_bits, per, launch;
};

__device__ __forceinline__ Scan image_scan(const StreamArgs& a, int b) {
    Scan s;
    int64_t off = a.meta[2 * b] & ~(int64_t)3;  // (what the host says is clamped to the buffer: a wrong offset reads wrong bits, inside it)
    const int64_t bits = a.meta[2 * b + 1], room = a.scan_bytes & ~(int64_t)3;
    off = off < 0 ? 0 : (off > room ? room : off);
    s.words = reinterpret_cast<const uint32_t*>(a.scan + off);
    s.bits = (int)(bits < 0 ? 0 : (bits > W2E_JPEG_MAX_SCAN_BITS ? W2E_JPEG_MAX_SCAN_BITS : bits));
    const int64_t have = (room - off) >> 2, want = ((int64_t)s.bits + 31) >> 5;
    s.nwords = (int)(want < have ? want : have);
    return s;
}

__device__ __forceinline__ int image_subsequences(const Scan& s, const StreamArgs& a) {  // at most the batch's a.nsub
    const int64_t n = ((int64_t)s.bits + a.sub_bits - 1) / a.sub_bits;
    return (int)(n < 1 ? 1 : (n > a.nsub ? a.nsub : n));
}

__device__ __forceinline__ uint32_t scan_word(const Scan& s, int i) { return i < s.nwords ? __builtin_bswap32(s.words[i]) : 0xffffffffu; }

// One table: (length << 8) | symbol of the code that begins the 16 bits v, 0 when none does.
__device__ __forceinline__ uint32_t decode_symbol(const uint32_t* t, uint32_t v) {
    const uint32_t e = reinterpret_cast<const uint16_t*>(t)[v >> 7];
    if (e) return e;
    const int* maxcode = reinterpret_cast<const int*>(t + T_MAXCODE);
    const int* valoff = reinterpret_cast<const int*>(t + T_VALOFF);
#pragma unroll 1
    for (int l = 10; l <= 16; ++l) {
        const int code = (int)(v >> (16 - l));
        if (code <= maxcode[l]) return ((uint32_t)l << 8) | reinterpret_cast<const uint8_t*>(t + T_VALS)[(code + valoff[l]) & 255];
    }
    return 0u;
}

enum { SYNC = 0, COUNT = 1, WRITE = 2 };
constexpr uint32_t FLAG_CATEGORY = 2u, FLAG_INSIDE = 4u;

// Walk subsequence i of an image from state st.  s_tab: the image's tables in LDS, [component][DC, AC][TW].  Returns the blocks
// completed (COUNT, WRITE) and leaves the state it stops in in st.  WRITE: dst is the image's coefficients, `block` the index of the
// first block this walk completes or continues, `blocks` the image's count.
template <int MODE>
__device__ __forceinline__ int walk(const Scan& sc, const uint32_t* s_tab, int per, int sub_bits, int i, State& st, uint32_t& flags,
                                    int16_t* dst = nullptr, int64_t block = 0, int64_t blocks = 0) {
    const int64_t far = ((int64_t)i + 1) * sub_bits;
    const int end = (int)(far < sc.bits ? far : sc.bits);
    int p = st.p, slot = (st.sk >> 8) & 7, k = st.sk & 63, done = 0;
    if (slot >= per) slot = 0;
    int wi = -2;
    uint64_t window = 0;
    for (int it = 0; it < sub_bits && p < end && p >= 0; ++it) {  // (every step advances p by at least one bit)
        const int w = p >> 5;
        if (w != wi) window = ((uint64_t)scan_word(sc, w) << 32) | scan_word(sc, w + 1), wi = w;
        const uint32_t v = (uint32_t)((window << (p & 31)) >> 32);  // the 32 bits at p
        const uint32_t* t = s_tab + (2 * slot_component(slot, per) + (k ? 1 : 0)) * TW;
        const uint32_t e = decode_symbol(t, v >> 16);
        if (e == 0u) {
            ++p;
            continue;
        }
        const int length = (int)(e >> 8) & 31, sym = (int)(e & 255u), size = sym & 15;  // length + size <= 31
        int value = size ? (int)((v << length) >> (32 - size)) : 0;
        if (size && value < (1 << (size - 1))) value -= (1 << size) - 1;
        const bool store = MODE == WRITE && block + done < blocks;
        int16_t* o = MODE == WRITE ? dst + (block + done) * 64 : nullptr;
        bool finished = false;
        if (k == 0) {
            if (size > 11) flags |= FLAG_CATEGORY;
            if (store) o[0] = (int16_t)value;
            k = 1, p += length + size;
        } else if (size == 0 && sym != 0xF0) {
            if (store)
                for (int j = k; j < 64; ++j) o[j] = 0;
            p += length, finished = true;
        } else {
            if (size > 10) flags |= FLAG_CATEGORY;
            const int run = size == 0 ? 16 : sym >> 4;
            const int stop = k + run < 64 ? k + run : 64;
            if (store)
                for (int j = k; j < stop; ++j) o[j] = 0;
            k += run;
            if (size && k <= 63) {
                if (store) o[k] = (int16_t)value;
                ++k;
            }
            p += length + size, finished = k > 63;
        }
        if (finished) ++done, k = 0, slot = slot + 1 == per ? 0 : slot + 1;
    }
    st.p = p, st.sk = (slot << 8) | k;
    return done;
}

__device__ __forceinline__ void stage_tables(const StreamArgs& a, int b, uint32_t* s_tab) {
    const uint32_t* t = a.tables + (int64_t)b * 6 * TW;
    for (int j = threadIdx.x; j < 6 * TW; j += JT) s_tab[j] = t[j];
}

__global__ __launch_bounds__(JT) void jpeg_decode_sync_kernel(const StreamArgs a) {
    __shared__ uint32_t s_tab[6 * TW];
    __shared__ State s_e[JT + 1];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t g = blockIdx.x, i64 = g * JT + tid;
    const Scan sc = image_scan(a, b);
    const int n = image_subsequences(sc, a);
    if (g * JT >= n) return;  // (the whole workgroup: this image is shorter than the batch's longest)
    stage_tables(a, b, s_tab);
    const int i = (int)i64;
    const bool active = i < n;
    State* entry = a.entry + (int64_t)b * a.nsub;
    const State* in = a.hand + ((int64_t)(a.launch & 1) * gridDim.y + b) * a.groups;
    State* out = a.hand + ((int64_t)((a.launch + 1) & 1) * gridDim.y + b) * a.groups;
    State cur;
    cur.p = (int)((int64_t)i * a.sub_bits), cur.sk = 0;  // the guess; exact for subsequence 0
    bool dirty = active;
    if (a.launch > 0 && active) {
        const State old = entry[i];
        if (tid == 0 && g > 0) cur = in[g], dirty = !same(cur, old);
        else cur = old, dirty = false;
    }
    State handed;  // what the next workgroup was handed this launch
    handed.p = (int)(((int64_t)g + 1) * JT * a.sub_bits), handed.sk = 0;
    if (a.launch > 0 && tid == JT - 1 && g + 1 < a.groups) handed = in[g + 1];
    s_e[tid] = cur;
    if (tid == JT - 1) s_e[JT] = handed;
    __syncthreads();
    uint32_t flags = 0;
    for (int r = 0; r < JT; ++r) {
        bool ch = false;
        if (dirty) {
            State nx = cur;
            walk<SYNC>(sc, s_tab, a.per, a.sub_bits, i, nx, flags);
            ch = !same(nx, s_e[tid + 1]);
            if (ch) s_e[tid + 1] = nx;
        }
        if (!__syncthreads_or(ch)) break;
        const State nx = s_e[tid];
        dirty = active && !same(nx, cur);
        cur = nx;
        __syncthreads();
    }
    if (active) entry[i] = cur;
    if (tid == JT - 1 && g + 1 < a.groups && (g + 1) * JT < n) {
        const State tail = s_e[JT];
        out[g + 1] = tail;
        if (!same(tail, handed)) atomicOr(a.changed, 1);
    }
}

__global__ __launch_bounds__(JT) void jpeg_decode_count_kernel(const StreamArgs a) {
    __shared__ uint32_t s_tab[6 * TW];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t i64 = (int64_t)blockIdx.x * JT + tid;
    const Scan sc = image_scan(a, b);
    const int n = image_subsequences(sc, a);
    if ((int64_t)blockIdx.x * JT >= n) return;
    stage_tables(a, b, s_tab);
    __syncthreads();
    if (i64 >= n) return;
    const int i = (int)i64;
    State st = a.entry[(int64_t)b * a.nsub + i];
    uint32_t flags = 0;
    const int done = walk<COUNT>(sc, s_tab, a.per, a.sub_bits, i, st, flags);
    if (i == n - 1 && ((st.sk & 63) != 0 || st.p > sc.bits)) flags |= FLAG_INSIDE;
    a.info[(int64_t)b * a.nsub + i] = (uint32_t)done | (flags << 24);
}

// exclusive prefix sum of an image's block counts, and its status
__global__ __launch_bounds__(JT) void jpeg_decode_scan_kernel(const StreamArgs a) {
    __shared__ unsigned s_wave[JT / 64];
    __shared__ unsigned s_flags[JT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const Scan sc = image_scan(a, b);
    const int n = image_subsequences(sc, a);
    const uint32_t* info = a.info + (int64_t)b * a.nsub;
    uint32_t* first = a.first + (int64_t)b * a.nsub;
    unsigned carry = 0, flags = 0;  // (a subsequence completes at most sub_bits / 2 blocks; a corrupt scan's sum may wrap: it is compared, and used as a guarded index)
    for (int t0 = 0; t0 < n; t0 += TILE) {
        const int i = t0 + 4 * tid;
        unsigned v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = i + k < n ? info[i + k] : 0u;
            v[k] = w & 0xffffffu, sum += v[k], flags |= w >> 24;
        }
        const unsigned inc = wave_scan_inclusive(sum);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < JT / 64; ++k) before += k < wave ? s_wave[k] : 0u, tile += s_wave[k];
        unsigned at = carry + before + (inc - sum);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i + k < n) first[i + k] = at;
            at += v[k];
        }
        carry += tile;
        __syncthreads();
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) flags |= (unsigned)__shfl_xor((int)flags, off, 64);
    if (lane == 0) s_flags[wave] = flags;
    __syncthreads();
    if (tid == 0) {
        unsigned f = 0;
        for (int k = 0; k < JT / 64; ++k) f |= s_flags[k];
        a.status[b] = (int)((carry != (unsigned)a.blocks ? 1u : 0u) | (f & (FLAG_CATEGORY | FLAG_INSIDE)));
    }
}

__global__ __launch_bounds__(JT) void jpeg_decode_write_kernel(const StreamArgs a) {
    __shared__ uint32_t s_tab[6 * TW];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t i64 = (int64_t)blockIdx.x * JT + tid;
    const Scan sc = image_scan(a, b);
    const int n = image_subsequences(sc, a);
    if ((int64_t)blockIdx.x * JT >= n) return;
    stage_tables(a, b, s_tab);
    __syncthreads();
    if (i64 >= n) return;
    const int i = (int)i64;
    State st = a.entry[(int64_t)b * a.nsub + i];
    uint32_t flags = 0;
    walk<WRITE>(sc, s_tab, a.per, a.sub_bits, i, st, flags, a.coef + (int64_t)b * a.blocks * 64, (int64_t)a.first[(int64_t)b * a.nsub + i], a.blocks);
}

// DC differences -> values: component c's blocks in scan order
__global__ __launch_bounds__(JT) void jpeg_decode_dc_kernel(int16_t* __restrict__ coef, int64_t blocks, int per) {
    __shared__ unsigned s_wave[JT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.x;
    int16_t* base = coef + (int64_t)blockIdx.y * blocks * 64;
    const int64_t mcus = blocks / per;
    const int64_t count = per == 6 && c == 0 ? 4 * mcus : mcus;
    unsigned carry = 0;
    for (int64_t t0 = 0; t0 < count; t0 += TILE) {
        const int64_t j = t0 + 4 * tid;
        int64_t at[4];
        unsigned v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t jj = j + k;
            at[k] = per == 6 ? (c == 0 ? (jj >> 2) * 6 + (jj & 3) : jj * 6 + 3 + c) : jj * per + c;
            v[k] = jj < count ? (unsigned)(int)base[at[k] * 64] : 0u;
            sum += v[k];
        }
        const unsigned inc = wave_scan_inclusive(sum);
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < JT / 64; ++k) before += k < wave ? s_wave[k] : 0u, tile += s_wave[k];
        unsigned run = carry + before + (inc - sum);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            run += v[k];
            if (j + k < count) base[at[k] * 64] = (int16_t)(int)run;
        }
        carry += tile;
        __syncthreads();
    }
}

// ---- stage 2 ----

constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270, FIX_0_899976223 = 7373,
              FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137, FIX_1_961570560 = 16069, FIX_2_053119869 = 16819,
              FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;
// NATURAL[k]: the natural (row-major) index of the k-th coefficient of the zigzag scan; ZZ_OF[natural] is its inverse
__constant__ uint8_t ZZ_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                  10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of jidctint (jpeg_idct_islow) over d[0..7] in place, descaled by N bits: 11 for the columns, 18 for the rows.
template <int N>
__device__ __forceinline__ void idct_pass(int (&d)[8]) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * FIX_0_541196100;
    int t2 = z1 - z3 * FIX_1_847759065, t3 = z1 + z2 * FIX_0_765366865;
    int t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2;
    int z4 = t1 + t3;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    t0 *= FIX_0_298631336, t1 *= FIX_2_053119869, t2 *= FIX_3_072711026, t3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223, z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5, z4 = z4 * -FIX_0_390180644 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    d[0] = descale(t10 + t3, N), d[7] = descale(t10 - t3, N);
    d[1] = descale(t11 + t2, N), d[6] = descale(t11 - t2, N);
    d[2] = descale(t12 + t1, N), d[5] = descale(t12 - t1, N);
    d[3] = descale(t13 + t0, N), d[4] = descale(t13 - t0, N);
}

struct PlaneArgs {
    const int16_t* coef;
    const int* q;      // [batch][3][64], natural order
    uint8_t* planes;   // [batch][64 * blocks]: Y, then Cb, then Cr
    int64_t blocks;
    int per, mx, my, groups;  // groups: workgroups per image
};

// Where the planes of an image lie in its 64 * blocks bytes, and their pitch: 4:2:0 Y [16 my][16 mx], Cb and Cr [8 my][8 mx];
// otherwise every plane [8 my][8 mx].
__device__ __forceinline__ int plane_pitch(int c, int per, int mx) { return per == 6 && c == 0 ? 16 * mx : 8 * mx; }
__device__ __forceinline__ int64_t plane_offset(int c, int per, int mx, int my) {
    const int64_t mcus = (int64_t)mx * my;
    return per == 6 ? (c == 0 ? 0 : (256 + 64 * (c - 1)) * mcus) : 64 * c * mcus;
}

__global__ __launch_bounds__(JT) void jpeg_planes_kernel(const PlaneArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t s_coef[PB * 64];
    __shared__ int s_mid[PB * 8 * MID_PITCH];
    __shared__ int s_q[3 * 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.groups;
    const int64_t b0 = (int64_t)(blockIdx.x - b * a.groups) * PB;
    const int nb = (int)(a.blocks - b0 < PB ? a.blocks - b0 : PB);
    if (tid < 3 * 64) s_q[tid] = a.q[b * 192 + tid];
    const uint4* src = reinterpret_cast<const uint4*>(a.coef + ((int64_t)b * a.blocks + b0) * 64);
    for (int i = tid; i < nb * 8; i += JT) reinterpret_cast<uint4*>(s_coef)[i] = src[i];
    __syncthreads();
    for (int i = tid; i < nb * 8; i += JT) {  // columns
        const int blk = i >> 3, col = i & 7;
        const int* q = s_q + 64 * slot_component((int)((b0 + blk) % a.per), a.per);
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (int)s_coef[blk * 64 + ZZ_OF[8 * k + col]] * q[8 * k + col];
        idct_pass<11>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) s_mid[(blk * 8 + k) * MID_PITCH + col] = d[k];
    }
    __syncthreads();
    uint8_t* planes = a.planes + (int64_t)b * a.blocks * 64;
    for (int i = tid; i < nb * 8; i += JT) {  // rows
        const int blk = i >> 3, row = i & 7;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = s_mid[i * MID_PITCH + k];
        idct_pass<18>(d);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= (uint32_t)min(max(d[k] + 128, 0), 255) << (8 * k);
            hi |= (uint32_t)min(max(d[k + 4] + 128, 0), 255) << (8 * k);
        }
        const int64_t gb = b0 + blk, mcu = gb / a.per;
        const int slot = (int)(gb - mcu * a.per), c = slot_component(slot, a.per);
        const int m_y = (int)(mcu / a.mx), m_x = (int)(mcu - (int64_t)m_y * a.mx);
        const int by = a.per == 6 && c == 0 ? 2 * m_y + (slot >> 1) : m_y, bx = a.per == 6 && c == 0 ? 2 * m_x + (slot & 1) : m_x;
        uint8_t* dst = planes + plane_offset(c, a.per, a.mx, a.my) + (int64_t)(8 * by + row) * plane_pitch(c, a.per, a.mx) + 8 * bx;
        *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);  // (every offset and pitch is a multiple of 8)
    }
}

constexpr int FIX_1_40200 = 91881, FIX_1_77200 = 116130, FIX_0_71414 = 46802, FIX_0_34414 = 22554;  // int(x * 65536 + .5)

struct ColourArgs {
    const uint8_t* planes;
    uint8_t* out;  // [batch][h][w][3]
    int64_t blocks;
    int h, w, per, mx, my, quads;  // quads: ceil(w / 4)
};

__global__ __launch_bounds__(JT) void jpeg_colour_kernel(const ColourArgs a) {
    const int64_t total = (int64_t)a.h * a.quads;
    const int b = blockIdx.y;
    const uint8_t* planes = a.planes + (int64_t)b * a.blocks * 64;
    const uint8_t* py = planes;
    const uint8_t* pc[2] = {planes + plane_offset(1, a.per, a.mx, a.my), planes + plane_offset(2, a.per, a.mx, a.my)};
    const int ypitch = plane_pitch(0, a.per, a.mx), cpitch = 8 * a.mx;
    const int ch = (a.h + 1) >> 1, cw = (a.w + 1) >> 1;
    const bool aligned = (a.w & 3) == 0;
    for (int64_t t = (int64_t)blockIdx.x * JT + threadIdx.x; t < total; t += (int64_t)gridDim.x * JT) {
        const int y = (int)(t / a.quads), x0 = 4 * (int)(t - (int64_t)y * a.quads);
        const uint32_t yy = *reinterpret_cast<const uint32_t*>(py + (int64_t)y * ypitch + x0);  // (the pitch is a multiple of 8: inside the plane)
        int cc[2][4];
        if (a.per == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) cc[0][k] = cc[1][k] = 128;
        } else if (a.per == 3) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t v = *reinterpret_cast<const uint32_t*>(pc[c] + (int64_t)y * cpitch + x0);
#pragma unroll
                for (int k = 0; k < 4; ++k) cc[c][k] = (int)((v >> (8 * k)) & 255u);
            }
        } else {
            const int cy = y >> 1, fy = min(max(cy + ((y & 1) ? 1 : -1), 0), ch - 1);
            const int i0 = x0 >> 1;  // the chroma columns i0, i0 + 1 and their neighbours, clamped to the real plane
            int col[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) col[k] = min(max(i0 - 1 + k, 0), cw - 1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint8_t* near = pc[c] + (int64_t)cy * cpitch;
                const uint8_t* farr = pc[c] + (int64_t)fy * cpitch;
                int s[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = 3 * (int)near[col[k]] + (int)farr[col[k]];
                cc[c][0] = (3 * s[1] + s[0] + 8) >> 4, cc[c][1] = (3 * s[1] + s[2] + 7) >> 4;
                cc[c][2] = (3 * s[2] + s[1] + 8) >> 4, cc[c][3] = (3 * s[2] + s[3] + 7) >> 4;
            }
        }
        uint8_t rgb[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int Y = (int)((yy >> (8 * k)) & 255u), cb = cc[0][k] - 128, cr = cc[1][k] - 128;
            rgb[3 * k + 0] = (uint8_t)min(max(Y + ((FIX_1_40200 * cr + 32768) >> 16), 0), 255);
            rgb[3 * k + 1] = (uint8_t)min(max(Y + ((-FIX_0_34414 * cb - FIX_0_71414 * cr + 32768) >> 16), 0), 255);
            rgb[3 * k + 2] = (uint8_t)min(max(Y + ((FIX_1_77200 * cb + 32768) >> 16), 0), 255);
        }
        uint8_t* dst = a.out + (((int64_t)b * a.h + y) * a.w + x0) * 3;
        if (aligned) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                reinterpret_cast<uint32_t*>(dst)[k] = (uint32_t)rgb[4 * k] | (uint32_t)rgb[4 * k + 1] << 8 | (uint32_t)rgb[4 * k + 2] << 16 | (uint32_t)rgb[4 * k + 3] << 24;
        } else {
            const int nbytes = 3 * min(4, a.w - x0);
#pragma unroll
            for (int k = 0; k < 12; ++k)
                if (k < nbytes) dst[k] = rgb[k];
        }
    }
}

const char* fill_stream_args(const char* who, StreamArgs& a, const uint8_t* scan, const int64_t* meta, const uint32_t* tables, int64_t scan_bytes, int batch,
                             int h, int w, int sampling, int64_t scan_bits, int sub_bits, void* workspace) {
    if (!scan || !meta || !tables) return refusal("%s: null tensor", who);
    if (!workspace) return refusal("%s: null workspace (w2e_jpeg_decode_plan: plan[4] bytes)", who);
    const char* why = check_common(who, batch, h, w, sampling);
    if (!why) why = check_stream(who, scan_bits, sub_bits);
    if (why) return why;
    if (scan_bytes < 0 || scan_bytes % 4) return refusal("%s: scan_bytes %lld is no multiple of 4 (the host pads every scan with 0xFF)", who, (long long)scan_bytes);
    if ((uintptr_t)scan % 4 || (uintptr_t)tables % 4 || (uintptr_t)meta % 8 || (uintptr_t)workspace % 8)
        return refusal("%s: scan and tables must be 4-byte aligned, meta and workspace 8-byte aligned", who);
    const Geom g = geom(h, w, sampling);
    a.scan = scan, a.meta = meta, a.tables = tables, a.scan_bytes = scan_bytes;
    a.nsub = subsequences(scan_bits, sub_bits), a.groups = ceil_div(a.nsub, JT), a.blocks = g.blocks;
    a.entry = static_cast<State*>(workspace);
    a.hand = a.entry + (int64_t)batch * a.nsub;
    a.info = reinterpret_cast<uint32_t*>(a.hand + 2 * (int64_t)batch * a.groups);
    a.first = a.info + (int64_t)batch * a.nsub;
    a.coef = nullptr, a.status = nullptr, a.changed = nullptr;
    a.sub_bits = sub_bits, a.per = g.per, a.launch = 0;
    return nullptr;
}

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_jpeg_decode_plan(int batch, int h, int w, int sampling, int64_t scan_bits, int sub_bits, int64_t* plan) {
    W2E_REQUIRE(plan, "jpeg_decode_plan: null plan");
    const char* why = check_common("jpeg_decode_plan", batch, h, w, sampling);
    if (!why) why = check_stream("jpeg_decode_plan", scan_bits, sub_bits);
    W2E_REQUIRE(!why, "%s", why);
    const Geom g = geom(h, w, sampling);
    const int64_t n = subsequences(scan_bits, sub_bits), groups = ceil_div(n, JT);
    plan[0] = g.blocks, plan[1] = g.mx, plan[2] = g.my;
    plan[3] = n;
    plan[4] = (int64_t)batch * 16 * (n + groups);
    plan[5] = (int64_t)batch * g.blocks * 64;
    plan[6] = groups + 1;
    plan[7] = g.blocks * 64;
    return 0;
}

extern "C" int w2e_jpeg_decode_sync(const uint8_t* scan, const int64_t* meta, const uint32_t* tables, int64_t scan_bytes, int batch, int h, int w,
                                    int sampling, int64_t scan_bits, int sub_bits, int launch, void* workspace, int32_t* changed, void* stream) {
    StreamArgs a;
    const char* why = fill_stream_args("jpeg_decode_sync", a, scan, meta, tables, scan_bytes, batch, h, w, sampling, scan_bits, sub_bits, workspace);
    W2E_REQUIRE(!why, "%s", why);
    W2E_REQUIRE(changed && (uintptr_t)changed % 4 == 0, "jpeg_decode_sync: changed must be a 4-byte aligned word (zero before the call)");
    W2E_REQUIRE(launch >= 0 && launch <= a.groups, "jpeg_decode_sync: launch %d is not in 0..%lld (w2e_jpeg_decode_plan: plan[6] launches at most)", launch,
                (long long)a.groups);
    if (batch == 0) return 0;
    a.changed = changed, a.launch = launch;
    jpeg_decode_sync_kernel<<<dim3((unsigned)a.groups, (unsigned)batch, 1), JT, 0, (hipStream_t)stream>>>(a);
    W2E_LAUNCH_CHECK("jpeg_decode_sync");
    return 0;
}

extern "C" int w2e_jpeg_decode_coefficients(const uint8_t* scan, const int64_t* meta, const uint32_t* tables, int64_t scan_bytes, int batch, int h, int w,
                                            int sampling, int64_t scan_bits, int sub_bits, void* workspace, int16_t* coef, int32_t* status, void* stream) {
    StreamArgs a;
    const char* why = fill_stream_args("jpeg_decode_coefficients", a, scan, meta, tables, scan_bytes, batch, h, w, sampling, scan_bits, sub_bits, workspace);
    W2E_REQUIRE(!why, "%s", why);
    W2E_REQUIRE(coef && status, "jpeg_decode_coefficients: null tensor");
    W2E_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)status % 4 == 0, "jpeg_decode_coefficients: coef must be 16-byte aligned, status 4-byte aligned");
    if (batch == 0) return 0;
    a.coef = coef, a.status = status;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.groups, (unsigned)batch, 1);
    jpeg_decode_count_kernel<<<grid, JT, 0, s>>>(a);
    W2E_LAUNCH_CHECK("jpeg_decode_coefficients (count)");
    jpeg_decode_scan_kernel<<<batch, JT, 0, s>>>(a);
    W2E_LAUNCH_CHECK("jpeg_decode_coefficients (scan)");
    jpeg_decode_write_kernel<<<grid, JT, 0, s>>>(a);
    W2E_LAUNCH_CHECK("jpeg_decode_coefficients (write)");
    const Geom g = geom(h, w, sampling);
    jpeg_decode_dc_kernel<<<dim3((unsigned)g.comps, (unsigned)batch, 1), JT, 0, s>>>(coef, g.blocks, g.per);
    W2E_LAUNCH_CHECK("jpeg_decode_coefficients (dc)");
    return 0;
}

extern "C" int w2e_jpeg_pixels(const int16_t* coef, const int32_t* qtables, int batch, int h, int w, int sampling, uint8_t* out, void* workspace,
                               void* stream) {
    W2E_REQUIRE(coef && qtables && out, "jpeg_pixels: null tensor");
    W2E_REQUIRE(workspace, "jpeg_pixels: null workspace (w2e_jpeg_decode_plan: plan[5] bytes)");
    const char* why = check_common("jpeg_pixels", batch, h, w, sampling);
    W2E_REQUIRE(!why, "%s", why);
    W2E_REQUIRE((uintptr_t)coef % 16 == 0 && (uintptr_t)workspace % 16 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)qtables % 4 == 0,
                "jpeg_pixels: coef and workspace must be 16-byte aligned, out and qtables 4-byte aligned");
    if (batch == 0) return 0;
    const Geom g = geom(h, w, sampling);
    hipStream_t s = (hipStream_t)stream;
    PlaneArgs p;
    p.coef = coef, p.q = qtables, p.planes = static_cast<uint8_t*>(workspace), p.blocks = g.blocks;
    p.per = g.per, p.mx = g.mx, p.my = g.my, p.groups = (int)ceil_div(g.blocks, PB);
    const int64_t grid = (int64_t)batch * p.groups;
    W2E_REQUIRE(grid <= 0x7fffffff, "jpeg_pixels: %lld workgroups in one call: split the batch", (long long)grid);
    jpeg_planes_kernel<<<(unsigned)grid, JT, 0, s>>>(p);
    W2E_LAUNCH_CHECK("jpeg_pixels (planes)");
    ColourArgs c;
    c.planes = p.planes, c.out = out, c.blocks = g.blocks;
    c.h = h, c.w = w, c.per = g.per, c.mx = g.mx, c.my = g.my, c.quads = (w + 3) / 4;
    jpeg_colour_kernel<<<dim3((unsigned)stream_grid((int64_t)h * c.quads, JT), (unsigned)batch, 1), JT, 0, s>>>(c);
    W2E_LAUNCH_CHECK("jpeg_pixels (colour)");
    return 0;
}
