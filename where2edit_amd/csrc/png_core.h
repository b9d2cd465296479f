// The PNG decoder's core as host-and-device code: the bit reader, the construction of the decode tables, the symbol decode, the
// bounds logic, the Adler-32 and the row filters (include/w2e_png.h; DESIGN.md "K17d").  csrc/png.hip compiles it into the kernels, with
// `lanes` = 64 (one wave per stream); tests/png_core_host.cpp compiles the same text into a stand-alone host program with `lanes` = 1,
// so that the robustness rules below can be run under the sanitizers without a GPU.
//
// The rules (a corrupt stream gives a nonzero status and garbage, never an access outside a buffer, never an unbounded loop):
//   * every iteration of the block loop and of the symbol loop consumes at least one input bit, and the loop ends as soon as more bits
//     were consumed than the stream has (W2E_PNG_STATUS_INPUT): the loops are bounded by the stream's bits;
//   * the input is read through a window that is filled with clamped loads: a byte past the stream reads as 0;
//   * every write goes to the ring (index masked) and leaves it through flush(), which is clamped to the expected size; a symbol that
//     would pass the expected size raises W2E_PNG_STATUS_LONG BEFORE anything is written;
//   * every table index is masked or compared with the table's size;
//   * the first status that is raised ends the decoding.
//
// Everything here is uniform across the lanes except where `lane` appears: all lanes hold the same reader state and take the same
// branches; the lanes share the work of filling the window, building the tables, copying a match and flushing the ring.
#pragma once
#include <stdint.h>

#include "../../include/w2e_png.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNG_HD __host__ __device__ __forceinline__
#else
#define PNG_HD inline
#endif

namespace w2e {
namespace png {

constexpr int RING = 32768;      // the deflate window: a distance reaches at most this far back
constexpr int IN_WORDS = 256;    // 32-bit words of the input window
constexpr int LIT_FAST = 10;     // bits of the literal/length code's direct table; a longer code walks the counts
constexpr int DIST_FAST = 8;     // the same for the distance code (and, with 7 bits of it, for the code-length code)
constexpr int FLUSH = 2048;      // bytes that leave the ring at once (a multiple of 4)
constexpr int MAX_LIT = 288, MAX_DIST = 32, MAX_LENS = 320;

// What a workgroup keeps in LDS (on the host: one heap object).  About 38 KiB: four streams per CU.
struct Shared {
    uint8_t ring[RING];
    uint32_t in[IN_WORDS];
    uint16_t lit_fast[1 << LIT_FAST];    // entry [next bits] = (symbol << 4) | length of the code that begins them, 0 when none does
    uint16_t dist_fast[1 << DIST_FAST];
    uint16_t lit_sym[MAX_LIT], dist_sym[MAX_DIST];  // the symbols in code order
    uint16_t lit_count[16], dist_count[16];         // codes of each length
    uint16_t code_of[MAX_LENS];                     // scratch of the builder: the code of each symbol,
    uint16_t offs[16], next[16];                    // the first index and the first code of each length
    uint8_t lens[MAX_LENS];                         // the code lengths of the block being opened
    int32_t flag;                                   // lane 0's verdict on a code-length set, for the others
};

// The cooperative steps.  On the device the workgroup is ONE wave, so the barrier costs a wait for the wave's own LDS traffic.
struct Lanes {
    int lane, lanes;
    PNG_HD void sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
    // A value that is the same in every lane, said so: what is read from LDS lands in vector registers, and everything computed from
    // it -- the whole reader state -- would stay there; from here on the compiler keeps it in scalar registers and branches on it
    // without a vote.
    PNG_HD uint32_t uniform(uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        v = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#endif
        return v;
    }
    PNG_HD uint32_t sum(uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
#endif
        return v;
    }
};

PNG_HD uint32_t reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// Length symbol 257..285 -> (base length, extra bits); distance symbol 0..29 -> (base distance, extra bits): RFC 1951, 3.2.5, as
// arithmetic (a table would be a global load per symbol).
PNG_HD void length_base(int sym, int& base, int& extra) {
    if (sym < 265) { base = sym - 254, extra = 0; return; }
    if (sym == 285) { base = 258, extra = 0; return; }
    extra = (sym - 261) >> 2;
    base = 3 + ((4 + ((sym - 261) & 3)) << extra);
}
PNG_HD void distance_base(int sym, int& base, int& extra) {
    if (sym < 4) { base = sym + 1, extra = 0; return; }
    extra = (sym >> 1) - 1;
    base = 1 + ((2 + (sym & 1)) << extra);
}

// ---- the row filters (PNG specification, 9.2): the reconstructed byte from the filtered one, a = left, b = above, c = above left ----
PNG_HD int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
PNG_HD uint8_t unfilter(int filter, int x, int a, int b, int c) {
    switch (filter) {
        case 1: return (uint8_t)(x + a);
        case 2: return (uint8_t)(x + b);
        case 3: return (uint8_t)(x + ((a + b) >> 1));
        case 4: return (uint8_t)(x + paeth(a, b, c));
        default: return (uint8_t)x;  // 0, and a filter byte above 4 (the caller raises W2E_PNG_STATUS_FILTER)
    }
}

// ---- inflate ----
struct Inflate {
    Shared& sh;
    const Lanes L;
    const uint8_t* streams;   // the whole buffer (4-byte aligned), stream_bytes long (a multiple of 4)
    int64_t stream_bytes, off, len;  // this stream: [off, off + len) of it, off a multiple of 4
    uint8_t* raw;             // this stream's output row (4-byte aligned)
    int64_t expected;         // bytes it must inflate to (the caller has clamped it to the row)
    // the reader: `hold` has `nbits` valid bits; the next word to load is at byte `inpos` of the stream; the window holds the words
    // from byte `inbase` on
    uint64_t hold;
    int nbits;
    int64_t inpos, inbase;
    // the writer
    int64_t outpos, flushed;
    uint32_t adler_a, adler_b;
    int status;

    PNG_HD Inflate(Shared& s, Lanes l, const uint8_t* streams_, int64_t stream_bytes_, int64_t off_, int64_t len_, uint8_t* raw_, int64_t expected_)
        : sh(s), L(l), streams(streams_), stream_bytes(stream_bytes_), off(off_), len(len_), raw(raw_), expected(expected_), hold(0), nbits(0),
          inpos(0), inbase(-1), outpos(0), flushed(0), adler_a(1), adler_b(0), status(0) {}

    // -- input --
    PNG_HD void fill_window() {
        L.sync();
        for (int k = L.lane; k < IN_WORDS; k += L.lanes) {
            const int64_t o = inbase + 4 * (int64_t)k;  // byte of this stream
            uint32_t w = 0;
            if (o < len && off + o + 4 <= stream_bytes) {
                w = reinterpret_cast<const uint32_t*>(streams)[(off + o) >> 2];
                if (o + 4 > len) w &= (1u << (8 * (int)(len - o))) - 1u;  // the bytes past this stream's end read as 0
            }
            sh.in[k] = w;
        }
        L.sync();
    }
    PNG_HD void refill() {  // afterwards nbits >= 32
        if (nbits < 32) {
            if (inbase < 0 || inpos - inbase >= 4 * IN_WORDS) {
                inbase = inpos;
                fill_window();
            }
            hold |= (uint64_t)L.uniform(sh.in[((inpos - inbase) >> 2) & (IN_WORDS - 1)]) << nbits;
            nbits += 32, inpos += 4;
        }
    }
    PNG_HD uint32_t take(int n) {  // n <= 32 bits of the nbits that are there
        const uint32_t v = (uint32_t)(hold & ((n >= 32) ? 0xffffffffull : ((1ull << n) - 1)));
        hold >>= n, nbits -= n;
        return v;
    }
    PNG_HD bool past_end() const { return 8 * inpos - nbits > 8 * len; }  // more bits consumed than the stream has

    // -- tables --
    // The code of n symbols with lengths lens[0..n) (each 0..15): count[], sym[] for the walk and the direct table of `fast` bits.
    // Returns false for an over-subscribed set.  An incomplete set is taken: a code that no symbol has decodes to -1.
    PNG_HD bool build(const uint8_t* lens, int n, uint16_t* count, uint16_t* sym, uint16_t* fast_table, int fast) {
        L.sync();
        for (int i = L.lane; i < (1 << fast); i += L.lanes) fast_table[i] = 0;
        if (L.lane == 0) {
            for (int l = 0; l < 16; ++l) count[l] = 0;
            for (int s = 0; s < n; ++s) ++count[lens[s] & 15];
            int left = 1, over = 0;
            for (int l = 1; l < 16; ++l) {
                left = 2 * left - count[l];
                if (left < 0) { over = 1; break; }
            }
            sh.flag = over;
            if (!over) {
                uint16_t* const offs = sh.offs;
                uint16_t* const next = sh.next;
                offs[1] = 0, next[1] = 0;
                for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + count[l], next[l + 1] = (uint16_t)((next[l] + count[l]) << 1);
                for (int s = 0; s < n; ++s) {
                    const int l = lens[s] & 15;
                    if (l) sym[offs[l]++] = (uint16_t)s, sh.code_of[s] = next[l]++;
                }
            }
        }
        L.sync();
        if (L.uniform((uint32_t)sh.flag)) return false;
        for (int s = L.lane; s < n; s += L.lanes) {
            const int l = lens[s] & 15;
            if (l && l <= fast) {
                const uint32_t r = reverse_bits(sh.code_of[s], l);
                for (uint32_t k = 0; k < (1u << (fast - l)); ++k) fast_table[(r | (k << l)) & ((1u << fast) - 1)] = (uint16_t)((s << 4) | l);
            }
        }
        L.sync();
        return true;
    }
    // The next symbol of a code of n symbols, or -1 when the bits match none.  Consumes at least one bit either way.
    PNG_HD int decode(const uint16_t* count, const uint16_t* sym, int n, const uint16_t* fast_table, int fast) {
        const uint32_t e = L.uniform(fast_table[(uint32_t)hold & ((1u << fast) - 1)]);
        if (e) {
            take((int)(e & 15));
            return (int)(e >> 4);
        }
        int code = 0, first = 0, index = 0;
        for (int l = 1; l < 16; ++l) {
            code |= (int)((hold >> (l - 1)) & 1);
            const int c = (int)L.uniform(count[l]);
            if (code - c < first) {
                take(l);
                const int at = index + (code - first);
                return at < n ? (int)L.uniform(sym[at]) : -1;
            }
            index += c, first += c;
            first <<= 1, code <<= 1;
        }
        take(15);
        return -1;
    }

    // -- output --
    // n bytes (n <= FLUSH + 3, flushed a multiple of 4) leave the ring for raw[flushed, flushed + n), and enter the Adler-32.
    PNG_HD void flush_chunk(int n) {
        L.sync();
        uint32_t s1 = 0, s2 = 0;
        const int words = (n + 3) >> 2;
        for (int k = L.lane; k < words; k += L.lanes) {
            const int64_t at = flushed + 4 * (int64_t)k;
            const uint32_t w = *reinterpret_cast<const uint32_t*>(&sh.ring[at & (RING - 1)]);
            const int here = n - 4 * k < 4 ? n - 4 * k : 4;
            for (int j = 0; j < here; ++j) {
                const uint32_t byte = (w >> (8 * j)) & 255u;
                s1 += byte, s2 += byte * (uint32_t)(n - (4 * k + j));
            }
            if (here == 4 && at + 4 <= expected) {
                *reinterpret_cast<uint32_t*>(raw + at) = w;
            } else {
                for (int j = 0; j < here; ++j)
                    if (at + j < expected) raw[at + j] = (uint8_t)(w >> (8 * j));
            }
        }
        s1 = L.uniform(L.sum(s1)), s2 = L.uniform(L.sum(s2));
        adler_b = (uint32_t)((adler_b + (uint64_t)n * adler_a + s2) % 65521u);
        adler_a = (adler_a + s1) % 65521u;
        flushed += n;
    }
    PNG_HD void flush_full() {
        while (outpos - flushed >= FLUSH) flush_chunk(FLUSH);
    }
    PNG_HD void flush_rest() {
        flush_full();
        if (outpos > flushed) flush_chunk((int)(outpos - flushed));
    }
    PNG_HD void put(uint8_t v) {
        if (L.lane == 0) sh.ring[outpos & (RING - 1)] = v;
        ++outpos;
    }
    // A match: n bytes (3..258) from dist back (1..32768, not before the start: the caller checked).  All lanes, `lanes` bytes per
    // round.  A distance of at least `lanes` never reaches into its own round, and the rounds follow one another (LDS operations of
    // one wave complete in order), so byte i comes from i - dist as in the serial copy.  A shorter distance overlaps within a round:
    // the source then repeats with a period of dist, and every lane reads a byte that was there before the match began (a run,
    // dist = 1, is the common case and needs no division).
    PNG_HD void copy(int n, int dist) {
        L.sync();
        const int64_t from = outpos - dist;
        for (int i = L.lane; i < n; i += L.lanes) {
            const int j = dist >= L.lanes ? i : (dist == 1 ? 0 : i % dist);
            sh.ring[(outpos + i) & (RING - 1)] = sh.ring[(from + j) & (RING - 1)];
        }
        outpos += n;
    }

    // -- blocks --
    PNG_HD void stored() {
        take(nbits & 7);  // to the byte boundary
        refill();
        const uint32_t v = take(32);
        const int n = (int)(v & 0xffffu);
        if (past_end()) { status |= W2E_PNG_STATUS_INPUT; return; }
        if (n != (int)((~v >> 16) & 0xffffu)) { status |= W2E_PNG_STATUS_STORED; return; }
        if (outpos + n > expected) { status |= W2E_PNG_STATUS_LONG; return; }
        // the bytes are whole from here on: take them from the reader four at a time (nbits is a multiple of 8)
        int left = n;
        while (left > 0) {
            refill();
            if (past_end()) { status |= W2E_PNG_STATUS_INPUT; return; }
            int here = nbits >> 3;
            if (here > 4) here = 4;
            if (here > left) here = left;
            const uint32_t w = take(8 * here);
            for (int j = 0; j < here; ++j) put((uint8_t)(w >> (8 * j)));
            left -= here;
            if (outpos - flushed >= FLUSH) flush_full();
        }
    }
    PNG_HD bool fixed_tables() {
        for (int s = L.lane; s < MAX_LENS; s += L.lanes) sh.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
        return build(sh.lens, 288, sh.lit_count, sh.lit_sym, sh.lit_fast, LIT_FAST) &&
               build(sh.lens + 288, 30, sh.dist_count, sh.dist_sym, sh.dist_fast, DIST_FAST);
    }
    PNG_HD bool dynamic_tables(int& nlit, int& ndist) {
        refill();
        nlit = (int)take(5) + 257, ndist = (int)take(5) + 1;
        const int ncode = (int)take(4) + 4;
        if (nlit > 286 || ndist > 30) return false;
        const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        L.sync();
        for (int s = L.lane; s < 19; s += L.lanes) sh.lens[s] = 0;
        L.sync();
        for (int i = 0; i < ncode; ++i) {
            refill();
            const uint8_t l = (uint8_t)take(3);
            if (L.lane == 0) sh.lens[order[i]] = l;
        }
        // the code-length code borrows the distance code's tables
        if (!build(sh.lens, 19, sh.dist_count, sh.dist_sym, sh.dist_fast, 7)) return false;
        int at = 0, prev = -1;
        while (at < nlit + ndist) {
            refill();
            if (past_end()) return false;
            const int s = decode(sh.dist_count, sh.dist_sym, 19, sh.dist_fast, 7);
            if (s < 0) return false;
            if (s < 16) {
                if (L.lane == 0) sh.lens[at] = (uint8_t)s;
                prev = s, ++at;
                continue;
            }
            int value = 0, repeat;
            if (s == 16) {
                if (prev < 0) return false;  // a repeat with nothing before it
                value = prev, repeat = 3 + (int)take(2);
            } else if (s == 17) {
                repeat = 3 + (int)take(3);
            } else {
                repeat = 11 + (int)take(7);
            }
            if (at + repeat > nlit + ndist) return false;
            if (L.lane == 0)
                for (int k = 0; k < repeat; ++k) sh.lens[at + k] = (uint8_t)value;
            prev = value, at += repeat;
        }
        L.sync();
        if (L.uniform(sh.lens[256]) == 0) return false;  // no end-of-block code: the block could not end
        return build(sh.lens, nlit, sh.lit_count, sh.lit_sym, sh.lit_fast, LIT_FAST) &&
               build(sh.lens + nlit, ndist, sh.dist_count, sh.dist_sym, sh.dist_fast, DIST_FAST);
    }
    PNG_HD void coded(int nlit, int ndist) {
        while (true) {
            refill();
            if (past_end()) { status |= W2E_PNG_STATUS_INPUT; return; }
            const int s = decode(sh.lit_count, sh.lit_sym, nlit, sh.lit_fast, LIT_FAST);
            if (past_end()) { status |= W2E_PNG_STATUS_INPUT; return; }  // (bits past the end read as 0: they are no evidence of anything else)
            if (s < 0 || s > 285) { status |= W2E_PNG_STATUS_CODE; return; }
            if (s < 256) {
                if (outpos >= expected) { status |= W2E_PNG_STATUS_LONG; return; }
                put((uint8_t)s);
            } else if (s == 256) {
                return;
            } else {
                int base, extra;
                length_base(s, base, extra);
                const int n = base + (int)take(extra);
                refill();
                const int d = decode(sh.dist_count, sh.dist_sym, ndist, sh.dist_fast, DIST_FAST);
                if (past_end()) { status |= W2E_PNG_STATUS_INPUT; return; }
                if (d < 0 || d > 29) { status |= W2E_PNG_STATUS_CODE; return; }
                distance_base(d, base, extra);
                const int dist = base + (int)take(extra);
                if (past_end()) { status |= W2E_PNG_STATUS_INPUT; return; }
                if (dist > outpos) { status |= W2E_PNG_STATUS_DISTANCE; return; }
                if (outpos + n > expected) { status |= W2E_PNG_STATUS_LONG; return; }
                copy(n, dist);
            }
            if (outpos - flushed >= FLUSH) flush_full();
        }
    }

    // The whole zlib stream: header (the host has checked it), blocks, Adler-32.  Returns the status.
    PNG_HD int run() {
        if (off < 0 || len < 0 || (off & 3) || off + len > stream_bytes) return W2E_PNG_STATUS_INPUT;
        refill();
        take(16);
        bool last = false;
        while (!last && !status) {
            refill();
            if (past_end()) { status |= W2E_PNG_STATUS_INPUT; break; }
            last = take(1) != 0;
            const int type = (int)take(2);
            if (past_end()) {
                status |= W2E_PNG_STATUS_INPUT;
            } else if (type == 0) {
                stored();
            } else if (type == 1) {
                if (!fixed_tables()) status |= W2E_PNG_STATUS_LENGTHS;
                else coded(288, 30);
            } else if (type == 2) {
                int nlit = 0, ndist = 0;
                if (!dynamic_tables(nlit, ndist)) status |= past_end() ? W2E_PNG_STATUS_INPUT : W2E_PNG_STATUS_LENGTHS;
                else coded(nlit, ndist);
            } else {
                status |= W2E_PNG_STATUS_TYPE;
            }
        }
        flush_rest();
        if (!status) {
            if (outpos < expected) status |= W2E_PNG_STATUS_SHORT;
            take(nbits & 7);
            refill();
            const uint32_t v = take(32);  // big-endian in the file
            const uint32_t want = (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
            if (past_end()) status |= W2E_PNG_STATUS_INPUT;
            else if (!status && want != ((adler_b << 16) | adler_a)) status |= W2E_PNG_STATUS_ADLER;
        }
        return status;
    }
};

}  // namespace png
}  // namespace w2e
