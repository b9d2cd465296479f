// The PNG encoder's deflate core as host-and-device code: the hash, the rounds of the match search, the greedy parse, the
// length-limited code construction, the dynamic header, the bit writer and the Adler-32 arithmetic (include/w2e_png.h, "encoding";
// DESIGN.md "K17e").  csrc/png_encode.hip compiles it into the kernel with `lanes` = 64 (one wave per chunk);
// tests/png_deflate_host.cpp compiles the same text into a stand-alone host program with `lanes` = 1.  The round width (ROUND = 64
// positions) is part of the algorithm, not of the lane count: everything that one position of a round hands to another goes through
// `Shared` between two sync()s, so one lane that takes the 64 positions in turn computes what 64 lanes compute at once, and the host
// program's bytes are the kernel's.
//
// One chunk (at most W2E_PNG_CHUNK bytes, held in LDS) becomes one deflate block in a slot:
//   1. search, in rounds of 64 consecutive positions: a position hashes its next 4 bytes, looks at distance 1 and at the two most recent
//      positions of EARLIER rounds with that hash (a 2-way table in LDS), and keeps the longest match (at most 258 bytes, never past the
//      chunk; the nearer on a tie).  Then the round inserts its positions into the table with the result of inserting them one by one in
//      position order, whatever the lane timing: way 0 is the bucket's last position, way 1 the one before it.
//   2. parse, greedy: position -> position + max(1, length), matches below MIN_MATCH taken as literals.  The walk is the same scalar
//      sequence in every lane; the tokens go to the workspace, their symbols into the histograms in LDS.
//   3. code lengths: symbols ranked by (frequency, symbol), a two-queue Huffman merge, depths clamped to the limit and the Kraft sum
//      brought back to exactly 1 by zlib's move (a leaf from the deepest populated level above the limit's goes one level down and takes
//      a leaf of the limit's level as its sibling: the sum falls by one unit of 2^-limit per move).  Complete codes for the
//      literal/length and the code-length alphabet (a lone symbol gets a partner); the distance alphabet may hold one code of one bit
//      or none at all.
//   4. the cheapest of stored, fixed and dynamic by bit cost; the bits of a token batch are placed by a prefix sum of their lengths and
//      ORed into LDS words; the slot leaves LDS in whole words.
// Every index is bounded by construction: positions are below n <= CHUNK, hash values below HASH, symbols below the alphabet sizes,
// token indices below n, bit positions below 8 * W2E_PNG_SLOT because no block is emitted that costs more than the stored form.
#pragma once
#include <stdint.h>

#include "../../include/w2e_png.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PNGE_HD __host__ __device__ __forceinline__
#else
#define PNGE_HD inline
#endif

namespace w2e {
namespace pngenc {

constexpr int CHUNK = W2E_PNG_CHUNK;
constexpr int ROUND = 64;                      // positions of a search round
constexpr int HASH_BITS = 12, HASH = 1 << HASH_BITS;
constexpr int MIN_MATCH = 8, MAX_MATCH = 258;  // a shorter match is coded as literals: zlib's Z_FILTERED rule, taken further (the sweep)
constexpr int EMPTY = 0xFFFF;                  // no position (positions are below 32768)
constexpr int DATA_WORDS = CHUNK / 4 + 2;      // the chunk, and the word a 4-byte load at its last byte touches
constexpr int SLOT_WORDS = W2E_PNG_SLOT / 4;
constexpr int BUF_WORDS = DATA_WORDS + HASH;   // the chunk and the table (2 ways of uint16 per bucket); later the slot being built
constexpr int LITS = 288, DISTS = 32, CLS = 20;  // alphabet sizes rounded up: 286 literal/length, 30 distance, 19 code-length symbols
constexpr int NLIT = 286, NDIST = 30, NCL = 19;
constexpr uint32_t ADLER_MOD = 65521;
static_assert(BUF_WORDS >= SLOT_WORDS, "the slot is built where the chunk and the table were");

// What a workgroup keeps in LDS (on the host: one heap object).  About 57 KiB: two chunks per CU.
struct Shared {
    uint32_t buf[BUF_WORDS];
    uint32_t lit_freq[LITS], dist_freq[DISTS], cl_freq[CLS];
    uint16_t lit_code[LITS], dist_code[DISTS], cl_code[CLS];  // bit-reversed: deflate sends a code from its most significant bit
    uint8_t lit_len[LITS], dist_len[DISTS], cl_len[CLS];
    uint8_t all_len[LITS + DISTS];   // the lengths the dynamic header sends, literal/length then distance
    uint16_t cl_seq[LITS + DISTS];   // the header's code-length symbols: symbol | extra bits << 8
    // scratch of the length builder: leaves in rank order, then the merge's inner nodes
    uint32_t node_freq[2 * LITS];
    uint16_t parent[2 * LITS], depth[2 * LITS], order[LITS];
    uint32_t level[16], next[16];    // leaves per code length; the first code of each length
    // a round's results, position by position
    uint16_t rlen[ROUND], rdist[ROUND], rhash[ROUND];
    uint32_t mask[2][2];             // by round parity: the positions of the round that hold a match
    // a token batch's bits
    uint64_t tval[ROUND];
    uint16_t tbits[ROUND];
    int32_t word[4];                 // lane 0's results for the others
};

// The cooperative steps.  On the device the workgroup is ONE wave.
struct Lanes {
    int lane, lanes;
    PNGE_HD void sync() const {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
    PNGE_HD uint32_t uniform(uint32_t v) const {  // a value that is the same in every lane, said so (scalar registers from here on)
#if defined(__HIP_DEVICE_COMPILE__)
        v = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#endif
        return v;
    }
    PNGE_HD uint32_t sum(uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
#endif
        return v;
    }
    // LDS read-modify-writes of several lanes on one word; integer, so their order does not show
    PNGE_HD void add(uint32_t* p, uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(p, v);
#else
        *p += v;
#endif
    }
    PNGE_HD void bits_or(uint32_t* p, uint32_t v) const {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(p, v);
#else
        *p |= v;
#endif
    }
};

PNGE_HD uint32_t load32(const uint32_t* d, int pos) {  // the 4 bytes at byte `pos`, the first in the low byte
    const int w = pos >> 2, s = (pos & 3) * 8;
    return (uint32_t)((d[w] | ((uint64_t)d[w + 1] << 32)) >> s);
}
PNGE_HD uint32_t byte_at(const uint32_t* d, int pos) { return (d[pos >> 2] >> ((pos & 3) * 8)) & 255u; }
PNGE_HD uint32_t hash4(uint32_t v) { return (v * 0x9E3779B1u) >> (32 - HASH_BITS); }
PNGE_HD int floor_log2(uint32_t v) { return 31 - __builtin_clz(v); }
PNGE_HD uint32_t reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// RFC 1951, 3.2.5 as arithmetic, the inverse of png_core.h's length_base / distance_base: a length 3..258 and a distance 1..32768 ->
// the symbol, the number of extra bits and their value.
PNGE_HD void length_symbol(int len, int& sym, int& extra, int& value) {
    const int l = len - 3;
    if (len == MAX_MATCH) { sym = 285, extra = 0, value = 0; return; }
    if (l < 8) { sym = 257 + l, extra = 0, value = 0; return; }
    extra = floor_log2((uint32_t)l) - 2;
    sym = 261 + 4 * extra + ((l >> extra) & 3);
    value = l & ((1 << extra) - 1);
}
PNGE_HD void distance_symbol(int dist, int& sym, int& extra, int& value) {
    const int d = dist - 1;
    if (d < 4) { sym = d, extra = 0, value = 0; return; }
    const int nb = floor_log2((uint32_t)d);
    extra = nb - 1;
    sym = 2 * nb + ((d >> extra) & 1);
    value = d & ((1 << extra) - 1);
}
PNGE_HD int length_extra(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
PNGE_HD int distance_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
PNGE_HD int fixed_length(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }
// the order in which the dynamic header sends the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
PNGE_HD int cl_order(int i) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

// Adler-32 of a stream from its chunks: (a, b) after the bytes so far, a chunk's own sums s1 = sum d[i], s2 = sum (n - i) d[i] (both
// mod 65521, i from 0) and its length n.  The stream starts from a = 1, b = 0; the checksum is b << 16 | a.
PNGE_HD void adler_combine(uint32_t& a, uint32_t& b, uint32_t s1, uint32_t s2, uint32_t n) {
    b = (uint32_t)((b + (uint64_t)(n % ADLER_MOD) * a + s2) % ADLER_MOD);
    a = (a + s1) % ADLER_MOD;
}

// The token of the workspace: a literal is its byte; a match is 1 << 31 | (length - 3) << 16 | (distance - 1).
constexpr uint32_t TOKEN_MATCH = 0x80000000u;

struct Deflate {
    Shared& sh;
    const Lanes L;
    const uint8_t* src;  // the chunk's bytes (4-byte aligned; the words that hold them can be read whole)
    int n;               // 0..CHUNK
    bool last;           // the image's last chunk: its block carries BFINAL and no marker follows
    uint32_t* tok;       // n entries (at least one)
    uint32_t* slot;      // SLOT_WORDS words
    uint32_t s1, s2;     // the chunk's Adler sums
    int ntok;

    PNGE_HD Deflate(Shared& s, Lanes l, const uint8_t* src_, int n_, bool last_, uint32_t* tok_, uint32_t* slot_)
        : sh(s), L(l), src(src_), n(n_), last(last_), tok(tok_), slot(slot_), s1(0), s2(0), ntok(0) {}

    PNGE_HD uint32_t* data() { return sh.buf; }
    PNGE_HD uint16_t* head() { return reinterpret_cast<uint16_t*>(sh.buf + DATA_WORDS); }

    // -- the chunk into LDS (bytes from n on read as 0), its Adler sums, empty table and histograms --
    PNGE_HD void load() {
        const uint32_t* words = reinterpret_cast<const uint32_t*>(src);
        const int full = (n + 3) / 4;
        uint64_t a = 0, b = 0;
        for (int k = L.lane; k < DATA_WORDS; k += L.lanes) {
            uint32_t v = k < full ? words[k] : 0u;
            if (4 * k + 4 > n) v &= 4 * k >= n ? 0u : (0xFFFFFFFFu >> (8 * (4 * k + 4 - n)));
            sh.buf[k] = v;
            for (int j = 0; j < 4; ++j) {
                const uint32_t d = (v >> (8 * j)) & 255u;
                a += d, b += (uint64_t)(n - 4 * k - j) * d;  // (d is 0 from byte n on, where the factor would go negative)
            }
        }
        for (int k = L.lane; k < HASH; k += L.lanes) sh.buf[DATA_WORDS + k] = 0xFFFFFFFFu;  // EMPTY in both ways
        for (int k = L.lane; k < LITS; k += L.lanes) sh.lit_freq[k] = 0;
        for (int k = L.lane; k < DISTS; k += L.lanes) sh.dist_freq[k] = 0;
        for (int k = L.lane; k < 4; k += L.lanes) sh.mask[k >> 1][k & 1] = 0;
        s1 = L.sum((uint32_t)(a % ADLER_MOD)) % ADLER_MOD;
        s2 = L.sum((uint32_t)(b % ADLER_MOD)) % ADLER_MOD;
        L.sync();
    }

    PNGE_HD int measure(int p, int q, int limit) {  // equal bytes at p and q, at most limit (p + limit <= n)
        const uint32_t* d = data();
        int len = 0;
        while (len < limit) {
            const uint32_t x = load32(d, p + len) ^ load32(d, q + len);
            if (x) {
                len += __builtin_ctz(x) >> 3;
                break;
            }
            len += 4;
        }
        return len < limit ? len : limit;
    }

    // -- steps 1 and 2 --
    PNGE_HD void search_and_parse() {
        uint16_t* table = head();
        int carry = 0;  // the position of the next token
        for (int base = 0, round = 0; base < n; base += ROUND, ++round) {
            const int cnt = n - base < ROUND ? n - base : ROUND;
            const bool reached = carry < base + cnt;  // otherwise the whole round lies inside a match: it is only inserted
            uint32_t* mask = sh.mask[round & 1];
            for (int k = L.lane; k < ROUND; k += L.lanes) {
                const int p = base + k;
                int h = EMPTY, best = 0, dist = 0;
                if (p + 4 <= n) {
                    h = (int)hash4(load32(data(), p));
                    if (reached && p >= carry) {
                        const int limit = n - p < MAX_MATCH ? n - p : MAX_MATCH;
                        if (p >= 1) best = measure(p, p - 1, limit), dist = 1;
                        for (int way = 0; way < 2 && best < limit; ++way) {
                            const int q = table[2 * h + way];
                            if (q == EMPTY || p - q == 1) continue;
                            const int len = measure(p, q, limit);
                            if (len > best) best = len, dist = p - q;
                        }
                    }
                }
                const bool match = best >= MIN_MATCH;
                sh.rhash[k] = (uint16_t)h, sh.rlen[k] = (uint16_t)(match ? best : 0), sh.rdist[k] = (uint16_t)dist;
                if (match) L.bits_or(&mask[k >> 5], 1u << (k & 31));
            }
            L.sync();
            // insert: what one-by-one insertion in position order leaves in a bucket
            for (int k = L.lane; k < ROUND; k += L.lanes) {
                const int h = sh.rhash[k];
                if (h == EMPTY) continue;
                int later = 0, earlier = 0;
                for (int j = 0; j < ROUND; ++j) {
                    const int same = sh.rhash[j] == h;
                    later += same & (j > k), earlier |= same & (j < k);
                }
                if (later == 0) {
                    if (!earlier) table[2 * h + 1] = table[2 * h];
                    table[2 * h] = (uint16_t)(base + k);
                } else if (later == 1) {
                    table[2 * h + 1] = (uint16_t)(base + k);
                }
            }
            if (L.lane == 0) sh.mask[(round + 1) & 1][0] = sh.mask[(round + 1) & 1][1] = 0;
            if (reached) {
                // the walk: literals up to the next match by bit arithmetic, one LDS read per match
                const uint64_t matches = L.uniform(mask[0]) | ((uint64_t)L.uniform(mask[1]) << 32);
                uint64_t starts = 0;
                int p = carry - base;
                while (p < cnt) {
                    const uint64_t rest = matches >> p;
                    int stop = rest ? p + __builtin_ctzll(rest) : cnt;
                    if (stop > cnt) stop = cnt;
                    if (stop > p) starts |= (stop - p == 64 ? ~0ull : ((1ull << (stop - p)) - 1ull)) << p;
                    p = stop;
                    if (p < cnt) starts |= 1ull << p, p += (int)L.uniform(sh.rlen[p]);
                }
                carry = base + p;
                for (int k = L.lane; k < ROUND; k += L.lanes) {
                    if (!((starts >> k) & 1ull)) continue;
                    const int at = ntok + __builtin_popcountll(starts & ((1ull << k) - 1ull));
                    const int len = sh.rlen[k];
                    if (len) {
                        int ls, ds, e, v;
                        length_symbol(len, ls, e, v);
                        distance_symbol(sh.rdist[k], ds, e, v);
                        tok[at] = TOKEN_MATCH | (uint32_t)(len - 3) << 16 | (uint32_t)(sh.rdist[k] - 1);
                        L.add(&sh.lit_freq[ls], 1), L.add(&sh.dist_freq[ds], 1);
                    } else {
                        const uint32_t lit = byte_at(data(), base + k);
                        tok[at] = lit;
                        L.add(&sh.lit_freq[lit], 1);
                    }
                }
                ntok += __builtin_popcountll(starts);
            }
            L.sync();
        }
        if (L.lane == 0) sh.lit_freq[256] = 1;  // the end of the block
        L.sync();
    }

    // -- step 3: code lengths of at most `limit` bits for the first nsym symbols of freq.  `complete`: the code must be complete, so a
    //    lone symbol gets a partner (its frequency becomes 1); otherwise a lone symbol gets one bit and no symbol gives no code.
    PNGE_HD void build_lengths(uint32_t* freq, int nsym, int limit, bool complete, uint8_t* lens) {
        uint32_t used = 0;
        for (int s = L.lane; s < nsym; s += L.lanes) used += freq[s] != 0;
        used = L.sum(used);
        L.sync();
        if (complete && used < 2) {
            if (L.lane == 0) {
                if (used == 0) freq[0] = freq[1] = 1;
                else freq[freq[0] ? 1 : 0] = 1;
            }
            used = 2;
            L.sync();
        }
        for (int s = L.lane; s < nsym; s += L.lanes) lens[s] = (used == 1 && freq[s]) ? 1 : 0;
        if (used < 2) {
            L.sync();
            return;
        }
        const int leaves = (int)used;
        for (int s = L.lane; s < nsym; s += L.lanes) {  // rank by (frequency, symbol)
            const uint32_t f = freq[s];
            if (!f) continue;
            int rank = 0;
            for (int j = 0; j < nsym; ++j) {
                const uint32_t g = freq[j];
                rank += (g != 0) & ((g < f) | ((g == f) & (j < s)));
            }
            sh.order[rank] = (uint16_t)s, sh.node_freq[rank] = f;
        }
        for (int k = L.lane; k < 16; k += L.lanes) sh.level[k] = 0;
        L.sync();
        if (L.lane == 0) {
            // the two-queue merge: leaves in rank order, inner nodes in the order they are made (their frequencies never fall)
            int i = 0, j = leaves, made = leaves;
            while (made < 2 * leaves - 1) {
                int pick[2];
                for (int t = 0; t < 2; ++t) pick[t] = (i < leaves && (j >= made || sh.node_freq[i] <= sh.node_freq[j])) ? i++ : j++;
                sh.node_freq[made] = sh.node_freq[pick[0]] + sh.node_freq[pick[1]];
                sh.parent[pick[0]] = sh.parent[pick[1]] = (uint16_t)made;
                ++made;
            }
            sh.depth[2 * leaves - 2] = 0;
            for (int k = 2 * leaves - 3; k >= 0; --k) sh.depth[k] = (uint16_t)(sh.depth[sh.parent[k]] + 1);  // (a parent is made after its children)
            int64_t kraft = 0;  // in units of 2^-limit
            for (int k = 0; k < leaves; ++k) {
                const int d = sh.depth[k] < limit ? sh.depth[k] : limit;
                sh.level[d] += 1, kraft += (int64_t)1 << (limit - d);
            }
            for (int64_t over = kraft - ((int64_t)1 << limit); over > 0; --over) {
                int bits = limit - 1;
                while (bits > 0 && sh.level[bits] == 0) --bits;
                sh.level[bits] -= 1, sh.level[bits + 1] += 2, sh.level[limit] -= 1;
            }
            int k = 0;  // the longest codes to the rarest symbols
            for (int bits = limit; bits >= 1; --bits)
                for (uint32_t c = sh.level[bits]; c > 0 && k < leaves; --c) lens[sh.order[k++]] = (uint8_t)bits;
        }
        L.sync();
    }

    // canonical codes (RFC 1951, 3.2.2), bit-reversed
    PNGE_HD void make_codes(const uint8_t* lens, int nsym, uint16_t* codes) {
        for (int k = L.lane; k < 16; k += L.lanes) sh.level[k] = 0;
        L.sync();
        for (int s = L.lane; s < nsym; s += L.lanes)
            if (lens[s]) L.add(&sh.level[lens[s]], 1);
        L.sync();
        if (L.lane == 0) {
            uint32_t code = 0;
            sh.next[0] = 0;
            for (int bits = 1; bits < 16; ++bits) code = (code + sh.level[bits - 1]) << 1, sh.next[bits] = code;
        }
        L.sync();
        for (int s = L.lane; s < nsym; s += L.lanes) {
            const int len = lens[s];
            uint32_t before = 0;
            for (int j = 0; j < s && len; ++j) before += lens[j] == len;
            codes[s] = len ? (uint16_t)reverse_bits(sh.next[len] + before, len) : 0;
        }
        L.sync();
    }

    // The dynamic header's code-length symbols for the lengths in use: sh.cl_seq, sh.cl_freq; returns their number, and HLIT / HDIST
    // as the numbers of lengths sent.
    PNGE_HD int header_symbols(int& hlit, int& hdist) {
        for (int k = L.lane; k < CLS; k += L.lanes) sh.cl_freq[k] = 0;
        L.sync();
        if (L.lane == 0) {
            int nl = NLIT, nd = NDIST;
            while (nl > 257 && sh.lit_len[nl - 1] == 0) --nl;
            while (nd > 1 && sh.dist_len[nd - 1] == 0) --nd;
            for (int k = 0; k < nl; ++k) sh.all_len[k] = sh.lit_len[k];
            for (int k = 0; k < nd; ++k) sh.all_len[nl + k] = sh.dist_len[k];
            const int total = nl + nd;
            int count = 0;
            auto put = [&](int sym, int extra) { sh.cl_seq[count++] = (uint16_t)(sym | extra << 8), sh.cl_freq[sym] += 1; };
            for (int i = 0; i < total;) {
                const int v = sh.all_len[i];
                int run = 1;
                while (i + run < total && sh.all_len[i + run] == v) ++run;
                i += run;
                if (v == 0) {
                    while (run >= 11) {
                        const int t = run < 138 ? run : 138;
                        put(18, t - 11), run -= t;
                    }
                    if (run >= 3) put(17, run - 3), run = 0;
                    while (run-- > 0) put(0, 0);
                } else {
                    put(v, 0), --run;
                    while (run >= 3) {
                        const int t = run < 6 ? run : 6;
                        put(16, t - 3), run -= t;
                    }
                    while (run-- > 0) put(v, 0);
                }
            }
            sh.word[0] = nl, sh.word[1] = nd, sh.word[2] = count;
        }
        L.sync();
        hlit = sh.word[0], hdist = sh.word[1];
        return sh.word[2];
    }

    // -- the bit writer: `count` bits of v at bit `at` of the slot being built (LSB first, as deflate packs them) --
    PNGE_HD void put_bits(int64_t at, uint64_t v, int count) {
        if (!count) return;
        const int w = (int)(at >> 5), s = (int)(at & 31);
        const uint32_t lo = (uint32_t)(v << s);
        const uint64_t rest = s ? v >> (32 - s) : v >> 32;
        if (lo) L.bits_or(&sh.buf[w], lo);
        if ((uint32_t)rest) L.bits_or(&sh.buf[w + 1], (uint32_t)rest);
        if (rest >> 32) L.bits_or(&sh.buf[w + 2], (uint32_t)(rest >> 32));
    }

    PNGE_HD void token_bits(uint32_t t, uint64_t& v, int& count) {
        if (!(t & TOKEN_MATCH)) {
            v = sh.lit_code[t], count = sh.lit_len[t];
            return;
        }
        int ls, le, lv, ds, de, dv;
        length_symbol((int)((t >> 16) & 255u) + 3, ls, le, lv);
        distance_symbol((int)(t & 0x7FFFu) + 1, ds, de, dv);
        v = sh.lit_code[ls], count = sh.lit_len[ls];
        v |= (uint64_t)lv << count, count += le;
        v |= (uint64_t)sh.dist_code[ds] << count, count += sh.dist_len[ds];
        v |= (uint64_t)dv << count, count += de;
    }

    // The stored form, and every slot's tail: byte i of the slot.
    PNGE_HD uint32_t stored_byte(int i) {
        const uint32_t len = (uint32_t)n, nlen = len ^ 0xFFFFu;  // LEN and its complement, low byte first
        if (i < 5) return i == 0 ? (last ? 1u : 0u) : i == 1 ? (len & 255u) : i == 2 ? (len >> 8) : i == 3 ? (nlen & 255u) : (nlen >> 8);
        if (i < 5 + n) return byte_at(data(), i - 5);
        return (!last && i >= 5 + n + 3 && i < 5 + n + 5) ? 255u : 0u;  // the marker: 00 00 00 FF FF
    }

    // -- the whole chunk: returns the bytes of the slot --
    PNGE_HD int run() {
        load();
        search_and_parse();
        build_lengths(sh.lit_freq, NLIT, 15, true, sh.lit_len);
        build_lengths(sh.dist_freq, NDIST, 15, false, sh.dist_len);
        int hlit, hdist;
        const int ncl = header_symbols(hlit, hdist);
        build_lengths(sh.cl_freq, NCL, 7, true, sh.cl_len);
        int hclen = NCL;
        while (hclen > 4 && sh.cl_len[cl_order(hclen - 1)] == 0) --hclen;
        // the three costs in bits, block header included
        uint32_t dynamic = 0, fixed = 0;
        for (int s = L.lane; s < NLIT; s += L.lanes) {
            const uint32_t f = s == 256 ? 1u : sh.lit_freq[s], e = s > 256 ? (uint32_t)length_extra(s) : 0u;
            dynamic += f * (sh.lit_len[s] + e), fixed += f * ((uint32_t)fixed_length(s) + e);
        }
        for (int s = L.lane; s < NDIST; s += L.lanes) {
            const uint32_t f = sh.dist_freq[s], e = (uint32_t)distance_extra(s);
            dynamic += f * (sh.dist_len[s] + e), fixed += f * (5u + e);
        }
        for (int k = L.lane; k < ncl; k += L.lanes) {
            const int sym = sh.cl_seq[k] & 255;
            dynamic += sh.cl_len[sym] + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
        }
        dynamic = L.sum(dynamic) + 3 + 14 + 3 * (uint32_t)hclen;
        fixed = L.sum(fixed) + 3;
        const uint32_t stored = 8u * (uint32_t)(n + 5);
        const int form = (stored <= fixed && stored <= dynamic) ? 0 : (fixed <= dynamic ? 1 : 2);
        int bytes;
        if (form == 0) {
            bytes = n + 5 + (last ? 0 : 5);
            L.sync();
            for (int w = L.lane; 4 * w < bytes; w += L.lanes) {
                uint32_t v = 0;
                for (int j = 0; j < 4; ++j) v |= stored_byte(4 * w + j) << (8 * j);
                slot[w] = v;
            }
            return bytes;
        }
        if (form == 1) {
            for (int s = L.lane; s < LITS; s += L.lanes) sh.lit_len[s] = (uint8_t)fixed_length(s);
            for (int s = L.lane; s < DISTS; s += L.lanes) sh.dist_len[s] = 5;
            L.sync();
            make_codes(sh.lit_len, LITS, sh.lit_code);
            make_codes(sh.dist_len, DISTS, sh.dist_code);
        } else {
            make_codes(sh.lit_len, NLIT, sh.lit_code);
            make_codes(sh.dist_len, NDIST, sh.dist_code);
            make_codes(sh.cl_len, NCL, sh.cl_code);
        }
        for (int w = L.lane; w < SLOT_WORDS; w += L.lanes) sh.buf[w] = 0;  // (the chunk and the table are no longer needed)
        L.sync();
        if (L.lane == 0) {
            int64_t at = 0;
            put_bits(at, (last ? 1u : 0u) | (uint32_t)form << 1, 3), at += 3;
            if (form == 2) {
                put_bits(at, (uint64_t)(hlit - 257) | (uint64_t)(hdist - 1) << 5 | (uint64_t)(hclen - 4) << 10, 14), at += 14;
                for (int i = 0; i < hclen; ++i) put_bits(at, sh.cl_len[cl_order(i)], 3), at += 3;
                for (int k = 0; k < ncl; ++k) {
                    const int sym = sh.cl_seq[k] & 255, extra = sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0;
                    put_bits(at, sh.cl_code[sym] | (uint64_t)(sh.cl_seq[k] >> 8) << sh.cl_len[sym], sh.cl_len[sym] + extra);
                    at += sh.cl_len[sym] + extra;
                }
            }
            sh.word[3] = (int32_t)at;
        }
        L.sync();
        int64_t at = sh.word[3];
        for (int t0 = 0; t0 <= ntok; t0 += ROUND) {  // (token ntok is the end of the block)
            for (int k = L.lane; k < ROUND; k += L.lanes) {
                const int t = t0 + k;
                uint64_t v = 0;
                int count = 0;
                if (t < ntok) token_bits(tok[t], v, count);
                else if (t == ntok) v = sh.lit_code[256], count = sh.lit_len[256];
                sh.tval[k] = v, sh.tbits[k] = (uint16_t)count;
            }
            L.sync();
            int total = 0;
            for (int k = L.lane; k < ROUND; k += L.lanes) {
                int before = 0;
                total = 0;
                for (int j = 0; j < ROUND; ++j) before += j < k ? sh.tbits[j] : 0, total += sh.tbits[j];
                put_bits(at + before, sh.tval[k], sh.tbits[k]);
            }
            at += (int64_t)L.uniform((uint32_t)total);
            L.sync();
        }
        if (!last) {
            at = (at + 3 + 7) / 8 * 8;  // the empty stored block: three zero bits, the rest of the byte, 00 00 FF FF
            if (L.lane == 0) put_bits(at + 16, 0xFFFFu, 16);
            at += 32;
        }
        bytes = (int)((at + 7) / 8);
        if (bytes > W2E_PNG_SLOT) bytes = W2E_PNG_SLOT;  // (never: the block costs less than the stored form; a slot is a slot regardless)
        L.sync();
        for (int w = L.lane; 4 * w < bytes; w += L.lanes) slot[w] = sh.buf[w];
        return bytes;
    }
};

// The two bytes before the blocks: a 32 KiB window, the default level, FCHECK making the pair a multiple of 31.
constexpr uint8_t ZLIB_CMF = 0x78, ZLIB_FLG = 0x9C;
static_assert((ZLIB_CMF * 256 + ZLIB_FLG) % 31 == 0, "FCHECK");

PNGE_HD int chunks_of(int64_t size) { return size <= CHUNK ? 1 : (int)((size + CHUNK - 1) / CHUNK); }

}  // namespace pngenc
}  // namespace w2e
