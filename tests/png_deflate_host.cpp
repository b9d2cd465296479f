// Stand-alone host program for csrc/png_deflate_core.h, the PNG encoder's host-and-device deflate core
// (tests/test_png_encode_host.py builds it with -fsanitize=address,undefined and runs it on a corpus file the test writes): the same
// hash, rounds, parse, code construction, header, bit writer and Adler arithmetic that the kernel of csrc/png_encode.hip compiles,
// with one lane instead of 64.  Every buffer is a heap allocation of exactly its size, so that a read or a write outside one is a
// sanitizer report.  No GPU call.
//
//   png_deflate_host CORPUS STREAMS
// The corpus: "PNGE", int32 count; per entry int64 length, the bytes.  The streams: "PNGS", int32 count; per entry int64 length, the
// zlib stream.  Before the corpus, the length builder is checked on adversarial frequency vectors for both limits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../where2edit_amd/csrc/png_deflate_core.h"

using namespace w2e;

static int failures = 0;
#define CHECK(cond, name)                                                       \
    do {                                                                        \
        if (!(cond)) {                                                          \
            printf("FAILED line %d (%s): %s\n", __LINE__, name, #cond);        \
            ++failures;                                                         \
        }                                                                       \
    } while (0)

template <typename T>
static T get(FILE* f) {
    T v;
    if (fread(&v, sizeof v, 1, f) != 1) {
        printf("png_deflate_host: the corpus ends early\n");
        exit(2);
    }
    return v;
}

// One buffer -> its zlib stream, chunk by chunk as the two launches do it.
static std::vector<uint8_t> deflate_one(const std::vector<uint8_t>& in) {
    const int64_t size = (int64_t)in.size();
    const int chunks = pngenc::chunks_of(size);
    std::vector<uint8_t> z = {pngenc::ZLIB_CMF, pngenc::ZLIB_FLG};
    uint32_t a = 1, b = 0;
    for (int c = 0; c < chunks; ++c) {
        const int64_t at = (int64_t)c * pngenc::CHUNK;
        const int n = (int)(size - at < pngenc::CHUNK ? size - at : pngenc::CHUNK);
        uint32_t* src = new uint32_t[(size_t)(n + 3) / 4 + 1];  // the words that hold the chunk, and never a zero-sized allocation
        memset(src, 0xA5, ((size_t)(n + 3) / 4 + 1) * 4);       // (what lies past byte n must not show)
        if (n) memcpy(src, in.data() + at, (size_t)n);
        uint32_t* tok = new uint32_t[(size_t)(n ? n : 1)];
        uint32_t* slot = new uint32_t[pngenc::SLOT_WORDS];
        pngenc::Shared* sh = new pngenc::Shared;
        pngenc::Deflate d(*sh, pngenc::Lanes{0, 1}, reinterpret_cast<const uint8_t*>(src), n, c == chunks - 1, tok, slot);
        const int bytes = d.run();
        CHECK(bytes >= 2 && bytes <= n + 10 && bytes <= W2E_PNG_SLOT, "slot");
        z.insert(z.end(), reinterpret_cast<uint8_t*>(slot), reinterpret_cast<uint8_t*>(slot) + bytes);
        pngenc::adler_combine(a, b, d.s1, d.s2, (uint32_t)n);
        delete sh;
        delete[] slot;
        delete[] tok;
        delete[] src;
    }
    for (int k = 3; k >= 0; --k) z.push_back((uint8_t)(((b << 16) | a) >> (8 * k)));
    CHECK((int64_t)z.size() <= size + 10 * (int64_t)chunks + 6, "stored bound");
    return z;
}

// The length builder on one frequency vector: the limit holds and the Kraft sum is exactly 1 -- apart from a lone symbol (one bit) and
// no symbol at all in an alphabet that need not be complete.
static void check_lengths(const std::vector<uint32_t>& freq, int limit, bool complete, const char* name, bool deep = false) {
    pngenc::Shared* sh = new pngenc::Shared;
    uint32_t dummy_tok, dummy_src = 0, dummy_slot;
    pngenc::Deflate d(*sh, pngenc::Lanes{0, 1}, reinterpret_cast<const uint8_t*>(&dummy_src), 0, true, &dummy_tok, &dummy_slot);
    const int nsym = (int)freq.size();
    int used = 0;
    for (int s = 0; s < nsym; ++s) sh->lit_freq[s] = freq[s], used += freq[s] != 0;
    d.build_lengths(sh->lit_freq, nsym, limit, complete, sh->lit_len);
    int64_t kraft = 0;
    int longest = 0;
    for (int s = 0; s < nsym; ++s) {
        const int len = sh->lit_len[s];
        longest = len > longest ? len : longest;
        CHECK(len <= limit, name);
        CHECK(freq[s] == 0 || len > 0, name);
        CHECK(freq[s] != 0 || len == 0 || (complete && used < 2), name);
        if (len) kraft += (int64_t)1 << (limit - len);
    }
    if (deep) CHECK(longest == limit, name);  // the unlimited code is deeper: the limit was at work
    const int64_t one = (int64_t)1 << limit;
    if (!complete && used == 0) CHECK(kraft == 0, name);
    else if (!complete && used == 1) CHECK(kraft == one / 2, name);
    else CHECK(kraft == one, name);
    if (used >= 2) {  // and it is a sensible code: a more frequent symbol never has the longer code
        for (int s = 0; s < nsym; ++s)
            for (int t = 0; t < nsym; ++t)
                if (freq[s] > freq[t] && freq[t]) CHECK(sh->lit_len[s] <= sh->lit_len[t], name);
    }
    d.make_codes(sh->lit_len, nsym, sh->lit_code);  // prefix-free by construction; the codes of one length must be distinct
    for (int s = 0; s < nsym; ++s)
        for (int t = 0; t < s; ++t)
            if (sh->lit_len[s] && sh->lit_len[s] == sh->lit_len[t]) CHECK(sh->lit_code[s] != sh->lit_code[t], name);
    delete sh;
}

static void check_builder() {
    uint32_t seed = 12345;
    auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u, seed >> 8; };
    const struct { int nsym, limit; bool complete; } alphabets[3] = {{pngenc::NLIT, 15, true}, {pngenc::NDIST, 15, false}, {pngenc::NCL, 7, true}};
    for (const auto& al : alphabets) {
        const int n = al.nsym;
        std::vector<uint32_t> f((size_t)n, 0);
        check_lengths(f, al.limit, al.complete, "no symbol");
        f[(size_t)n / 2] = 7;
        check_lengths(f, al.limit, al.complete, "single symbol");
        f.assign((size_t)n, 0), f[0] = 3;
        check_lengths(f, al.limit, al.complete, "single symbol 0");
        f[(size_t)n - 1] = 1000;
        check_lengths(f, al.limit, al.complete, "two symbols");
        f.assign((size_t)n, 1);
        check_lengths(f, al.limit, al.complete, "all equal");
        f.assign((size_t)n, 0);
        for (uint32_t k = 0, a = 1, b = 1; k < (uint32_t)(n < 40 ? n : 40); ++k) {  // Fibonacci: the deepest tree a total allows
            f[(size_t)(n - 1 - k)] = a;
            const uint32_t c = a + b;
            a = b, b = c;
        }
        check_lengths(f, al.limit, al.complete, "Fibonacci", true);  // 19, 30 or 40 numbers: 18 to 39 bits unlimited
        for (int k = 0; k < n; ++k) f[(size_t)k] = k < 30 ? 1u << k : 0;  // powers of two: a chain
        check_lengths(f, al.limit, al.complete, "powers of two", true);
        for (int trial = 0; trial < 50; ++trial) {
            for (int k = 0; k < n; ++k) {
                const uint32_t r = rnd();
                f[(size_t)k] = (r & 3) == 0 ? 0 : (r >> 2) % (1u << (1 + rnd() % 15));  // zeros, and frequencies of every magnitude
            }
            check_lengths(f, al.limit, al.complete, "random");
        }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) {
        printf("usage: png_deflate_host CORPUS STREAMS\n");
        return 2;
    }
    check_builder();
    for (int len = 3; len <= 258; ++len) {  // the symbol arithmetic against the table form of RFC 1951, 3.2.5
        int sym, extra, value;
        pngenc::length_symbol(len, sym, extra, value);
        CHECK(sym >= 257 && sym <= 285 && extra == pngenc::length_extra(sym) && value < (1 << extra), "length_symbol");
        const int base = sym < 265 ? sym - 254 : sym == 285 ? 258 : 3 + ((4 + ((sym - 261) & 3)) << extra);
        CHECK(base + value == len, "length_symbol");
    }
    for (int dist = 1; dist <= 32768; ++dist) {
        int sym, extra, value;
        pngenc::distance_symbol(dist, sym, extra, value);
        CHECK(sym >= 0 && sym <= 29 && extra == pngenc::distance_extra(sym) && value < (1 << extra), "distance_symbol");
        const int base = sym < 4 ? sym + 1 : 1 + ((2 + (sym & 1)) << extra);
        CHECK(base + value == dist, "distance_symbol");
    }
    const int want_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) CHECK(pngenc::cl_order(i) == want_order[i], "cl_order");

    FILE* f = fopen(argv[1], "rb");
    if (!f || get<char>(f) != 'P' || get<char>(f) != 'N' || get<char>(f) != 'G' || get<char>(f) != 'E') {
        printf("png_deflate_host: cannot read the corpus %s\n", argv[1]);
        return 2;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) {
        printf("png_deflate_host: cannot write %s\n", argv[2]);
        return 2;
    }
    const int32_t count = get<int32_t>(f);
    fwrite("PNGS", 1, 4, out);
    fwrite(&count, sizeof count, 1, out);
    for (int i = 0; i < count; ++i) {
        const int64_t size = get<int64_t>(f);
        std::vector<uint8_t> in((size_t)size);
        if (size && fread(in.data(), 1, (size_t)size, f) != (size_t)size) {
            printf("png_deflate_host: the corpus ends early\n");
            return 2;
        }
        const std::vector<uint8_t> z = deflate_one(in);
        const int64_t len = (int64_t)z.size();
        fwrite(&len, sizeof len, 1, out);
        fwrite(z.data(), 1, z.size(), out);
    }
    fclose(f);
    fclose(out);
    printf("png_deflate_host: %d streams\n", (int)count);
    printf(failures ? "png_deflate_host: %d check(s) failed\n" : "png_deflate_host: ok\n", failures);
    return failures != 0;
}
