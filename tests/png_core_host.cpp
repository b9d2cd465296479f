// Stand-alone host program for csrc/png_core.h, the PNG decoder's host-and-device core (tests/test_png_host.py builds it with
// -fsanitize=address,undefined and runs it on a corpus file the test writes): the same bit reader, table construction, symbol decode,
// bounds logic, Adler-32 and filters that the kernels of csrc/png.hip compile, with one lane instead of 64.  Every buffer is a heap
// allocation of exactly its size, so that a read or a write outside one is a sanitizer report.  No GPU call.
//
// The corpus: "PNGC", int32 count; per entry int32 name length, the name, int64 stream length, the stream, int64 expected size, int32
// wanted status (-1: any nonzero), int64 length of the wanted output (0: not checked) and the output; then int32 h, int32 row bytes
// (without the filter byte), int32 bpp (h = 0: no filter step), int32 wanted filter status, int64 length of the wanted rows, the rows.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../where2edit_amd/csrc/png_core.h"

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
        printf("png_core_host: the corpus ends early\n");
        exit(2);
    }
    return v;
}
static std::vector<uint8_t> get_bytes(FILE* f, int64_t n) {
    std::vector<uint8_t> v((size_t)n);
    if (n && fread(v.data(), 1, (size_t)n, f) != (size_t)n) {
        printf("png_core_host: the corpus ends early\n");
        exit(2);
    }
    return v;
}

// One stream, placed at byte `lead` (a multiple of 4) of a buffer that ends with the stream's last word.
static int inflate_one(const std::vector<uint8_t>& z, int64_t lead, int64_t expected, std::vector<uint8_t>& out) {
    const int64_t total = (lead + (int64_t)z.size() + 3) / 4 * 4;
    uint32_t* words = new uint32_t[(size_t)(total / 4) + 1]();  // (+1: never a zero-sized allocation)
    memcpy(reinterpret_cast<uint8_t*>(words) + lead, z.data(), z.size());
    const int64_t pitch = (expected + 3) / 4 * 4;
    uint32_t* raw = new uint32_t[(size_t)(pitch / 4) + 1]();
    png::Shared* sh = new png::Shared();
    png::Inflate inf(*sh, png::Lanes{0, 1}, reinterpret_cast<const uint8_t*>(words), total, lead, (int64_t)z.size(), reinterpret_cast<uint8_t*>(raw), expected);
    const int status = inf.run();
    out.assign(reinterpret_cast<uint8_t*>(raw), reinterpret_cast<uint8_t*>(raw) + expected);
    delete sh;
    delete[] raw;
    delete[] words;
    return status;
}

// The filter step as the kernel's lanes do it, one row after the other.
static int unfilter_rows(std::vector<uint8_t>& data, int h, int row_bytes, int bpp, std::vector<uint8_t>& rows) {
    int status = 0;
    rows.assign((size_t)h * row_bytes, 0);
    for (int y = 0; y < h; ++y) {
        int filter = data[(size_t)y * (row_bytes + 1)];
        if (filter > 4) filter = 0, status |= W2E_PNG_STATUS_FILTER;
        for (int x = 0; x < row_bytes; ++x) {
            const int a = x >= bpp ? rows[(size_t)y * row_bytes + x - bpp] : 0, b = y ? rows[(size_t)(y - 1) * row_bytes + x] : 0;
            const int c = (x >= bpp && y) ? rows[(size_t)(y - 1) * row_bytes + x - bpp] : 0;
            rows[(size_t)y * row_bytes + x] = png::unfilter(filter, data[(size_t)y * (row_bytes + 1) + 1 + x], a, b, c);
        }
    }
    return status;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: png_core_host CORPUS\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f || get<char>(f) != 'P' || get<char>(f) != 'N' || get<char>(f) != 'G' || get<char>(f) != 'C') {
        printf("png_core_host: cannot read the corpus %s\n", argv[1]);
        return 2;
    }
    const int count = get<int32_t>(f);
    int valid = 0, corrupt = 0;
    for (int i = 0; i < count; ++i) {
        const int name_len = get<int32_t>(f);
        const std::vector<uint8_t> name_bytes = get_bytes(f, name_len);
        const std::string name_s(name_bytes.begin(), name_bytes.end());
        const char* name = name_s.c_str();
        const std::vector<uint8_t> z = get_bytes(f, get<int64_t>(f));
        const int64_t expected = get<int64_t>(f);
        const int want = get<int32_t>(f);
        const std::vector<uint8_t> want_out = get_bytes(f, get<int64_t>(f));
        const int h = get<int32_t>(f), row_bytes = get<int32_t>(f), bpp = get<int32_t>(f), want_filter = get<int32_t>(f);
        const std::vector<uint8_t> want_rows = get_bytes(f, get<int64_t>(f));
        std::vector<uint8_t> out;
        for (int64_t lead = 0; lead <= 8; lead += 4) {  // alone in its buffer, and behind other bytes
            const int status = inflate_one(z, lead, expected, out);
            if (want < 0) CHECK(status != 0, name);
            else CHECK(status == want, name);
            if (status != want && want >= 0) printf("  %s: status %d, wanted %d\n", name, status, want);
            if (!want_out.empty()) CHECK(out == want_out, name);
        }
        if (h) {
            std::vector<uint8_t> rows;
            CHECK((int64_t)out.size() == (int64_t)h * (row_bytes + 1), name);
            CHECK(unfilter_rows(out, h, row_bytes, bpp, rows) == want_filter, name);
            if (!want_rows.empty()) CHECK(rows == want_rows, name);
        }
        want == 0 ? ++valid : ++corrupt;
    }
    fclose(f);
    {  // the arithmetic forms of the length and distance tables against RFC 1951, 3.2.5
        const int lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
        const int dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        for (int s = 0; s < 29; ++s) {
            int base, extra;
            png::length_base(257 + s, base, extra);
            CHECK(base == lbase[s] && extra == ((s < 8 || s == 28) ? 0 : (s - 4) / 4), "length_base");
        }
        for (int s = 0; s < 30; ++s) {
            int base, extra;
            png::distance_base(s, base, extra);
            CHECK(base == dbase[s] && extra == (s < 4 ? 0 : s / 2 - 1), "distance_base");
        }
    }
    printf("png_core_host: %d valid and %d corrupt streams\n", valid, corrupt);
    printf(failures ? "png_core_host: %d check(s) failed\n" : "png_core_host: ok\n", failures);
    return failures != 0;
}
