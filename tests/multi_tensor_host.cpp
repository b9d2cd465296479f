// Stand-alone host program for csrc/multi_tensor.h's table-filling loop (tests/test_multi_tensor_host.py builds it with
// -fsanitize=address,undefined and runs it): every non-empty tensor lands in exactly one table, in order, at most MT_MAXT per
// table, with the unit offsets the kernels' lookup expects, and a table is closed before its unit count would pass INT32_MAX.
// No GPU call: `launch` records the tables.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../where2edit_amd/csrc/multi_tensor.h"

using namespace w2e;

struct Table : MultiTensorTable {
    int tag[MT_MAXT];  // an extra column, as RangerTable has
};

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED line %d: %s\n", __LINE__, #cond);         \
            ++failures;                                              \
        }                                                            \
    } while (0)

// `numel[i]` elements and `units[i]` units per tensor; returns the number of launches, -1000 + i for a tensor i that fits no launch, or
// `launch`'s error code negated.
static int run(const std::vector<int64_t>& numel, const std::vector<int64_t>& units, int fail_launch = -1) {
    const int count = (int)numel.size();
    std::vector<float> pool(count + 1);
    std::vector<float*> p(count), m(count), v(count);
    std::vector<const float*> g(count);
    for (int i = 0; i < count; ++i) p[i] = m[i] = v[i] = pool.data() + i, g[i] = pool.data() + i;
    std::vector<int> seen;
    int launches = 0;
    const int rc = mt_for_each_table<Table>(
        count, p.data(), g.data(), m.data(), v.data(), numel.data(), [&](int i) { return units[i]; },
        [&](Table& tb, int k, int i) { tb.tag[k] = i; },
        [&](const Table& tb) {
            if (launches == fail_launch) return 7;
            ++launches;
            CHECK(tb.count >= 1 && tb.count <= MT_MAXT);
            int64_t at = 0;
            for (int k = 0; k < tb.count; ++k) {
                const int i = (int)(tb.p[k] - pool.data());
                CHECK(i >= 0 && i < count && tb.tag[k] == i && tb.g[k] == g[i] && tb.m[k] == m[i] && tb.v[k] == v[i]);
                CHECK(numel[i] > 0 && tb.n[k] == numel[i] && tb.first[k] == at);
                at += units[i];
                seen.push_back(i);
            }
            CHECK(at <= INT32_MAX && tb.units == at);
            for (int k = tb.count; k < MT_MAXT; ++k) CHECK(tb.p[k] == nullptr && tb.n[k] == 0);
            return 0;
        });
    if (rc) return rc < 0 ? -1000 + (-1 - rc) : -rc;
    std::vector<int> want;
    for (int i = 0; i < count; ++i)
        if (numel[i]) want.push_back(i);
    CHECK(seen == want);
    return launches;
}

int main() {
    const int counts[] = {0, 1, 64, 65, 200};
    for (int c : counts) {
        std::vector<int64_t> numel(c), units(c);
        for (int i = 0; i < c; ++i) numel[i] = 1 + 37 * i, units[i] = (numel[i] + 1023) / 1024;
        CHECK(run(numel, units) == (c + MT_MAXT - 1) / MT_MAXT);
        for (int i = 0; i < c; i += 3) numel[i] = 0;  // empty tensors interleaved: they take no table entry
        const int live = c - (c + 2) / 3;
        CHECK(run(numel, units) == (live + MT_MAXT - 1) / MT_MAXT);
        std::vector<int64_t> none(c, 0);
        CHECK(run(none, units) == 0);
    }
    {  // rows of one element: 2^30 units each, so two of them do not fit one launch
        const int64_t big = (int64_t)1 << 30;
        CHECK(run({big, 0, big, big, 5, 0, big}, {big, 0, big, big, 1, 0, big}) == 4);
        CHECK(run({INT32_MAX, 1}, {INT32_MAX, 1}) == 2);
        CHECK(run({INT32_MAX - 1, 1}, {INT32_MAX - 1, 1}) == 1);
        CHECK(run({5, big}, {1, (int64_t)INT32_MAX + 1}) == -999);  // a tensor that fits no launch, after the table before it
        CHECK(run({big}, {(int64_t)INT32_MAX + 1}) == -1000);
    }
    CHECK(run(std::vector<int64_t>(130, 8), std::vector<int64_t>(130, 1), 1) == -7);  // a failed launch ends the loop with its code
    printf(failures ? "multi_tensor_host: %d check(s) failed\n" : "multi_tensor_host: ok\n", failures);
    return failures != 0;
}
