// The multi-tensor optimizer scheme (ranger.hip, adam.hip): a whole list of parameters is updated by ONE launch in which a wave
// owns one "unit" of one tensor (a chunk of consecutive elements, or a row).  The tensors travel as a table in the kernel
// arguments, MT_MAXT per launch.  Here: the table's common fields, the unit -> tensor lookup and the host loop that fills the
// tables.  An optimizer derives its table from MultiTensorTable for its extra columns and keeps its scalars and its per-element
// update.
#pragma once
#include <stdint.h>

namespace w2e {

constexpr int MT_MAXT = 64;  // tensors per launch: Ranger's 64 x 52 bytes of table (the larger) stay inside the 4 KB of kernel arguments

struct MultiTensorTable {
    float* p[MT_MAXT];
    const float* g[MT_MAXT];
    float* m[MT_MAXT];     // exp_avg
    float* v[MT_MAXT];     // exp_avg_sq
    int n[MT_MAXT];        // elements
    int first[MT_MAXT];    // index of the tensor's first unit
    int count, units;
};

// The tensor that owns `unit` (wave-uniform; unit < tb.units).
#ifdef __HIPCC__
__device__ inline int mt_tensor_of(const MultiTensorTable& tb, int unit) {
    int t = 0;
    while (t + 1 < tb.count && unit >= tb.first[t + 1]) ++t;
    return t;
}
#endif

// Walks the argument lists, fills one Table (a MultiTensorTable or a struct derived from it) per launch and hands it to
// `launch(tb)`, which returns 0 or an error code.  Empty tensors own no unit and take no table entry; a table is closed at MT_MAXT
// tensors, or before the tensor whose units would take the launch's unit count past INT32_MAX.  `units_of(i)`: the units tensor i
// needs (numel[i] > 0); `extra(tb, k, i)` fills the caller's own columns of entry k from tensor i.  Returns 0, `launch`'s error
// (positive), or -1 - i for a tensor i that alone needs more than INT32_MAX units (the caller reports it).
template <class Table, class UnitsOf, class Extra, class Launch>
int mt_for_each_table(int count, float* const* p, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                      const int64_t* numel, UnitsOf units_of, Extra extra, Launch launch) {
    int at = 0;
    while (at < count) {
        Table tb{};
        int64_t units = 0;
        for (; at < count && tb.count < MT_MAXT; ++at) {
            if (numel[at] == 0) continue;
            const int64_t mine = units_of(at);
            if (units + mine > INT32_MAX) {
                if (tb.count == 0) return -1 - at;
                break;  // the next launch takes it
            }
            const int k = tb.count++;
            tb.p[k] = p[at], tb.g[k] = grad[at], tb.m[k] = exp_avg[at], tb.v[k] = exp_avg_sq[at];
            tb.n[k] = (int)numel[at], tb.first[k] = (int)units;
            extra(tb, k, at);
            units += mine;
        }
        if (tb.count == 0) continue;
        tb.units = (int)units;
        if (const int rc = launch(tb)) return rc;
    }
    return 0;
}

}  // namespace w2e
