// K13 (optimizer): the Ranger update (mapper/training/ranger.py:78-164 -- RAdam + look-ahead + gradient centralisation) of a whole
// list of parameters as ONE launch.  As multi-tensor ops it was about ten launches per step that each re-read their lists (scale v,
// addcmul, scale m, add, sqrt, add eps, addcdiv, plus stack / mean / sub for the centralisation); here every element of p, grad,
// exp_avg and exp_avg_sq is read once and p, exp_avg, exp_avg_sq (and slow_buffer on a look-ahead step) are written once.
//
// The rectification, the step size and the look-ahead period are host control flow (ranger.py:124-161): the host passes the
// finished scalars.  A wave owns one "unit": a row (all dimensions but the first) of a tensor that is centralised -- the row's mean is
// a wave_sum, the centralised gradient lives in registers only and p.grad is never written -- or 1024 consecutive elements of a tensor
// that is not.  The tensors travel as a table in the kernel arguments (multi_tensor.h).
#include "common.h"
#include "device.h"
#include "multi_tensor.h"

namespace w2e {

constexpr int RG_REGS = 16;          // gradient elements a lane keeps: rows up to 64 * 16 = 1024 elements are read once
constexpr int RG_CHUNK = 64 * RG_REGS;

struct RangerTable : MultiTensorTable {   // 64 x 52 bytes + the two counts: 3336 of the 4 KB of kernel arguments, 44 more for the scalars
    float* slow[MT_MAXT];    // slow_buffer (look-ahead steps only)
    int row[MT_MAXT];        // row length for the centralisation, 0 = none
};

struct RangerScalars {
    float beta1, beta2, omb1, omb2, eps, neg_step, decay, alpha;   // omb = 1 - beta (rounded from the host's double, as the multi-tensor
                                                                   // ops round their scalars), neg_step = -step_size * lr, decay = 1 - weight_decay * lr
    int rectified, decayed, lookahead;
};

__global__ __launch_bounds__(256) void ranger_step_kernel(RangerTable tb, RangerScalars sc) {
    const int lane = threadIdx.x & 63;
    const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (unit >= tb.units) return;
    const int t = mt_tensor_of(tb, unit);
    const int u = unit - tb.first[t], row = tb.row[t];
    const int64_t base = row ? (int64_t)u * row : (int64_t)u * RG_CHUNK;
    const int64_t left = (int64_t)tb.n[t] - base;
    const int len = row ? row : (left < RG_CHUNK ? (int)left : RG_CHUNK);
    float* __restrict__ p = tb.p[t] + base;
    const float* __restrict__ g = tb.g[t] + base;
    float* __restrict__ m = tb.m[t] + base;
    float* __restrict__ v = tb.v[t] + base;
    float* __restrict__ slow = sc.lookahead ? tb.slow[t] + base : nullptr;

    float gr[RG_REGS];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < RG_REGS; ++j) {
        const int i = lane + 64 * j;
        gr[j] = i < len ? g[i] : 0.f;
        s += gr[j];
    }
    float mean = 0.f;
    if (row) {
        for (int i = lane + RG_CHUNK; i < len; i += 64) s += g[i];   // a longer row: summed here, read again below
        mean = wave_sum(s) / (float)row;
    }
    const auto update = [&](int i, float gc) {
        const float vv = v[i] * sc.beta2 + sc.omb2 * gc * gc;
        const float mm = m[i] * sc.beta1 + sc.omb1 * gc;
        float pp = p[i];
        if (sc.decayed) pp *= sc.decay;
        pp += sc.rectified ? sc.neg_step * (mm / (sqrtf(vv) + sc.eps)) : sc.neg_step * mm;
        if (sc.lookahead) {
            const float sl = slow[i] + sc.alpha * (pp - slow[i]);
            slow[i] = sl;
            pp = sl;
        }
        v[i] = vv, m[i] = mm, p[i] = pp;
    };
#pragma unroll
    for (int j = 0; j < RG_REGS; ++j) {
        const int i = lane + 64 * j;
        if (i < len) update(i, gr[j] - mean);
    }
    for (int i = lane + RG_CHUNK; i < len; i += 64) update(i, g[i] - mean);
}

}  // namespace w2e

using namespace w2e;

extern "C" int w2e_ranger_step(int count, float* const* p, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                               float* const* slow_buffer, const int64_t* numel, const int64_t* row_len, double beta1, double beta2, double eps,
                               double neg_step_size, int rectified, double decay, int lookahead, double alpha, void* stream) {
    W2E_REQUIRE(count >= 0 && (count == 0 || (p && grad && exp_avg && exp_avg_sq && numel && row_len)), "ranger_step: null argument");
    W2E_REQUIRE(!lookahead || count == 0 || slow_buffer, "ranger_step: a look-ahead step needs the slow buffers");
    for (int i = 0; i < count; ++i) {
        W2E_REQUIRE(numel[i] >= 0 && numel[i] <= INT32_MAX, "ranger_step: tensor %d has %lld elements (0 .. 2^31 - 1)", i, (long long)numel[i]);
        W2E_REQUIRE(numel[i] == 0 || (p[i] && grad[i] && exp_avg[i] && exp_avg_sq[i] && (!lookahead || slow_buffer[i])),
                    "ranger_step: tensor %d has a null pointer", i);
        W2E_REQUIRE(row_len[i] >= 0 && (row_len[i] == 0 || (numel[i] % row_len[i]) == 0),
                    "ranger_step: tensor %d: %lld elements are no whole number of rows of %lld", i, (long long)numel[i], (long long)row_len[i]);
    }
    RangerScalars sc{(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)neg_step_size, (float)decay,
                     (float)alpha, rectified != 0, decay != 1.0, lookahead != 0};
    const int rc = mt_for_each_table<RangerTable>(
        count, p, grad, exp_avg, exp_avg_sq, numel,
        [&](int i) { return row_len[i] ? numel[i] / row_len[i] : ceil_div(numel[i], RG_CHUNK); },
        [&](RangerTable& tb, int k, int i) { tb.slow[k] = lookahead ? slow_buffer[i] : nullptr, tb.row[k] = (int)row_len[i]; },
        [&](const RangerTable& tb) {
            ranger_step_kernel<<<(unsigned)ceil_div(tb.units, 4), 256, 0, (hipStream_t)stream>>>(tb, sc);
            W2E_LAUNCH_CHECK("ranger_step");
            return 0;
        });
    W2E_REQUIRE(rc >= 0, "ranger_step: tensor %d has too many rows", -1 - rc);
    return rc;
}
