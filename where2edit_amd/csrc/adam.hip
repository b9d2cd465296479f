// K13b (optimizer): torch.optim.Adam's update (no amsgrad, no maximize) of a whole list of parameters as ONE launch -- the optimizer of
// the region-attention loop (attention/run_attention.py:1051, :1419).  As multi-tensor ops it is a dozen passes that each re-read
// their lists of about 110 tensors; here every element of p, grad, exp_avg and exp_avg_sq is read once and p, exp_avg, exp_avg_sq
// are written once.  The bias corrections and the step size are host arithmetic: the host passes the finished scalars.  A wave owns
// 1024 consecutive elements of one tensor; the tensors travel as a table in the kernel arguments (multi_tensor.h).
#include "common.h"
#include "device.h"
#include "multi_tensor.h"

namespace w2e {

constexpr int AD_CHUNK = 1024;  // elements per wave

struct AdamTable : MultiTensorTable {};  // no extra column: 64 x 40 bytes + the two counts of the 4 KB of kernel arguments

struct AdamScalars {
    float beta1, beta2, omb1, omb2, eps, step_size, bc2_sqrt, weight_decay;  // omb = 1 - beta, rounded from the host's double
};

__global__ __launch_bounds__(256) void adam_step_kernel(AdamTable tb, AdamScalars sc) {
    const int lane = threadIdx.x & 63;
    const int unit = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (unit >= tb.units) return;
    const int t = mt_tensor_of(tb, unit);
    const int64_t base = (int64_t)(unit - tb.first[t]) * AD_CHUNK;
    const int64_t left = (int64_t)tb.n[t] - base;
    const int len = left < AD_CHUNK ? (int)left : AD_CHUNK;
    float* __restrict__ p = tb.p[t] + base;
    const float* __restrict__ g = tb.g[t] + base;
    float* __restrict__ m = tb.m[t] + base;
    float* __restrict__ v = tb.v[t] + base;
#pragma unroll 4
    for (int i = lane; i < len; i += 64) {
        float pp = p[i], gg = g[i];
        if (sc.weight_decay != 0.f) gg += sc.weight_decay * pp;
        const float mm = sc.beta1 * m[i] + sc.omb1 * gg;
        const float vv = sc.beta2 * v[i] + sc.omb2 * gg * gg;
        pp -= sc.step_size * (mm / (sqrtf(vv) / sc.bc2_sqrt + sc.eps));
        m[i] = mm, v[i] = vv, p[i] = pp;
    }
}

}  // namespace w2e

using namespace w2e;

extern "C" int w2e_adam_step(int count, float* const* p, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                             const int64_t* numel, double beta1, double beta2, double eps, double step_size, double bias_correction2_sqrt,
                             double weight_decay, void* stream) {
    W2E_REQUIRE(count >= 0 && (count == 0 || (p && grad && exp_avg && exp_avg_sq && numel)), "adam_step: null argument");
    W2E_REQUIRE(bias_correction2_sqrt > 0.0, "adam_step: bias_correction2_sqrt must be positive");
    for (int i = 0; i < count; ++i) {
        W2E_REQUIRE(numel[i] >= 0 && numel[i] <= INT32_MAX, "adam_step: tensor %d has %lld elements (0 .. 2^31 - 1)", i, (long long)numel[i]);
        W2E_REQUIRE(numel[i] == 0 || (p[i] && grad[i] && exp_avg[i] && exp_avg_sq[i]), "adam_step: tensor %d has a null pointer", i);
    }
    const AdamScalars sc{(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, (float)step_size,
                         (float)bias_correction2_sqrt, (float)weight_decay};
    const int rc = mt_for_each_table<AdamTable>(
        count, p, grad, exp_avg, exp_avg_sq, numel, [&](int i) { return ceil_div(numel[i], AD_CHUNK); }, [](AdamTable&, int, int) {},
        [&](const AdamTable& tb) {
            adam_step_kernel<<<(unsigned)ceil_div(tb.units, 4), 256, 0, (hipStream_t)stream>>>(tb, sc);
            W2E_LAUNCH_CHECK("adam_step");
            return 0;
        });
    W2E_REQUIRE(rc >= 0, "adam_step: tensor %d has too many elements for one launch", -1 - rc);
    return rc;
}
