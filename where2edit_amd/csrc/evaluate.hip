// Evaluation of the region mask against parsing labels (include/w2e_attention.h, "evaluation"): the confusion counts the IoU of
// utils.py:654-726 is made of, accumulated on the device.  The reference moves every mask to the host, builds a [N*S*S, 8] one-hot
// matrix and hands both to scikit-learn; here the only bytes that leave the GPU are the 3*T integers at the end.
//
// Shape of the pass.  A streaming reduction of B*T*S*S*4 bytes of masks (+ B*S*S label bytes, read once for all T masks).  A thread
// takes 4 consecutive pixels of one image per step: one 4-byte label load, T 16-byte mask loads, all issued before the first
// compare (8 planes in flight per thread), 3*T 32-bit counters in registers.  That needs S*S % 4 == 0, a 16-byte aligned
// mask and a 4-byte aligned label pointer (every plane then starts on a 16-byte boundary); anything else takes the one-pixel-per-
// thread form of the same loop.  At the end: wave butterfly, LDS across the 4 waves, ONE 64-bit integer atomicAdd per workgroup and
// counter.  Integer adds commute: the result does not depend on the order the workgroups arrive in.
#include "../../include/w2e_attention.h"
#include "device.h"

namespace w2e {
namespace {

constexpr int IOU_THREADS = 256;

// VEC pixels per thread and step (4: the vector form; 1: the scalar form).  TP: compile-time bound of the region loop (T <= TP).
// The per-thread counters are 32-bit: the host side keeps B*S*S <= 2^40, which with the grid of stream_grid() leaves a thread at
// most 2^21 + 4 pixels and a workgroup's sum below 2^30.
template <int TP, int VEC>
__global__ __launch_bounds__(IOU_THREADS) void mask_iou_counts_kernel(const float* __restrict__ mask, const uint8_t* __restrict__ label,
                                                                      const uint8_t* __restrict__ lut, float threshold, int T,
                                                                      int64_t npix, int64_t units, int64_t units_per_img,
                                                                      unsigned long long* __restrict__ counts) {
    __shared__ uint8_t s_lut[256];
    __shared__ unsigned s_red[IOU_THREADS / 64][3 * TP];
    s_lut[threadIdx.x] = lut[threadIdx.x];  // (IOU_THREADS == 256 == the table)
    __syncthreads();
    unsigned inter[TP], pred[TP], real[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) inter[t] = pred[t] = real[t] = 0u;

    const int64_t step = (int64_t)gridDim.x * IOU_THREADS;
    for (int64_t u = (int64_t)blockIdx.x * IOU_THREADS + threadIdx.x; u < units; u += step) {
        const int64_t b = u / units_per_img, p = (u - b * units_per_img) * VEC;
        const float* m = mask + b * T * npix + p;
        int r[VEC];
        if constexpr (VEC == 4) {
            const uchar4 l = *reinterpret_cast<const uchar4*>(label + b * npix + p);
            r[0] = s_lut[l.x], r[1] = s_lut[l.y], r[2] = s_lut[l.z], r[3] = s_lut[l.w];
        } else {
            r[0] = s_lut[label[b * npix + p]];
        }
#pragma unroll
        for (int t0 = 0; t0 < TP; t0 += 8) {  // 8 planes' loads in flight, then their compares
            float v[8][VEC];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int t = t0 + i;
                if constexpr (VEC == 4) {
                    const float4 q = t < T ? *reinterpret_cast<const float4*>(m + t * npix) : make_float4(0.f, 0.f, 0.f, 0.f);
                    v[i][0] = q.x, v[i][1] = q.y, v[i][2] = q.z, v[i][3] = q.w;
                } else {
                    v[i][0] = t < T ? m[t * npix] : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int t = t0 + i;
                if (t < T) {  // the same in every lane
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        const unsigned pr = v[i][j] >= threshold;  // false for a NaN
                        const unsigned re = r[j] == t + 1;
                        inter[t] += pr & re, pred[t] += pr, real[t] += re;
                    }
                }
            }
        }
    }

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < TP; ++t) {
        const unsigned a = wave_sum(inter[t]), b = wave_sum(pred[t]), c = wave_sum(real[t]);
        if (lane == 0) s_red[wave][3 * t] = a, s_red[wave][3 * t + 1] = b, s_red[wave][3 * t + 2] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x < 3 * T) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < IOU_THREADS / 64; ++w) s += s_red[w][threadIdx.x];
        if (s) atomicAdd(counts + threadIdx.x, s);
    }
}

}  // namespace
}  // namespace w2e

using namespace w2e;

extern "C" int w2e_mask_iou_counts(const float* mask, const uint8_t* label, const uint8_t* lut, float threshold, int batch, int classes,
                                   int size, unsigned long long* counts, void* stream) {
    W2E_REQUIRE(mask && label && lut && counts, "mask_iou_counts: null tensor");
    W2E_REQUIRE(batch >= 0 && size >= 1, "mask_iou_counts: bad dims");
    W2E_REQUIRE(classes >= 1 && classes <= 16, "mask_iou_counts: 1 <= classes <= 16 (got %d)", classes);
    W2E_REQUIRE(threshold == threshold, "mask_iou_counts: the threshold is NaN");
    W2E_REQUIRE((uintptr_t)mask % 4 == 0 && (uintptr_t)counts % 8 == 0, "mask_iou_counts: mask must be 4-byte, counts 8-byte aligned");
    const int64_t npix = (int64_t)size * size, total = (int64_t)batch * npix;
    W2E_REQUIRE(total <= (1ll << 40), "mask_iou_counts: more than 2^40 pixels in one call (32-bit per-thread counters): split the batch");
    if (total == 0) return 0;
    const bool vec = npix % 4 == 0 && (uintptr_t)mask % 16 == 0 && (uintptr_t)label % 4 == 0;
    const int64_t per_img = vec ? npix / 4 : npix, units = (int64_t)batch * per_img;
    const int grid = stream_grid(units, IOU_THREADS);
    hipStream_t s = (hipStream_t)stream;
#define IOU_GO(TP_, VEC_) \
    mask_iou_counts_kernel<TP_, VEC_><<<grid, IOU_THREADS, 0, s>>>(mask, label, lut, threshold, classes, npix, units, per_img, counts)
    if (classes <= 8) {
        if (vec) IOU_GO(8, 4);
        else IOU_GO(8, 1);
    } else {
        if (vec) IOU_GO(16, 4);
        else IOU_GO(16, 1);
    }
#undef IOU_GO
    W2E_LAUNCH_CHECK("mask_iou_counts");
    return 0;
}
