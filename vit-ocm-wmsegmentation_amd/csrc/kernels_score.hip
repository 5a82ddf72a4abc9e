// kernels_score.hip — the numbers eval.py's validate loop reports for a mask (eval.py:204-221): calculate_metrics
// (utils.py:388-408: sklearn's jaccard, f1, recall, precision and accuracy of the 0/1 classes value > 0.5), the ROC-AUC of a 0/1
// score that PGT.py / finetune.py add, and the per-image sigmoid Dice loss (utils.py:410-424), for a batch of images in one pass
// over the prediction (uint8 mask taken as v / 255, or fp32) and the fp32 target.
//   score_partial_kernel  grid (groups, batch). An image's `count` elements are cut into spans (a function of the count alone,
//                         every span a multiple of 16 elements); workgroup g of image b counts tp, fp and fn and sums p t, p and t
//                         (p = sigmoid(value), fp32 sigmoid_parts; the sums in float64) over span g and writes one ScorePart.
//   score_finish_kernel   grid (batch), one wave: adds the image's partials and writes counts[b] = {tp, fp, fn, tn} and
//                         scores[b] = {jaccard, f1, recall, precision, accuracy, auc, dice_loss} in float64.
// Fixed order everywhere and no atomics: per thread in index order (32-bit counters, widened to 64 bits before anything is added
// across threads), the wave by the xor butterfly, the four waves in wave order, the partials by lane (g = l, l + 64, ...) and the
// same butterfly. Equal inputs give equal bits.
// Images start at b * count elements, so an odd count leaves later images unaligned. Each workgroup looks at its own image's
// addresses: 16-byte loads where they are 16-byte aligned (16 mask bytes, 4 floats), element loads otherwise. Both ways give a
// thread the same elements in the same order, so an image scores to the same bits wherever it starts.
#include <cmath>

#include "common.h"
#include "host_common.h"

#define fail ocm_fail

// the scores are IEEE float64 quotients of integers, as sklearn computes them: separate operations
#pragma clang fp contract(off)

namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_SPAN = 4096;     // elements per workgroup until the cap is reached
constexpr int SC_MAX_GROUPS = 256;  // workgroups (= partials) per image
constexpr size_t SC_MAX_COUNT = (size_t)1 << 36;  // at most 2^36 / (256 * 256) + 16 elements per thread: 32-bit counters do

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct alignas(16) ScorePart {
    double pt, p, t;            // sum p t, sum p, sum t
    unsigned long long tp, fp, fn;
};

struct ScoreAcc {
    double pt = 0.0, p = 0.0, t = 0.0;
    uint32_t tp = 0, fp = 0, fn = 0;
};

// value > 0.5f and target > 0.5f: a NaN compares false (class 0)
__device__ __forceinline__ void tally(ScoreAcc &a, float p, bool pc, float t) {
    const bool tc = t > 0.5f;
    a.tp += pc && tc;
    a.fp += pc && !tc;
    a.fn += !pc && tc;
    a.pt += (double)p * (double)t;
    a.p += (double)p;
    a.t += (double)t;
}

__device__ __forceinline__ f32x4 load4(const float *p, bool vec) {
    if (vec) return *(const f32x4 *)p;
    f32x4 v;
    v[0] = p[0], v[1] = p[1], v[2] = p[2], v[3] = p[3];
    return v;
}

__device__ __forceinline__ u32x4 load16(const uint8_t *p, bool vec) {
    if (vec) return *(const u32x4 *)p;
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        v[j] = (uint32_t)p[4 * j] | (uint32_t)p[4 * j + 1] << 8 | (uint32_t)p[4 * j + 2] << 16 | (uint32_t)p[4 * j + 3] << 24;
    return v;
}

__device__ __forceinline__ ScorePart wave_sum(ScorePart v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v.pt += __shfl_xor(v.pt, o, 64);
        v.p += __shfl_xor(v.p, o, 64);
        v.t += __shfl_xor(v.t, o, 64);
        v.tp += __shfl_xor(v.tp, o, 64);
        v.fp += __shfl_xor(v.fp, o, 64);
        v.fn += __shfl_xor(v.fn, o, 64);
    }
    return v;
}

struct ScorePlan {
    size_t span;
    int groups;
};

int score_max_groups(size_t count) { return (int)std::min<size_t>((count + SC_SPAN - 1) / SC_SPAN, SC_MAX_GROUPS); }

// groups <= score_max_groups(count): the span is at least count / that
ScorePlan score_plan(size_t count) {
    const size_t g0 = score_max_groups(count);
    ScorePlan p;
    p.span = ((count + g0 - 1) / g0 + 15) / 16 * 16;
    p.groups = (int)((count + p.span - 1) / p.span);
    return p;
}

// U8: pred is a uint8 mask with the value v / 255.0f (eval.py's output / 255). A byte has 256 values: their sigmoids come
// from a table in LDS, and v / 255.0f > 0.5f exactly when v >= 128 (127 / 255 = 0.498, 128 / 255 = 0.502).
template <bool U8>
__global__ __launch_bounds__(SC_THREADS) void score_partial_kernel(const void *__restrict__ pred, const float *__restrict__ target,
                                                                   ScorePart *__restrict__ part, size_t count, size_t span) {
    __shared__ float s_sig[U8 ? 256 : 1];
    __shared__ ScorePart s_wave[SC_THREADS / 64];
    const size_t begin = (size_t)blockIdx.x * span, end = std::min<size_t>(count, begin + span), n = end - begin;
    const size_t first = (size_t)blockIdx.y * count + begin;
    const float *ts = target + first;
    const bool tvec = ((uintptr_t)ts & 15) == 0;
    ScoreAcc acc;
    if constexpr (U8) {
        float p, pq;
        sigmoid_parts((float)threadIdx.x / 255.0f, p, pq);
        s_sig[threadIdx.x] = p;
        __syncthreads();
        const uint8_t *ps = (const uint8_t *)pred + first;
        const bool pvec = ((uintptr_t)ps & 15) == 0;
        const size_t nc = n / 16;
        for (size_t i = threadIdx.x; i < nc; i += SC_THREADS) {
            const u32x4 pv = load16(ps + 16 * i, pvec);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 tv = load4(ts + 16 * i + 4 * j, tvec);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t v = pv[j] >> (8 * e) & 255u;
                    tally(acc, s_sig[v], v > 127u, tv[e]);
                }
            }
        }
        for (size_t i = 16 * nc + threadIdx.x; i < n; i += SC_THREADS) tally(acc, s_sig[ps[i]], ps[i] > 127, ts[i]);
    } else {
        const float *ps = (const float *)pred + first;
        const bool pvec = ((uintptr_t)ps & 15) == 0;
        const size_t nc = n / 4;
        for (size_t i = threadIdx.x; i < nc; i += SC_THREADS) {
            const f32x4 xv = load4(ps + 4 * i, pvec), tv = load4(ts + 4 * i, tvec);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float p, pq;
                sigmoid_parts(xv[e], p, pq);
                tally(acc, p, xv[e] > 0.5f, tv[e]);
            }
        }
        for (size_t i = 4 * nc + threadIdx.x; i < n; i += SC_THREADS) {
            float p, pq;
            sigmoid_parts(ps[i], p, pq);
            tally(acc, p, ps[i] > 0.5f, ts[i]);
        }
    }
    ScorePart v = {acc.pt, acc.p, acc.t, acc.tp, acc.fp, acc.fn};  // 64-bit counts from here on
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        ScorePart r = s_wave[0];
#pragma unroll
        for (int k = 1; k < SC_THREADS / 64; ++k) {
            r.pt += s_wave[k].pt;
            r.p += s_wave[k].p;
            r.t += s_wave[k].t;
            r.tp += s_wave[k].tp;
            r.fp += s_wave[k].fp;
            r.fn += s_wave[k].fn;
        }
        part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
    }
}

__device__ __forceinline__ double ratio(unsigned long long num, unsigned long long den) {
    return den ? (double)num / (double)den : 0.0;  // sklearn's zero_division="warn" value
}

// grid (batch), 64 threads
__global__ __launch_bounds__(64) void score_finish_kernel(const ScorePart *__restrict__ part, int groups, size_t count,
                                                          float smooth, long long *__restrict__ counts,
                                                          double *__restrict__ scores) {
    const int b = blockIdx.x;
    ScorePart a = {0.0, 0.0, 0.0, 0ull, 0ull, 0ull};
    for (int g = threadIdx.x; g < groups; g += 64) {
        const ScorePart v = part[(size_t)b * groups + g];
        a.pt += v.pt;
        a.p += v.p;
        a.t += v.t;
        a.tp += v.tp;
        a.fp += v.fp;
        a.fn += v.fn;
    }
    a = wave_sum(a);
    if (threadIdx.x != 0) return;
    const unsigned long long tp = a.tp, fp = a.fp, fn = a.fn, tn = (unsigned long long)count - tp - fp - fn;
    long long *c = counts + 4 * (size_t)b;
    c[0] = (long long)tp, c[1] = (long long)fp, c[2] = (long long)fn, c[3] = (long long)tn;
    double *s = scores + 7 * (size_t)b;
    s[0] = ratio(tp, tp + fp + fn);
    s[1] = ratio(2 * tp, 2 * tp + fp + fn);
    s[2] = ratio(tp, tp + fn);
    s[3] = ratio(tp, tp + fp);
    s[4] = (double)(tp + tn) / (double)count;
    // the area under the three-point ROC curve of a 0/1 score; undefined (NaN, as sklearn 1.7 returns) with one class only
    s[5] = (tp + fn) && (tn + fp) ? 0.5 * ((double)tp / (double)(tp + fn) + (double)tn / (double)(tn + fp)) : (double)NAN;
    const double sm = (double)smooth;
    s[6] = 1.0 - (2.0 * a.pt + sm) / (a.p + a.t + sm);
}

bool score_shape_ok(int32_t batch, size_t count) { return batch >= 1 && batch <= 65535 && count >= 1 && count <= SC_MAX_COUNT; }

}  // namespace

// [partials: batch x score_max_groups(count)]
extern "C" size_t ocm_mask_scores_workspace_bytes(int32_t batch, size_t count) {
    if (!score_shape_ok(batch, count)) return 0;
    return (size_t)batch * score_max_groups(count) * sizeof(ScorePart);
}

extern "C" int ocm_op_mask_scores(const void *pred, int32_t pred_is_u8, const float *target, int32_t batch, size_t count,
                                  float smooth, int64_t *counts, double *scores, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    if (!pred || !target || !counts || !scores) return fail(OCM_EINVAL, "null argument");
    if (batch < 1 || batch > 65535) return fail(OCM_EINVAL, "mask_scores: batch = %d (1..65535)", batch);
    if (count < 1 || count > SC_MAX_COUNT) return fail(OCM_EINVAL, "mask_scores: count = %zu (1..2^36 elements per image)", count);
    if (!std::isfinite(smooth) || smooth < 0.f) return fail(OCM_EINVAL, "mask_scores: smooth = %g (finite, >= 0)", (double)smooth);
    const size_t need = ocm_mask_scores_workspace_bytes(batch, count);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "mask_scores workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const ScorePlan p = score_plan(count);
    ScorePart *part = (ScorePart *)workspace;
    const dim3 grid(p.groups, batch), block(SC_THREADS);
    if (pred_is_u8)
        score_partial_kernel<true><<<grid, block, 0, s>>>(pred, target, part, count, p.span);
    else
        score_partial_kernel<false><<<grid, block, 0, s>>>(pred, target, part, count, p.span);
    HIP_TRY(hipGetLastError());
    score_finish_kernel<<<dim3(batch), dim3(64), 0, s>>>(part, p.groups, count, smooth, (long long *)counts, scores);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
