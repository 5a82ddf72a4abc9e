// kernels_kmeans_px.hip — cv2.kmeans(Z, 2, None, (EPS + MAX_ITER, max_iter, eps), attempts, KMEANS_RANDOM_CENTERS) on the
// pixel triples of a uint8 image, then np.uint8(centres)[labels] and its Otsu mask: the reference's utils.kmeans
// (utils.py:118-169, eval.py's "k-means" / "k-means_ours" methods) for a batch of independent problems on the device. The loop
// is restated from OpenCV 4.x modules/core/src/kmeans.cpp for K = 2, dims = 3; include/ocm_vit.h states it in full (parity with
// a live cv2 unpinned: cv2 is not installable here). The random centres come from uniforms the host draws (ocm_cv_rng_uniform,
// cv::RNG): their number does not depend on the data.
//   kmpx_attempt_kernel  grid (attempts, problems): one workgroup runs one attempt's whole loop. One pass over the samples per
//                        iteration: it assigns the labels (stored in the workspace, 16 per store) and counts cluster 1 and its
//                        column sums in per-thread 32-bit integers, widened to 64 bits and added over the wave by the xor
//                        butterfly and over the eight waves through LDS. Cluster 0 is the problem's total minus cluster 1. The
//                        last pass adds the float64 compactness in one fixed order instead. An empty cluster (a branch the whole
//                        workgroup takes together) costs one more pass: a (distance, index) maximum that prefers the larger
//                        index. The attempt's 3 N bytes stay in L2 between the passes.
//   kmpx_finish_kernel   grid (problems): the first attempt with the smallest compactness; its labels and centres; the histogram
//                        of res = uint8(centre)[label] (at most six bins) from the counts; the Otsu level by the statements of
//                        ocm_otsu_threshold (otsu.h); mask = res > level ? 255 : 0.
// Workgroups never communicate: no global atomics, no grid barrier, no spin wait, nothing synchronises with the host. A thread
// reads back only labels it stored itself. Sums of the samples are exact integers, rounded to float32 once; equal inputs give
// equal bits, alone or inside a batch.
// Problems start at p * 3 N bytes, so an N that is no multiple of 16 leaves later problems unaligned: 16-byte loads and stores
// where the problem's own address is 16-byte aligned, element accesses otherwise, the same elements per thread in the same
// order either way. Label slots in the workspace are padded to 16 bytes and always take the 16-byte path.
#include <cmath>

#include "host_common.h"
#include "otsu.h"

#define fail ocm_fail

// OpenCV's float32 statements one by one: no fused multiply-add
#pragma clang fp contract(off)

namespace {

constexpr int KP_THREADS = 512;  // measured against 256 and 1024 at 384 x 384
constexpr int KP_WAVES = KP_THREADS / 64;
static_assert(KP_THREADS >= 256 && KP_THREADS % 64 == 0, "kmpx_finish_kernel clears its 256 histogram bins with the first 256 threads");
constexpr int KP_CHUNK = 16;  // samples per chunk: 48 pixel bytes (three 16-byte loads), 16 label bytes (one store)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct alignas(16) KpAttempt {  // what an attempt leaves for the finishing launch
    float c[2][3];
    long long cnt1;  // members of cluster 1 (cluster 0: N - cnt1)
};

__device__ __forceinline__ u32x4 load16(const uint8_t *p, bool vec) {
    if (vec) return *(const u32x4 *)p;
    u32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        v[j] = (uint32_t)p[4 * j] | (uint32_t)p[4 * j + 1] << 8 | (uint32_t)p[4 * j + 2] << 16 | (uint32_t)p[4 * j + 3] << 24;
    return v;
}

__device__ __forceinline__ void store16(uint8_t *p, u32x4 v, bool vec) {
    if (vec) {
        *(u32x4 *)p = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) p[j] = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
}

struct Chunk {  // 16 samples
    u32x4 v[3];
    __device__ __forceinline__ void load(const uint8_t *p, bool vec) {
        v[0] = load16(p, vec), v[1] = load16(p + 16, vec), v[2] = load16(p + 32, vec);
    }
    __device__ __forceinline__ uint32_t byte(int b) const { return v[b >> 4][(b >> 2) & 3] >> (8 * (b & 3)) & 255u; }
};

// ((t0 t0 + t1 t1) + t2 t2), t = x - c, in float32
__device__ __forceinline__ float dist3(float x0, float x1, float x2, const float *c) {
    const float t0 = x0 - c[0], t1 = x1 - c[1], t2 = x2 - c[2];
    return (t0 * t0 + t1 * t1) + t2 * t2;
}

// Integer sums over the workgroup, every thread gets the totals. s: K x KP_WAVES slots.
template <int K>
__device__ __forceinline__ void block_sum(unsigned long long (&v)[K], unsigned long long *s) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    __syncthreads();  // an earlier use of s has been read by everyone
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k * KP_WAVES + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        unsigned long long r = s[k * KP_WAVES];
#pragma unroll
        for (int w = 1; w < KP_WAVES; ++w) r += s[k * KP_WAVES + w];
        v[k] = r;
    }
}

// The largest key of the workgroup in every thread (ties are equal keys).
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long *s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long r = s[0];
#pragma unroll
    for (int w = 1; w < KP_WAVES; ++w) r = s[w] > r ? s[w] : r;
    return r;
}

// grid (attempts, problems). n: samples per problem; label_stride: bytes per label slot, a multiple of 16.
__global__ __launch_bounds__(KP_THREADS) void kmpx_attempt_kernel(const uint8_t *__restrict__ pixels,
                                                                  const float *__restrict__ uniforms, uint8_t *ws_labels,
                                                                  KpAttempt *__restrict__ ws_att, double *__restrict__ compactness,
                                                                  int *__restrict__ iters, long long n, size_t label_stride,
                                                                  int iter_cap, double eps2) {
    __shared__ unsigned long long s_red[4 * KP_WAVES];
    __shared__ double s_dsum[KP_WAVES];
    const int tid = threadIdx.x;
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;  // [problem][attempt]
    const uint8_t *px = pixels + (size_t)blockIdx.y * 3 * (size_t)n;
    const bool vec = ((uintptr_t)px & 15) == 0;
    uint8_t *lab = ws_labels + slot * label_stride;
    const long long nc = n / KP_CHUNK;
    const long long tail = nc * KP_CHUNK + tid;  // this thread's sample past the whole chunks, when tail < n

    // the box and the column totals
    uint32_t lo[3] = {255u, 255u, 255u}, hi[3] = {0u, 0u, 0u}, ts[3] = {0u, 0u, 0u};
    for (long long ch = tid; ch < nc; ch += KP_THREADS) {
        Chunk q;
        q.load(px + 48 * ch, vec);
#pragma unroll
        for (int i = 0; i < KP_CHUNK; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t x = q.byte(3 * i + j);
                lo[j] = min(lo[j], x), hi[j] = max(hi[j], x), ts[j] += x;
            }
    }
    if (tail < n) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t x = px[3 * tail + j];
            lo[j] = min(lo[j], x), hi[j] = max(hi[j], x), ts[j] += x;
        }
    }
    unsigned long long tot[3] = {ts[0], ts[1], ts[2]};
    block_sum<3>(tot, s_red);
    // both ends of the box as maxima: of 255 - lo and of hi
    float flo[3], fhi[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const unsigned long long a = block_max((unsigned long long)(255u - lo[j]), s_red);
        const unsigned long long b = block_max((unsigned long long)hi[j], s_red);
        flo[j] = (float)(255u - (uint32_t)a), fhi[j] = (float)(uint32_t)b;
    }

    // c = (u (1 + 2 margin) - margin) (hi - lo) + lo, margin = 1 / 3
    float c[2][3];
    {
        const float margin = 1.f / 3;
        const float *u = uniforms + slot * 6;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) c[k][j] = (u[3 * k + j] * (1.f + margin * 2.f) - margin) * (fhi[j] - flo[j]) + flo[j];
    }

    unsigned long long cnt1 = 0, sum1[3] = {0, 0, 0};  // of the labels in `lab`, the same in every thread
    int iter = 0;
    for (;;) {
        double shift = INFINITY;
        if (iter > 0) {
            if (cnt1 == 0 || cnt1 == (unsigned long long)n) {  // the same decision in every thread
                // K = 2: the other cluster m holds every sample, so b is the mean of them all and every sample is a candidate
                const uint32_t k = cnt1 == 0;  // the empty cluster
                float b[3];
                const float inv = __fdiv_rn(1.f, (float)(unsigned long long)n);
#pragma unroll
                for (int j = 0; j < 3; ++j) b[j] = (float)tot[j] * inv;
                // a distance is no less than +0, so its bits order as an integer: (distance, index), the larger index on a tie
                unsigned long long best = 0;
                for (long long ch = tid; ch < nc; ch += KP_THREADS) {
                    Chunk q;
                    q.load(px + 48 * ch, vec);
#pragma unroll
                    for (int i = 0; i < KP_CHUNK; ++i) {
                        const float d = dist3((float)q.byte(3 * i), (float)q.byte(3 * i + 1), (float)q.byte(3 * i + 2), b);
                        const unsigned long long key =
                            (unsigned long long)__float_as_uint(d) << 32 | (unsigned long long)(ch * KP_CHUNK + i);
                        best = key > best ? key : best;
                    }
                }
                if (tail < n) {
                    const float d = dist3((float)px[3 * tail], (float)px[3 * tail + 1], (float)px[3 * tail + 2], b);
                    const unsigned long long key = (unsigned long long)__float_as_uint(d) << 32 | (unsigned long long)tail;
                    best = key > best ? key : best;
                }
                best = block_max(best, s_red);
                const long long far = (long long)(best & 0xffffffffull);
                // its owner relabels it: a thread reads back only labels it stored itself
                const long long owner = far < nc * KP_CHUNK ? (far / KP_CHUNK) % KP_THREADS : far - nc * KP_CHUNK;
                if (tid == owner) lab[far] = (uint8_t)k;
                cnt1 = k ? 1ull : (unsigned long long)n - 1;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const unsigned long long x = px[3 * far + j];
                    sum1[j] = k ? x : tot[j] - x;
                }
            }
            const float inv0 = __fdiv_rn(1.f, (float)((unsigned long long)n - cnt1)), inv1 = __fdiv_rn(1.f, (float)cnt1);
            double d0 = 0.0, d1 = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float n0 = (float)(tot[j] - sum1[j]) * inv0, n1 = (float)sum1[j] * inv1;
                const double t0 = (double)(n0 - c[0][j]), t1 = (double)(n1 - c[1][j]);
                d0 += t0 * t0, d1 += t1 * t1;
                c[0][j] = n0, c[1][j] = n1;
            }
            shift = fmax(d0, d1);
        }
        const bool last = ++iter == iter_cap || shift <= eps2;
        if (last) break;

        // assignment: label 1 when d(x, c1) < d(x, c0), a tie goes to 0
        uint32_t t_cnt = 0, t_sum[3] = {0u, 0u, 0u};
        for (long long ch = tid; ch < nc; ch += KP_THREADS) {
            Chunk q;
            q.load(px + 48 * ch, vec);
            u32x4 lw = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < KP_CHUNK; ++i) {
                const uint32_t x0 = q.byte(3 * i), x1 = q.byte(3 * i + 1), x2 = q.byte(3 * i + 2);
                const uint32_t l = dist3((float)x0, (float)x1, (float)x2, c[1]) < dist3((float)x0, (float)x1, (float)x2, c[0]);
                lw[i >> 2] |= l << (8 * (i & 3));
                t_cnt += l, t_sum[0] += l * x0, t_sum[1] += l * x1, t_sum[2] += l * x2;
            }
            *(u32x4 *)(lab + 16 * ch) = lw;
        }
        if (tail < n) {
            const uint32_t x0 = px[3 * tail], x1 = px[3 * tail + 1], x2 = px[3 * tail + 2];
            const uint32_t l = dist3((float)x0, (float)x1, (float)x2, c[1]) < dist3((float)x0, (float)x1, (float)x2, c[0]);
            lab[tail] = (uint8_t)l;
            t_cnt += l, t_sum[0] += l * x0, t_sum[1] += l * x1, t_sum[2] += l * x2;
        }
        unsigned long long r[4] = {t_cnt, t_sum[0], t_sum[1], t_sum[2]};
        block_sum<4>(r, s_red);
        cnt1 = r[0], sum1[0] = r[1], sum1[1] = r[2], sum1[2] = r[3];
    }

    // compactness of the labels as they stand (not reassigned): float64, per thread in index order, the wave by the xor
    // butterfly, the eight waves in order
    double acc = 0.0;
    for (long long ch = tid; ch < nc; ch += KP_THREADS) {
        Chunk q;
        q.load(px + 48 * ch, vec);
        const u32x4 lw = *(const u32x4 *)(lab + 16 * ch);
#pragma unroll
        for (int i = 0; i < KP_CHUNK; ++i) {
            const bool l = lw[i >> 2] >> (8 * (i & 3)) & 1u;
            const float cc[3] = {l ? c[1][0] : c[0][0], l ? c[1][1] : c[0][1], l ? c[1][2] : c[0][2]};
            acc += (double)dist3((float)q.byte(3 * i), (float)q.byte(3 * i + 1), (float)q.byte(3 * i + 2), cc);
        }
    }
    if (tail < n) {
        const bool l = lab[tail] & 1u;
        const float cc[3] = {l ? c[1][0] : c[0][0], l ? c[1][1] : c[0][1], l ? c[1][2] : c[0][2]};
        acc += (double)dist3((float)px[3 * tail], (float)px[3 * tail + 1], (float)px[3 * tail + 2], cc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((tid & 63) == 0) s_dsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double r = s_dsum[0];
#pragma unroll
        for (int w = 1; w < KP_WAVES; ++w) r += s_dsum[w];
        compactness[slot] = r;
        iters[slot] = iter;
        KpAttempt out;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) out.c[k][j] = c[k][j];
        out.cnt1 = (long long)cnt1;
        ws_att[slot] = out;
    }
}

// grid (problems)
__global__ __launch_bounds__(KP_THREADS) void kmpx_finish_kernel(const uint8_t *__restrict__ ws_labels,
                                                                 const KpAttempt *__restrict__ ws_att,
                                                                 const double *__restrict__ compactness, uint8_t *__restrict__ labels,
                                                                 float *__restrict__ centers, int *__restrict__ best,
                                                                 uint8_t *__restrict__ mask, long long n, size_t label_stride,
                                                                 int attempts) {
    __shared__ unsigned long long s_hist[256];
    __shared__ int s_level;
    const int tid = threadIdx.x, p = blockIdx.x;
    // an attempt replaces the best only when its compactness is strictly smaller (a NaN never is)
    int a = 0;
    double bc = compactness[(size_t)p * attempts];
    for (int k = 1; k < attempts; ++k) {
        const double v = compactness[(size_t)p * attempts + k];
        if (v < bc) bc = v, a = k;
    }
    const KpAttempt att = ws_att[(size_t)p * attempts + a];
    uint32_t res[2][3];  // np.uint8(centres): the centres are means of bytes, truncated
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) res[k][j] = (uint32_t)(int)att.c[k][j] & 255u;
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long cnt[2] = {(unsigned long long)(n - att.cnt1), (unsigned long long)att.cnt1};
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 3; ++j) s_hist[res[k][j]] += cnt[k];
        s_level = ocm_otsu_level((const uint64_t *)s_hist, 3 * n);
        best[p] = a;
        for (int k = 0; k < 2; ++k)
            for (int j = 0; j < 3; ++j) centers[(size_t)p * 6 + 3 * k + j] = att.c[k][j];
    }
    __syncthreads();
    const uint32_t level = (uint32_t)s_level;
    uint32_t mv[2][3];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) mv[k][j] = res[k][j] > level ? 255u : 0u;

    const uint8_t *src = ws_labels + ((size_t)p * attempts + a) * label_stride;
    uint8_t *lab = labels + (size_t)p * (size_t)n, *mk = mask + (size_t)p * 3 * (size_t)n;
    const bool lvec = ((uintptr_t)lab & 15) == 0, mvec = ((uintptr_t)mk & 15) == 0;
    const long long nc = n / KP_CHUNK;
    for (long long ch = tid; ch < nc; ch += KP_THREADS) {
        const u32x4 lw = *(const u32x4 *)(src + 16 * ch);
        store16(lab + 16 * ch, lw, lvec);
        u32x4 m[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
        for (int i = 0; i < KP_CHUNK; ++i) {
            const bool l = lw[i >> 2] >> (8 * (i & 3)) & 1u;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int b = 3 * i + j;
                m[b >> 4][(b >> 2) & 3] |= (l ? mv[1][j] : mv[0][j]) << (8 * (b & 3));
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) store16(mk + 48 * ch + 16 * k, m[k], mvec);
    }
    const long long tail = nc * KP_CHUNK + tid;
    if (tail < n) {
        const uint8_t l = src[tail];
        lab[tail] = l;
#pragma unroll
        for (int j = 0; j < 3; ++j) mk[3 * tail + j] = (uint8_t)(l ? mv[1][j] : mv[0][j]);
    }
}

constexpr int64_t KP_MAX_SAMPLES = (int64_t)1 << 24;  // 255 N < 2^32: a thread's 32-bit sums and a 32-bit index hold

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t label_stride(int64_t samples) { return ((size_t)samples + 15) & ~(size_t)15; }

bool shape_ok(int32_t problems, int64_t samples, int32_t attempts) {
    return problems >= 1 && problems <= 65535 && samples >= 2 && samples <= KP_MAX_SAMPLES && attempts >= 1 && attempts <= 32;
}

}  // namespace

// cv::RNG: state = (state & 0xffffffff) * 4164903690 + (state >> 32); a draw is (float)(uint32)state * 2^-32 as a float32 product
extern "C" int ocm_cv_rng_uniform(uint64_t *state, float *out, int64_t n) {
    if (!state || n < 0 || (n > 0 && !out)) return fail(OCM_EINVAL, "cv_rng_uniform: null argument or n = %lld < 0", (long long)n);
    uint64_t s = *state ? *state : 0xffffffffull;  // cv::RNG's seed 0, and a fresh process's state
    for (int64_t i = 0; i < n; ++i) {
        s = (uint64_t)(uint32_t)s * 4164903690u + (s >> 32);
        out[i] = (float)(uint32_t)s * 2.3283064365386963e-10f;
    }
    *state = s;
    return OCM_OK;
}

// [labels: problems x attempts slots of samples rounded up to 16 bytes][problems x attempts KpAttempt]
extern "C" size_t ocm_kmeans_px_workspace_bytes(int32_t problems, int64_t samples, int32_t attempts) {
    if (!shape_ok(problems, samples, attempts)) return 0;
    const size_t slots = (size_t)problems * attempts;
    return align256(slots * label_stride(samples)) + align256(slots * sizeof(KpAttempt));
}

extern "C" int ocm_op_kmeans_px(const uint8_t *pixels, int32_t problems, int64_t samples, const float *uniforms, int32_t attempts,
                                int32_t max_iter, double eps, uint8_t *labels, float *centers, double *compactness, int32_t *iters,
                                int32_t *best, uint8_t *mask, void *workspace, size_t workspace_bytes, void *stream) {
    if (!pixels || !uniforms || !labels || !centers || !compactness || !iters || !best || !mask)
        return fail(OCM_EINVAL, "null argument");
    if (problems < 1 || problems > 65535) return fail(OCM_EINVAL, "kmeans_px: problems = %d (1..65535)", problems);
    if (samples < 2 || samples > KP_MAX_SAMPLES)
        return fail(OCM_EINVAL, "kmeans_px: samples = %lld (2..2^24 pixel triples per problem)", (long long)samples);
    if (attempts < 1 || attempts > 32) return fail(OCM_EINVAL, "kmeans_px: attempts = %d (1..32)", attempts);
    if (max_iter < 1 || max_iter > 1000) return fail(OCM_EINVAL, "kmeans_px: max_iter = %d (1..1000)", max_iter);
    if (!std::isfinite(eps) || eps < 0.0) return fail(OCM_EINVAL, "kmeans_px: eps = %g (finite, >= 0)", eps);
    const size_t need = ocm_kmeans_px_workspace_bytes(problems, samples, attempts);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "kmeans_px workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 15) return fail(OCM_EINVAL, "kmeans_px workspace: not 16-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const size_t slots = (size_t)problems * attempts, stride = label_stride(samples);
    uint8_t *ws_labels = (uint8_t *)workspace;
    KpAttempt *ws_att = (KpAttempt *)((char *)workspace + align256(slots * stride));
    kmpx_attempt_kernel<<<dim3(attempts, problems), dim3(KP_THREADS), 0, s>>>(pixels, uniforms, ws_labels, ws_att, compactness, iters,
                                                                            (long long)samples, stride, max_iter < 2 ? 2 : max_iter,
                                                                            eps * eps);
    HIP_TRY(hipGetLastError());
    kmpx_finish_kernel<<<dim3(problems), dim3(KP_THREADS), 0, s>>>(ws_labels, ws_att, compactness, labels, centers, best, mask,
                                                                 (long long)samples, stride, attempts);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
