// kernels_dino.hip — the row kernels of DINO self-distillation (dino/vision_transformer.py DINOHead, dino/utils.py DINOLoss):
// the head's L2 normalisation and weight-normed last layer, forward and backward, the DINO loss over out_dim columns with its
// one-pass gradient, and the centre's batch sum and momentum update. Everything is fp32 data, memory-bound, and free of atomics.
//   l2norm_kernel / l2norm_bwd_kernel    one workgroup per row of `dim` floats
//   wnorm_kernel / wnorm_bwd_kernel      one workgroup per row of the (N, K) direction tensor v
//   loss_stats_kernel                    one workgroup per logit row (V*B student rows, then 2*B teacher rows): the row maximum
//                                        and the sum of exp(z - max), z = S / ts or (T - c) / tt
//   loss_dots_kernel                     one workgroup per (image b, slice of LOSS_SLICE columns): the 2 x V table of q_i . S_v over
//                                        the slice, the teacher probabilities q_0, q_1 of the slice held in registers
//   loss_finish_kernel                   one workgroup: adds the slices in order, forms the loss from the identity
//                                        sum_k q l = (q . S_v) / ts - lse_v
//   loss_bwd_kernel                      one workgroup per (b, slice): dS of all V crops, q_0, q_1 in registers again
//   center_sum_kernel                    one lane per four columns, the rows added in rising order in fp32
//   center_update_kernel                 c = c m + (sum / n) (1 - m), three roundings
// A thread owns quads of four consecutive elements (quad j of a row or slice: thread j % 256, in rising j); a quad that lies
// wholly inside the row is read with one 16-byte load when its row pointer is 16-byte aligned and element by element otherwise,
// the quad that straddles the end of a row element by element up to the end. Both ways give a thread the same elements in the
// same order, so the sums (per thread in float64, the xor butterfly of a wave, the waves in order) have one fixed order: equal
// inputs give equal bits wherever they lie. Every output element is written exactly once and no access goes past a row.
#include <cmath>

#include "common.h"
#include "host_common.h"

#define fail ocm_fail

// the centre update and the EMA are torch's statements operation by operation; the rest gains nothing from contraction either
#pragma clang fp contract(off)

namespace {

constexpr int DN_THREADS = 256;
constexpr int DN_WAVES = DN_THREADS / 64;
constexpr int LOSS_QUADS = 4;                             // quads per thread and slice
constexpr int LOSS_SLICE = DN_THREADS * 4 * LOSS_QUADS;   // 4096 columns per workgroup
constexpr int CS_THREADS = 64;                            // centre sum: 256 columns per workgroup
constexpr float L2_EPS = 1e-12f;                          // F.normalize's eps

__device__ __forceinline__ bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// elements k .. k+3 of a row of n (k % 4 == 0, k < n): zeros past the end
__device__ __forceinline__ f32x4 load_quad(const float *row, int k, int n, bool vec) {
    if (k + 4 <= n) {
        if (vec) return *(const f32x4 *)(row + k);
        f32x4 v;
        v[0] = row[k], v[1] = row[k + 1], v[2] = row[k + 2], v[3] = row[k + 3];
        return v;
    }
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < 4; ++e)
        if (k + e < n) v[e] = row[k + e];
    return v;
}

__device__ __forceinline__ void store_quad(float *row, int k, int n, f32x4 v, bool vec) {
    if (k + 4 <= n) {
        if (vec) {
            *(f32x4 *)(row + k) = v;
        } else {
            row[k] = v[0], row[k + 1] = v[1], row[k + 2] = v[2], row[k + 3] = v[3];
        }
        return;
    }
    for (int e = 0; e < 4; ++e)
        if (k + e < n) row[k + e] = v[e];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// the workgroup's sum in every thread; s_wave holds DN_WAVES doubles and may be reused after the call
__device__ __forceinline__ double block_sum(double v, double *s_wave) {
    v = wave_sum(v);
    __syncthreads();  // the previous use of s_wave is over
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s_wave[0];
#pragma unroll
    for (int k = 1; k < DN_WAVES; ++k) r += s_wave[k];
    return r;
}

__device__ __forceinline__ float block_max(float v, float *s_wave) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = s_wave[0];
#pragma unroll
    for (int k = 1; k < DN_WAVES; ++k) r = fmaxf(r, s_wave[k]);
    return r;
}

// sum_k a[k] b[k] of one row, the products and the sum in float64
__device__ __forceinline__ double row_dot(const float *a, const float *b, int n, double *s_wave) {
    const bool va = aligned16(a), vb = aligned16(b);
    double acc = 0.0;
    for (int k = 4 * (int)threadIdx.x; k < n; k += 4 * DN_THREADS) {
        const f32x4 x = load_quad(a, k, n, va), y = load_quad(b, k, n, vb);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)x[e] * (double)y[e];
    }
    return block_sum(acc, s_wave);
}

// ---- F.normalize(p = 2, dim = -1) ----
__global__ __launch_bounds__(DN_THREADS) void l2norm_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                            float *__restrict__ norm, int dim) {
    __shared__ double s_wave[DN_WAVES];
    const float *xr = x + (size_t)blockIdx.x * dim;
    float *yr = y + (size_t)blockIdx.x * dim;
    float nrm = (float)sqrt(row_dot(xr, xr, dim, s_wave));
    nrm = fmaxf(nrm, L2_EPS);
    const bool vx = aligned16(xr), vy = aligned16(yr);
    for (int k = 4 * (int)threadIdx.x; k < dim; k += 4 * DN_THREADS) {
        f32x4 v = load_quad(xr, k, dim, vx);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / nrm;
        store_quad(yr, k, dim, v, vy);
    }
    if (threadIdx.x == 0) norm[blockIdx.x] = nrm;
}

// dx = (dy - y (y . dy)) / norm; a row whose norm is the clamp itself passes dy / eps, as the clamp's zero gradient gives
__global__ __launch_bounds__(DN_THREADS) void l2norm_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ y,
                                                                const float *__restrict__ norm, float *__restrict__ dx, int dim) {
    __shared__ double s_wave[DN_WAVES];
    const float *gr = dy + (size_t)blockIdx.x * dim;
    const float *yr = y + (size_t)blockIdx.x * dim;
    float *dr = dx + (size_t)blockIdx.x * dim;
    const float nrm = norm[blockIdx.x];
    const bool clamped = nrm <= L2_EPS;
    const float dot = clamped ? 0.f : (float)row_dot(gr, yr, dim, s_wave);
    const bool vg = aligned16(gr), vy = aligned16(yr), vd = aligned16(dr);
    for (int k = 4 * (int)threadIdx.x; k < dim; k += 4 * DN_THREADS) {
        const f32x4 g = load_quad(gr, k, dim, vg), yy = load_quad(yr, k, dim, vy);
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = clamped ? g[e] / nrm : (g[e] - yy[e] * dot) / nrm;
        store_quad(dr, k, dim, d, vd);
    }
}

// ---- nn.utils.weight_norm, dim = 0: W[n] = g[n] v[n] / |v[n]| ----
__global__ __launch_bounds__(DN_THREADS) void wnorm_kernel(const float *__restrict__ v, const float *__restrict__ g,
                                                           float *__restrict__ w, float *__restrict__ norm, int K) {
    __shared__ double s_wave[DN_WAVES];
    const float *vr = v + (size_t)blockIdx.x * K;
    float *wr = w + (size_t)blockIdx.x * K;
    const float nrm = (float)sqrt(row_dot(vr, vr, K, s_wave));
    const float scale = g[blockIdx.x] / nrm;
    const bool vv = aligned16(vr), vw = aligned16(wr);
    for (int k = 4 * (int)threadIdx.x; k < K; k += 4 * DN_THREADS) {
        f32x4 x = load_quad(vr, k, K, vv);
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] * scale;
        store_quad(wr, k, K, x, vw);
    }
    if (threadIdx.x == 0) norm[blockIdx.x] = nrm;
}

// dg = (dW . v) / |v|,  dv = g / |v| (dW - v (dW . v) / |v|^2)
__global__ __launch_bounds__(DN_THREADS) void wnorm_bwd_kernel(const float *__restrict__ dw, const float *__restrict__ v,
                                                               const float *__restrict__ g, const float *__restrict__ norm,
                                                               float *__restrict__ dg, float *__restrict__ dv, int K) {
    __shared__ double s_wave[DN_WAVES];
    const float *gr = dw + (size_t)blockIdx.x * K;
    const float *vr = v + (size_t)blockIdx.x * K;
    const float nrm = norm[blockIdx.x];
    const double dot = row_dot(gr, vr, K, s_wave);
    if (dg && threadIdx.x == 0) dg[blockIdx.x] = (float)(dot / (double)nrm);
    if (!dv) return;
    float *dr = dv + (size_t)blockIdx.x * K;
    const float scale = g[blockIdx.x] / nrm;
    const float coef = (float)(dot / ((double)nrm * (double)nrm));
    const bool vg = aligned16(gr), vv = aligned16(vr), vd = aligned16(dr);
    for (int k = 4 * (int)threadIdx.x; k < K; k += 4 * DN_THREADS) {
        const f32x4 a = load_quad(gr, k, K, vg), x = load_quad(vr, k, K, vv);
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = scale * (a[e] - x[e] * coef);
        store_quad(dr, k, K, d, vd);
    }
}

// ---- the DINO loss ----
// stats[row] = (max_k z, sum_k exp(z - max)) in float64; rows 0 .. V*B-1 the student's (z = S / ts), then 2*B teacher rows
// (z = (T - c) / tt). The second pass over the row is served by the caches for rows up to a few MB.
__global__ __launch_bounds__(DN_THREADS) void loss_stats_kernel(const float *__restrict__ student, const float *__restrict__ teacher,
                                                                const float *__restrict__ center, float ts, float tt,
                                                                int student_rows, int K, double *__restrict__ stats) {
    __shared__ double s_wave[DN_WAVES];
    __shared__ float s_max[DN_WAVES];
    const int row = blockIdx.x;
    const bool is_teacher = row >= student_rows;
    const float *r = is_teacher ? teacher + (size_t)(row - student_rows) * K : student + (size_t)row * K;
    const float temp = is_teacher ? tt : ts;
    const bool vr = aligned16(r), vc = aligned16(center);
    float m = -INFINITY;
    for (int k = 4 * (int)threadIdx.x; k < K; k += 4 * DN_THREADS) {
        f32x4 x = load_quad(r, k, K, vr);
        if (is_teacher) {
            const f32x4 c = load_quad(center, k, K, vc);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = x[e] - c[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) m = fmaxf(m, x[e] / temp);
    }
    m = block_max(m, s_max);
    double acc = 0.0;
    for (int k = 4 * (int)threadIdx.x; k < K; k += 4 * DN_THREADS) {
        f32x4 x = load_quad(r, k, K, vr);
        if (is_teacher) {
            const f32x4 c = load_quad(center, k, K, vc);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = x[e] - c[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < K) acc += (double)expf(x[e] / temp - m);
    }
    const double sum = block_sum(acc, s_wave);
    if (threadIdx.x == 0) stats[2 * (size_t)row] = (double)m, stats[2 * (size_t)row + 1] = sum;
}

// the teacher probabilities of this thread's quads of slice `slice` of image b: q[i][j] = exp(z - max_i) / sum_i, 0 past K
__device__ __forceinline__ void teacher_quads(const float *__restrict__ teacher, const float *__restrict__ center,
                                              const double *__restrict__ tstats, float tt, int B, int K, int b, int k0,
                                              f32x4 (&q)[2][LOSS_QUADS]) {
    const bool vc = aligned16(center);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const size_t row = (size_t)i * B + b;
        const float *tr = teacher + row * K;
        const bool vt = aligned16(tr);
        const float m = (float)tstats[2 * row], sum = (float)tstats[2 * row + 1];
#pragma unroll
        for (int j = 0; j < LOSS_QUADS; ++j) {
            const int k = k0 + 4 * ((int)threadIdx.x + j * DN_THREADS);
            f32x4 p = {0.f, 0.f, 0.f, 0.f};
            if (k < K) {
                const f32x4 t = load_quad(tr, k, K, vt), c = load_quad(center, k, K, vc);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < K) p[e] = expf((t[e] - c[e]) / tt - m) / sum;
            }
            q[i][j] = p;
        }
    }
}

// dots[((b * slices + slice) * 2 + i) * V + v] = sum over the slice of q[i, b, k] S[v, b, k]
__global__ __launch_bounds__(DN_THREADS) void loss_dots_kernel(const float *__restrict__ student, const float *__restrict__ teacher,
                                                               const float *__restrict__ center, const double *__restrict__ stats,
                                                               float tt, int B, int V, int K, double *__restrict__ dots) {
    __shared__ double s_wave[DN_WAVES];
    const int b = blockIdx.x, slice = blockIdx.y, slices = gridDim.y;
    const int k0 = slice * LOSS_SLICE;
    f32x4 q[2][LOSS_QUADS];
    teacher_quads(teacher, center, stats + 2 * (size_t)V * B, tt, B, K, b, k0, q);
    double *out = dots + ((size_t)b * slices + slice) * 2 * V;
    for (int v = 0; v < V; ++v) {
        const float *sr = student + ((size_t)v * B + b) * K;
        const bool vs = aligned16(sr);
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int j = 0; j < LOSS_QUADS; ++j) {
            const int k = k0 + 4 * ((int)threadIdx.x + j * DN_THREADS);
            if (k < K) {
                const f32x4 s = load_quad(sr, k, K, vs);
#pragma unroll
                for (int e = 0; e < 4; ++e) a0 += (double)q[0][j][e] * (double)s[e], a1 += (double)q[1][j][e] * (double)s[e];
            }
        }
        a0 = block_sum(a0, s_wave);
        a1 = block_sum(a1, s_wave);
        if (threadIdx.x == 0) out[v] = a0, out[V + v] = a1;
    }
}

// loss = 1 / (2 (V - 1) B) sum_b sum_i sum_{v != i} (lse[v, b] - (q_i . S_v) / ts)
__global__ __launch_bounds__(DN_THREADS) void loss_finish_kernel(const double *__restrict__ stats, const double *__restrict__ dots,
                                                                 float ts, int B, int V, int slices, float *__restrict__ loss) {
    __shared__ double s_wave[DN_WAVES];
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += DN_THREADS) {
        for (int v = 0; v < V; ++v) {
            const size_t row = (size_t)v * B + b;
            const double lse = stats[2 * row] + log(stats[2 * row + 1]);
            for (int i = 0; i < 2; ++i) {
                if (i == v) continue;
                double d = 0.0;
                for (int s = 0; s < slices; ++s) d += dots[(((size_t)b * slices + s) * 2 + i) * V + v];
                acc += lse - d / (double)ts;
            }
        }
    }
    const double total = block_sum(acc, s_wave);
    if (threadIdx.x == 0) *loss = (float)(total / (2.0 * (V - 1) * (double)B));
}

// dS[v, b, k] = g / (2 (V - 1) B ts) (c_v p[v, b, k] - sum_{i != v} q[i, b, k]),  c_v = 1 for v < 2, else 2
__global__ __launch_bounds__(DN_THREADS) void loss_bwd_kernel(const float *__restrict__ grad_loss, const float *__restrict__ student,
                                                              const float *__restrict__ teacher, const float *__restrict__ center,
                                                              const double *__restrict__ stats, float ts, float tt, int B, int V,
                                                              int K, float *__restrict__ dstudent) {
    const int b = blockIdx.x, k0 = blockIdx.y * LOSS_SLICE;
    f32x4 q[2][LOSS_QUADS];
    teacher_quads(teacher, center, stats + 2 * (size_t)V * B, tt, B, K, b, k0, q);
    const float scale = (float)((double)grad_loss[0] / (2.0 * (V - 1) * (double)B * (double)ts));
    for (int v = 0; v < V; ++v) {
        const size_t row = (size_t)v * B + b;
        const float *sr = student + row * K;
        float *dr = dstudent + row * K;
        const bool vs = aligned16(sr), vd = aligned16(dr);
        const float m = (float)stats[2 * row], sum = (float)stats[2 * row + 1];
        const float cv = v < 2 ? 1.f : 2.f;
#pragma unroll
        for (int j = 0; j < LOSS_QUADS; ++j) {
            const int k = k0 + 4 * ((int)threadIdx.x + j * DN_THREADS);
            if (k < K) {
                const f32x4 s = load_quad(sr, k, K, vs);
                f32x4 d;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = expf(s[e] / ts - m) / sum;
                    const float qs = v == 0 ? q[1][j][e] : v == 1 ? q[0][j][e] : q[0][j][e] + q[1][j][e];
                    d[e] = scale * (cv * p - qs);
                }
                store_quad(dr, k, K, d, vd);
            }
        }
    }
}

// ---- the centre ----
// sum[k] = ((T[0][k] + T[1][k]) + T[2][k]) + ... in fp32
__global__ __launch_bounds__(CS_THREADS) void center_sum_kernel(const float *__restrict__ teacher, int64_t rows, int K,
                                                                float *__restrict__ sum) {
    const int k = 4 * (int)(blockIdx.x * CS_THREADS + threadIdx.x);
    if (k >= K) return;
    f32x4 acc = load_quad(teacher, k, K, aligned16(teacher));
    for (int64_t r = 1; r < rows; ++r) {
        const float *tr = teacher + (size_t)r * K;
        const f32x4 t = load_quad(tr, k, K, aligned16(tr));
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + t[e];
    }
    store_quad(sum, k, K, acc, aligned16(sum));
}

// center = center * m + (sum / n) * w, each operation rounded on its own
__global__ __launch_bounds__(DN_THREADS) void center_update_kernel(float *__restrict__ center, const float *__restrict__ sum, int K,
                                                                   float n, float m, float w) {
    const int k = 4 * (int)(blockIdx.x * DN_THREADS + threadIdx.x);
    if (k >= K) return;
    const bool vc = aligned16(center);
    f32x4 c = load_quad(center, k, K, vc);
    const f32x4 s = load_quad(sum, k, K, aligned16(sum));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float mean = s[e] / n;
        const float keep = c[e] * m;
        const float add = mean * w;
        c[e] = keep + add;
    }
    store_quad(center, k, K, c, vc);
}

bool misaligned4(const void *p) { return ((uintptr_t)p & 3) != 0; }

int rows_ok(const char *op, int64_t rows, int32_t dim) {
    if (rows < 1 || rows > 0x7fffffff || dim < 1) return fail(OCM_EINVAL, "%s: rows = %lld, dim = %d (1 .. 2^31 - 1 rows, dim >= 1)", op, (long long)rows, dim);
    return OCM_OK;
}

int loss_shape_ok(const char *op, int32_t B, int32_t V, int32_t K, float ts, float tt) {
    if (B < 1 || V < 2 || K < 1) return fail(OCM_EINVAL, "%s: B = %d, V = %d, K = %d (B >= 1, V >= 2, K >= 1)", op, B, V, K);
    if ((int64_t)B * (V + 2) > 0x7fffffff || (int64_t)((K + LOSS_SLICE - 1) / LOSS_SLICE) > 65535)
        return fail(OCM_EINVAL, "%s: B = %d, V = %d, K = %d: too many rows or columns for one grid", op, B, V, K);
    if (!(ts > 0.f) || !(tt > 0.f) || !std::isfinite(ts) || !std::isfinite(tt))
        return fail(OCM_EINVAL, "%s: student_temp = %g, teacher_temp = %g (finite, > 0)", op, ts, tt);
    return OCM_OK;
}

int loss_slices(int32_t K) { return (K + LOSS_SLICE - 1) / LOSS_SLICE; }

}  // namespace

extern "C" int ocm_op_l2_normalize(const float *x, float *y, float *norm, int64_t rows, int32_t dim, void *stream) {
    if (!x || !y || !norm) return fail(OCM_EINVAL, "l2_normalize: null argument");
    if (misaligned4(x) || misaligned4(y) || misaligned4(norm)) return fail(OCM_EINVAL, "l2_normalize: a pointer is not 4-byte aligned");
    if (int rc = rows_ok("l2_normalize", rows, dim)) return rc;
    l2norm_kernel<<<dim3((unsigned)rows), dim3(DN_THREADS), 0, (hipStream_t)stream>>>(x, y, norm, dim);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_l2_normalize_backward(const float *dy, const float *y, const float *norm, float *dx, int64_t rows, int32_t dim,
                                            void *stream) {
    if (!dy || !y || !norm || !dx) return fail(OCM_EINVAL, "l2_normalize_backward: null argument");
    if (misaligned4(dy) || misaligned4(y) || misaligned4(norm) || misaligned4(dx))
        return fail(OCM_EINVAL, "l2_normalize_backward: a pointer is not 4-byte aligned");
    if (int rc = rows_ok("l2_normalize_backward", rows, dim)) return rc;
    l2norm_bwd_kernel<<<dim3((unsigned)rows), dim3(DN_THREADS), 0, (hipStream_t)stream>>>(dy, y, norm, dx, dim);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_weight_norm(const float *v, const float *g, float *w, float *norm, int32_t N, int32_t K, void *stream) {
    if (!v || !g || !w || !norm) return fail(OCM_EINVAL, "weight_norm: null argument");
    if (misaligned4(v) || misaligned4(g) || misaligned4(w) || misaligned4(norm))
        return fail(OCM_EINVAL, "weight_norm: a pointer is not 4-byte aligned");
    if (int rc = rows_ok("weight_norm", N, K)) return rc;
    wnorm_kernel<<<dim3((unsigned)N), dim3(DN_THREADS), 0, (hipStream_t)stream>>>(v, g, w, norm, K);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_weight_norm_backward(const float *dw, const float *v, const float *g, const float *norm, float *dg, float *dv,
                                           int32_t N, int32_t K, void *stream) {
    if (!dw || !v || !g || !norm) return fail(OCM_EINVAL, "weight_norm_backward: null argument");
    if (!dg && !dv) return fail(OCM_EINVAL, "weight_norm_backward: both outputs are null");
    if (misaligned4(dw) || misaligned4(v) || misaligned4(g) || misaligned4(norm) || misaligned4(dg) || misaligned4(dv))
        return fail(OCM_EINVAL, "weight_norm_backward: a pointer is not 4-byte aligned");
    if (int rc = rows_ok("weight_norm_backward", N, K)) return rc;
    wnorm_bwd_kernel<<<dim3((unsigned)N), dim3(DN_THREADS), 0, (hipStream_t)stream>>>(dw, v, g, norm, dg, dv, K);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

// [dots: B x slices x 2 x V float64]; 0 for a shape the operator refuses
extern "C" size_t ocm_dino_loss_workspace_bytes(int32_t B, int32_t V, int32_t K) {
    if (B < 1 || V < 2 || K < 1) return 0;
    return (size_t)B * loss_slices(K) * 2 * V * sizeof(double);
}

extern "C" int ocm_op_dino_loss(const float *student, const float *teacher, const float *center, float student_temp,
                                float teacher_temp, int32_t B, int32_t V, int32_t K, float *loss_out, double *row_stats,
                                void *workspace, size_t workspace_bytes, void *stream) {
    if (!student || !teacher || !center || !loss_out || !row_stats) return fail(OCM_EINVAL, "dino_loss: null argument");
    if (int rc = loss_shape_ok("dino_loss", B, V, K, student_temp, teacher_temp)) return rc;
    if (misaligned4(student) || misaligned4(teacher) || misaligned4(center) || misaligned4(loss_out) || ((uintptr_t)row_stats & 7))
        return fail(OCM_EINVAL, "dino_loss: a pointer is not aligned to its element");
    const size_t need = ocm_dino_loss_workspace_bytes(B, V, K);
    if (!workspace || workspace_bytes < need) return fail(OCM_EINVAL, "dino_loss workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace & 7) return fail(OCM_EINVAL, "dino_loss workspace: not 8-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int slices = loss_slices(K);
    loss_stats_kernel<<<dim3((unsigned)(B * (V + 2))), dim3(DN_THREADS), 0, st>>>(student, teacher, center, student_temp, teacher_temp,
                                                                                B * V, K, row_stats);
    HIP_TRY(hipGetLastError());
    loss_dots_kernel<<<dim3((unsigned)B, (unsigned)slices), dim3(DN_THREADS), 0, st>>>(student, teacher, center, row_stats, teacher_temp,
                                                                                      B, V, K, (double *)workspace);
    HIP_TRY(hipGetLastError());
    loss_finish_kernel<<<dim3(1), dim3(DN_THREADS), 0, st>>>(row_stats, (const double *)workspace, student_temp, B, V, slices, loss_out);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_dino_loss_backward(const float *grad_loss, const float *student, const float *teacher, const float *center,
                                         float student_temp, float teacher_temp, int32_t B, int32_t V, int32_t K,
                                         const double *row_stats, float *dstudent, void *stream) {
    if (!grad_loss || !student || !teacher || !center || !row_stats || !dstudent)
        return fail(OCM_EINVAL, "dino_loss_backward: null argument");
    if (int rc = loss_shape_ok("dino_loss_backward", B, V, K, student_temp, teacher_temp)) return rc;
    if (misaligned4(grad_loss) || misaligned4(student) || misaligned4(teacher) || misaligned4(center) || misaligned4(dstudent) ||
        ((uintptr_t)row_stats & 7))
        return fail(OCM_EINVAL, "dino_loss_backward: a pointer is not aligned to its element");
    loss_bwd_kernel<<<dim3((unsigned)B, (unsigned)loss_slices(K)), dim3(DN_THREADS), 0, (hipStream_t)stream>>>(
        grad_loss, student, teacher, center, row_stats, student_temp, teacher_temp, B, V, K, dstudent);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_dino_center(int32_t mode, const float *teacher, int64_t rows, int32_t K, float *batch_sum, float *center,
                                  double count, double momentum, void *stream) {
    if (mode != OCM_DINO_CENTER_SUM && mode != OCM_DINO_CENTER_UPDATE) return fail(OCM_EINVAL, "dino_center: unknown mode %d", mode);
    if (K < 1) return fail(OCM_EINVAL, "dino_center: K = %d (>= 1)", K);
    if (!batch_sum || misaligned4(batch_sum)) return fail(OCM_EINVAL, "dino_center: null or misaligned batch_sum");
    const hipStream_t st = (hipStream_t)stream;
    const int quads = (K + 3) / 4;
    if (mode == OCM_DINO_CENTER_SUM) {
        if (!teacher || misaligned4(teacher)) return fail(OCM_EINVAL, "dino_center: null or misaligned teacher logits");
        if (rows < 1) return fail(OCM_EINVAL, "dino_center: rows = %lld (>= 1)", (long long)rows);
        center_sum_kernel<<<dim3((unsigned)((quads + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0, st>>>(teacher, rows, K,
                                                                                                              batch_sum);
    } else {
        if (!center || misaligned4(center)) return fail(OCM_EINVAL, "dino_center: null or misaligned center");
        if (!(count >= 1.0) || !std::isfinite(count) || !std::isfinite(momentum))
            return fail(OCM_EINVAL, "dino_center: count = %g (>= 1), momentum = %g (finite)", count, momentum);
        center_update_kernel<<<dim3((unsigned)((quads + DN_THREADS - 1) / DN_THREADS)), dim3(DN_THREADS), 0, st>>>(
            center, batch_sum, K, (float)count, (float)momentum, (float)(1.0 - momentum));
    }
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
