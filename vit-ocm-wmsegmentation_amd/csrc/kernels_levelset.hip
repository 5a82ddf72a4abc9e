// kernels_levelset.hip — skimage.segmentation.chan_vese (0.19.x) as the reference's utils.py:199-225 calls it (eval.py's
// "chan-vese" / "chan-vese_ours" methods), for a batch of independent level sets on device. State and arithmetic are float64,
// as skimage's are for a uint8 image; every term of an iteration reads the old phi (Jacobi, ping-pong buffers).
//
// One stream-ordered launch per iteration and no host synchronisation:
//   cv_prologue_kernel  partial sums of phi_0 (count and sum of the image inside phi > 0, sum outside), stop[b] = -1
//   cv_step_kernel      launch k = 1 .. max_num_iter. Every workgroup of an image adds up the partials launch k - 1 wrote, in
//                       one fixed order, and derives c1, c2 and phivar_(k-1) = sqrt(sum (phi_(k-1) - phi_(k-2))^2 / (h w)) from
//                       them: all workgroups of an image hold the same bits and take the same decision. The image has stopped
//                       when stop[b] >= 0 or (k > 1 and not phivar_(k-1) > tol); then the workgroup returns at once (workgroup 0
//                       records stop[b] = k - 1 first). Otherwise it writes phi_k for its tiles into buffer k & 1 and its own
//                       partial sums of phi_k into slot k & 1.
//   cv_epilogue_kernel  iters[b] = stop[b] >= 0 ? stop[b] : max_num_iter; phi and mask from buffer iters[b] & 1
// Buffer 0 is the caller's phi, buffer 1 lives in the workspace. An image that has stopped is not written again, so its final
// level set waits in the buffer of its own parity whatever the other images of the batch go on doing.
// No workgroup waits for another one: what must be complete before the next step is separated from it by a kernel boundary. No
// floating-point atomics: a partial is one slot per workgroup, and the sums are taken in a fixed order (per thread in tile
// order, xor butterfly over the wave, the four waves in order, the workgroups' slots by the same tree), so equal inputs give
// equal bits.
// The 4-neighbourhood is read straight from global memory (L1 / L2): a variant with an LDS halo tile measured 5 % slower on 16
// level sets of 384 x 384, where the float64 divisions and square roots, not the neighbour reads, fill the time.
#include <cfloat>
#include <cmath>

#include "host_common.h"

#define fail ocm_fail

// the expression of skimage's _cv_calculate_variation as numpy evaluates it: separate IEEE operations
#pragma clang fp contract(off)

namespace {

constexpr int CT = 32;            // tile side: 256 threads, four rows of the tile apart by 8 per thread
constexpr int CV_THREADS = 256;
constexpr int CV_MAX_GROUPS = 256;  // workgroups (= partial slots) per image: one slot per thread of the consumer

struct alignas(32) CvPart {
    double cnt, sum_in, sum_out, ssd;  // pixels with phi > 0, sum of the image over them, over the others, sum (new - old)^2
};

struct CvParams {
    double mu, lambda1, lambda2, tol, dt;
};

// Sum over the workgroup, the same bits in every thread. s_wave: 4 slots.
__device__ __forceinline__ CvPart block_sum(CvPart v, CvPart *s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        v.cnt += __shfl_xor(v.cnt, o, 64);
        v.sum_in += __shfl_xor(v.sum_in, o, 64);
        v.sum_out += __shfl_xor(v.sum_out, o, 64);
        v.ssd += __shfl_xor(v.ssd, o, 64);
    }
    __syncthreads();  // an earlier use of s_wave has been read by everyone
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    CvPart r = s_wave[0];
#pragma unroll
    for (int k = 1; k < CV_THREADS / 64; ++k) {
        r.cnt += s_wave[k].cnt;
        r.sum_in += s_wave[k].sum_in;
        r.sum_out += s_wave[k].sum_out;
        r.ssd += s_wave[k].ssd;
    }
    return r;
}

__device__ __forceinline__ void tally(CvPart &acc, double phi_new, double img) {
    if (phi_new > 0.0) {
        acc.cnt += 1.0;
        acc.sum_in += img;
    } else {
        acc.sum_out += img;
    }
}

// grid (groups, batch)
__global__ __launch_bounds__(CV_THREADS) void cv_prologue_kernel(const double *__restrict__ image, const double *__restrict__ phi,
                                                                 CvPart *__restrict__ part, int *__restrict__ stop, int h, int w,
                                                                 int tiles_x, int ntiles) {
    __shared__ CvPart s_wave[CV_THREADS / 64];
    const int b = blockIdx.y;
    const size_t base = (size_t)b * h * w;
    const int lx = threadIdx.x & (CT - 1), ly = threadIdx.x / CT;
    CvPart acc = {0.0, 0.0, 0.0, 0.0};
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int x = (t % tiles_x) * CT + lx, y0 = (t / tiles_x) * CT + ly;
        if (x >= w) continue;
#pragma unroll
        for (int k = 0; k < CT * CT / CV_THREADS; ++k) {
            const int y = y0 + k * (CV_THREADS / CT);
            if (y >= h) break;
            const size_t i = base + (size_t)y * w + x;
            tally(acc, phi[i], image[i]);
        }
    }
    acc = block_sum(acc, s_wave);
    if (threadIdx.x == 0) {
        part[(size_t)b * gridDim.x + blockIdx.x] = acc;
        if (blockIdx.x == 0) stop[b] = -1;
    }
}

// grid (groups, batch): phi_k (dst) from phi_(k-1) (src)
__global__ __launch_bounds__(CV_THREADS) void cv_step_kernel(const double *__restrict__ image, const double *__restrict__ src,
                                                             double *__restrict__ dst, const CvPart *__restrict__ part_in,
                                                             CvPart *__restrict__ part_out, int *stop, int h, int w, int tiles_x,
                                                             int ntiles, int k, CvParams p) {
    __shared__ CvPart s_wave[CV_THREADS / 64];
    __shared__ int s_stop;
    const int b = blockIdx.y;
    // workgroup 0 of this launch may be storing k - 1 here right now: a workgroup that reads the old -1 reaches the same
    // decision from the partials below. One thread reads, so that the whole workgroup acts on one value.
    if (threadIdx.x == 0) s_stop = __hip_atomic_load(stop + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_stop >= 0) return;
    CvPart tot = {0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < gridDim.x) tot = part_in[(size_t)b * gridDim.x + threadIdx.x];
    tot = block_sum(tot, s_wave);
    const double n = (double)h * (double)w;
    if (k > 1) {
        const double phivar = sqrt(tot.ssd / n);
        if (!(phivar > p.tol)) {  // the loop condition `phivar > tol` fails (a NaN ends the loop as well)
            if (blockIdx.x == 0 && threadIdx.x == 0)
                __hip_atomic_store(stop + b, k - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    const double cnt_out = n - tot.cnt;
    const double c1 = tot.cnt != 0.0 ? tot.sum_in / tot.cnt : tot.sum_in;
    const double c2 = cnt_out != 0.0 ? tot.sum_out / cnt_out : tot.sum_out;
    const double eta = 1e-16;
    const double mudt = p.mu * p.dt;

    const size_t base = (size_t)b * h * w;
    const int lx = threadIdx.x & (CT - 1), ly = threadIdx.x / CT;
    CvPart acc = {0.0, 0.0, 0.0, 0.0};
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int x = (t % tiles_x) * CT + lx, y0 = (t / tiles_x) * CT + ly;
        if (x >= w) continue;
        const int xe = min(x + 1, w - 1), xw = max(x - 1, 0);
#pragma unroll
        for (int kk = 0; kk < CT * CT / CV_THREADS; ++kk) {
            const int y = y0 + kk * (CV_THREADS / CT);
            if (y >= h) break;
            const double *row = src + base + (size_t)y * w;
            const double c = row[x], e = row[xe], wv = row[xw];
            const double s = src[base + (size_t)min(y + 1, h - 1) * w + x];
            const double nv = src[base + (size_t)max(y - 1, 0) * w + x];
            const double xp = e - c, xn = c - wv, x0 = (e - wv) / 2.0;
            const double yp = s - c, yn = c - nv, y0d = (s - nv) / 2.0;
            const double C1 = 1.0 / sqrt(eta + xp * xp + y0d * y0d);
            const double C2 = 1.0 / sqrt(eta + xn * xn + y0d * y0d);
            const double C3 = 1.0 / sqrt(eta + x0 * x0 + yp * yp);
            const double C4 = 1.0 / sqrt(eta + x0 * x0 + yn * yn);
            const double K = e * C1 + wv * C2 + s * C3 + nv * C4;
            const double img = image[base + (size_t)y * w + x];
            const double d1 = img - c1, d2 = img - c2;
            const double D = -p.lambda1 * (d1 * d1) + p.lambda2 * (d2 * d2);
            const double delta = 1.0 / (1.0 + c * c);
            const double dd = p.dt * delta;
            const double num = c + dd * (p.mu * K + D);
            const double den = 1.0 + mudt * delta * (C1 + C2 + C3 + C4);
            const double nw = num / den;
            dst[base + (size_t)y * w + x] = nw;
            tally(acc, nw, img);
            const double df = nw - c;
            acc.ssd += df * df;
        }
    }
    acc = block_sum(acc, s_wave);
    if (threadIdx.x == 0) part_out[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

// grid (blocks, batch)
__global__ __launch_bounds__(CV_THREADS) void cv_epilogue_kernel(double *__restrict__ phi, const double *__restrict__ phi1,
                                                                 const int *__restrict__ stop, uint8_t *__restrict__ mask,
                                                                 int *__restrict__ iters, int n, int max_num_iter) {
    const int b = blockIdx.y;
    const int st = stop[b];
    const int it = st >= 0 ? st : max_num_iter;
    const size_t base = (size_t)b * n;
    const bool odd = it & 1;
    for (int i = blockIdx.x * CV_THREADS + threadIdx.x; i < n; i += gridDim.x * CV_THREADS) {
        double v;
        if (odd) {
            v = phi1[base + i];
            phi[base + i] = v;
        } else {
            v = phi[base + i];
        }
        mask[base + i] = v > 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) iters[b] = it;
}

constexpr int MAX_SIDE = 32768;
constexpr int64_t MAX_PIXELS = (int64_t)1 << 30;
constexpr int MAX_ITER = 10000;

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

bool shape_ok(int32_t batch, int32_t h, int32_t w) {
    return batch >= 1 && batch <= 65535 && h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE && (int64_t)h * w <= MAX_PIXELS;
}

int cv_tiles(int32_t h, int32_t w) { return ((h + CT - 1) / CT) * ((w + CT - 1) / CT); }  // at most 2^20
int cv_groups(int32_t h, int32_t w) { return cv_tiles(h, w) < CV_MAX_GROUPS ? cv_tiles(h, w) : CV_MAX_GROUPS; }

}  // namespace

extern "C" int32_t ocm_chan_vese_tile(void) { return CT; }

// [phi buffer 1: batch h w doubles][partials: 2 slots x batch x groups][stop: batch ints]
extern "C" size_t ocm_chan_vese_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    if (!shape_ok(batch, h, w)) return 0;
    return align256((size_t)batch * h * w * sizeof(double)) + align256(2 * (size_t)batch * cv_groups(h, w) * sizeof(CvPart)) +
           align256((size_t)batch * sizeof(int));
}

extern "C" int ocm_op_chan_vese(const double *image, double *phi, uint8_t *mask, int32_t *iters, int32_t batch, int32_t h,
                                int32_t w, double mu, double lambda1, double lambda2, double tol, int32_t max_num_iter, double dt,
                                void *workspace, size_t workspace_bytes, void *stream) {
    if (!image || !phi || !mask || !iters) return fail(OCM_EINVAL, "null argument");
    if (batch < 1 || batch > 65535) return fail(OCM_EINVAL, "chan_vese: batch = %d (1..65535)", batch);
    if (!shape_ok(batch, h, w))
        return fail(OCM_EINVAL, "chan_vese: image %d x %d (sides 1..%d, at most 2^30 pixels)", h, w, MAX_SIDE);
    if (max_num_iter < 0 || max_num_iter > MAX_ITER)
        return fail(OCM_EINVAL, "chan_vese: max_num_iter = %d (0..%d)", max_num_iter, MAX_ITER);
    if (!std::isfinite(mu) || mu < 0.0) return fail(OCM_EINVAL, "chan_vese: mu = %g (finite, >= 0)", mu);
    if (!std::isfinite(dt) || dt < 0.0) return fail(OCM_EINVAL, "chan_vese: dt = %g (finite, >= 0)", dt);
    if (!std::isfinite(tol) || tol < 0.0) return fail(OCM_EINVAL, "chan_vese: tol = %g (finite, >= 0)", tol);
    if (!std::isfinite(lambda1) || !std::isfinite(lambda2))
        return fail(OCM_EINVAL, "chan_vese: lambda1 = %g, lambda2 = %g (finite)", lambda1, lambda2);
    const size_t need = ocm_chan_vese_workspace_bytes(batch, h, w);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "chan_vese workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const int n = h * w, tiles_x = (w + CT - 1) / CT, ntiles = cv_tiles(h, w), groups = cv_groups(h, w);
    char *ws = (char *)workspace;
    double *buf[2] = {phi, (double *)ws};
    ws += align256((size_t)batch * n * sizeof(double));
    const size_t slot = (size_t)batch * groups;
    CvPart *part[2] = {(CvPart *)ws, (CvPart *)ws + slot};
    ws += align256(2 * slot * sizeof(CvPart));
    int *stop = (int *)ws;
    const dim3 grid(groups, batch), block(CV_THREADS);
    const CvParams p = {mu, lambda1, lambda2, tol, dt};
    cv_prologue_kernel<<<grid, block, 0, s>>>(image, phi, part[0], stop, h, w, tiles_x, ntiles);
    HIP_TRY(hipGetLastError());
    for (int k = 1; k <= max_num_iter; ++k)
        cv_step_kernel<<<grid, block, 0, s>>>(image, buf[(k - 1) & 1], buf[k & 1], part[(k - 1) & 1], part[k & 1], stop, h, w,
                                              tiles_x, ntiles, k, p);
    const unsigned eg = (unsigned)(((size_t)n + CV_THREADS - 1) / CV_THREADS);
    cv_epilogue_kernel<<<dim3(eg < 1024 ? eg : 1024, batch), block, 0, s>>>(phi, buf[1], stop, mask, iters, n, max_num_iter);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
