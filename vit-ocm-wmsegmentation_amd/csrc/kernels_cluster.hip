// kernels_cluster.hip — the k-means feature clustering of eval.py's `k-means_feature_clustering` method (reference
// eval.py:185-202, utils.py:171-197) on device: the row-wise work of sklearn's KMeans(n_clusters=2, n_init=10) over the
// [S*S][D] key-feature matrix. The host (cluster.py) replays sklearn's control flow; every pass over X runs here:
//   kfeat_kernel              keys of the patch tokens of one image, bilinearly upsampled (align_corners=False) to S x S
//   zs_pass_kernel<MODE>      per-channel fp64 partial sums over a fixed row split: mean, (x - mean)^2, the z-score write
//   zs_finish_kernel<MODE>    (with its column sums), sklearn's centring write (with its column sums and squares)
//   kdist_kernel<CPL, K>      ||x - c||^2 in fp64 to one or two candidate centres, optionally min'ed with closest_dist_sq
//   lloyd_kernel<CPL, ASSIGN> argmin over two centres (ties: the lower index), labels, per-block fp64 cluster sums /
//                             counts / inertia / changed flag; lloyd_cols_kernel and lloyd_info_kernel add the per-block
//                             partials in block order: new centres, squared shifts, counts, inertia
// No atomics: every partial has one writer and is summed in a fixed order, so a rerun gives the same bits.
// X rows are read as 16-byte vectors. In kdist / lloyd a row belongs to a group of 32 lanes (two rows per wave in flight,
// each wave walking a contiguous run of rows); lane l of a group holds float4 chunks l, l + 32, ... of the row and of the
// centres (CPL chunks per lane, in registers), and the group's fp64 partial distances meet in a xor butterfly.
#include "host_common.h"
#include "launch.h"

#define fail ocm_fail

// torch's CPU F.interpolate and numpy evaluate with separate IEEE multiplies and adds: no fused multiply-add contraction
// here (the same rule as kernels_post.hip), so that the roundings happen where theirs do.
#pragma clang fp contract(off)

namespace {

constexpr int KM_LANES = 32;       // lanes per row in kdist / lloyd: two rows per wave in flight
constexpr int KM_MAX_DIM = 1024;   // 32 lanes x 8 float4 chunks
constexpr int LLOYD_THREADS = 256; // 4 waves
constexpr int LLOYD_WAVES = LLOYD_THREADS / 64;
constexpr int LLOYD_SCAL = 4;      // per-block scalars: count0, count1, inertia, changed

// ---- feature map ---------------------------------------------------------------------------------------------------------
// X[(y*S + x)][h*hd + j] = bilinear(k[image][h][1 + token][j]) from the g x g token grid, torch's align_corners=False rule:
// src = max(fma(g / S, dst + 0.5, -0.5), 0), i0 = floor(src) (at most g - 1), i1 = i0 + (i0 < g - 1), l1 = src - i0, l0 = 1 - l1.
__global__ __launch_bounds__(256) void kfeat_kernel(const float *__restrict__ qkv, float *__restrict__ X, int B, int H, int N,
                                                    int hd, int image, int g, int S, float scale) {
    const int D4 = H * hd / 4;
    const int64_t total = (int64_t)S * S * D4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % D4);
        const int64_t pix = i / D4;
        const int x = (int)(pix % S), y = (int)(pix / S);
        const int c = c4 * 4, h = c / hd, j = c % hd;
        // torch's CPU build contracts scale * (dst + 0.5) - 0.5 into one fma (measured against F.interpolate)
        float sy = fmaf(scale, (float)y + 0.5f, -0.5f), sx = fmaf(scale, (float)x + 0.5f, -0.5f);
        sy = sy < 0.f ? 0.f : sy;
        sx = sx < 0.f ? 0.f : sx;
        const int y0 = min((int)sy, g - 1), x0 = min((int)sx, g - 1);
        const int y1 = y0 + (y0 < g - 1 ? 1 : 0), x1 = x0 + (x0 < g - 1 ? 1 : 0);
        const float ly1 = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx1 = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
        const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        const float w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1;
        const float *kb = qkv + ((size_t)(B + image) * H + h) * (size_t)N * hd + j;  // qkv[1][image][h][.][j]
        const f32x4 v00 = *(const f32x4 *)(kb + (size_t)(1 + y0 * g + x0) * hd);
        const f32x4 v01 = *(const f32x4 *)(kb + (size_t)(1 + y0 * g + x1) * hd);
        const f32x4 v10 = *(const f32x4 *)(kb + (size_t)(1 + y1 * g + x0) * hd);
        const f32x4 v11 = *(const f32x4 *)(kb + (size_t)(1 + y1 * g + x1) * hd);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = ((v00[e] * w00 + v01[e] * w01) + v10[e] * w10) + v11[e] * w11;
        *(f32x4 *)(X + (size_t)pix * (H * hd) + c) = o;
    }
}

// ---- column statistics and z-score -----------------------------------------------------------------------------------------
// Rows are cut into R chunks (a function of the row count alone); a workgroup covers 256 channels (64 lanes x float4) of one
// chunk with 4 row groups (rows strided by 4) combined in LDS in group order, and writes part[k][chunk][c]. stats [4][D] fp64:
//   [0] mean   [1] unbiased std (torch.std)   [2] sklearn's fp32 centring mean X.mean(axis=0) (as fp64)   [3] np.var of
//   the final X (biased).
//   MODE 0: sum x              MODE 1: sum (x - mean)^2
//   MODE 2: z = (x - (float)mean) / (float)std written in place, sum z
//   MODE 3: v = z - (float)stats[2] written in place, sum v and sum v^2
int zs_chunks(int64_t rows) { return (int)std::min<int64_t>((rows + 255) / 256, 512); }

template <int MODE>
__global__ __launch_bounds__(256) void zs_pass_kernel(float *__restrict__ X, const double *__restrict__ stats,
                                                      double *__restrict__ part, int64_t rows, int D, int64_t chunk) {
    __shared__ double red[2][4][64][4];
    const int lane = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * 4, R = gridDim.y;
    const bool active = c < D;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = std::min<int64_t>(rows, r0 + chunk);
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        double mu[4];
        float pa[4], pb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mu[e] = MODE == 1 ? stats[c + e] : 0.0;
            pa[e] = MODE == 2 ? (float)stats[c + e] : MODE == 3 ? (float)stats[2 * D + c + e] : 0.f;
            pb[e] = MODE == 2 ? (float)stats[D + c + e] : 1.f;
        }
        for (int64_t m = r0 + rg; m < r1; m += 4) {
            f32x4 *p = (f32x4 *)(X + (size_t)m * D + c);
            f32x4 v = *p;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (MODE == 0) {
                    s0[e] += (double)v[e];
                } else if (MODE == 1) {
                    const double d = (double)v[e] - mu[e];
                    s0[e] += d * d;
                } else if (MODE == 2) {
                    v[e] = (v[e] - pa[e]) / pb[e];
                    s0[e] += (double)v[e];
                } else {
                    v[e] = v[e] - pa[e];
                    s0[e] += (double)v[e];
                    s1[e] += (double)v[e] * (double)v[e];
                }
            }
            if (MODE >= 2) *p = v;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[0][rg][lane][e] = s0[e];
        red[1][rg][lane][e] = s1[e];
    }
    __syncthreads();
    if (rg == 0 && active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            part[(size_t)blockIdx.y * D + c + e] =
                ((red[0][0][lane][e] + red[0][1][lane][e]) + red[0][2][lane][e]) + red[0][3][lane][e];
            if (MODE == 3)
                part[((size_t)R + blockIdx.y) * D + c + e] =
                    ((red[1][0][lane][e] + red[1][1][lane][e]) + red[1][2][lane][e]) + red[1][3][lane][e];
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void zs_finish_kernel(const double *__restrict__ part, int R, int D, int64_t rows,
                                                        double *__restrict__ stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    double s0 = 0.0, s1 = 0.0;
    for (int r = 0; r < R; ++r) s0 += part[(size_t)r * D + c];
    const double n = (double)rows;
    if (MODE == 0) {
        stats[c] = s0 / n;
    } else if (MODE == 1) {
        stats[D + c] = sqrt(s0 / (n - 1.0));
    } else if (MODE == 2) {
        stats[2 * D + c] = (double)(float)(s0 / n);
    } else {
        for (int r = 0; r < R; ++r) s1 += part[((size_t)R + r) * D + c];
        const double m = s0 / n;
        stats[3 * D + c] = s1 / n - m * m;
    }
}

template <int MODE>
hipError_t launch_zs(float *X, double *stats, double *part, int64_t rows, int D, hipStream_t s) {
    const int R = zs_chunks(rows);
    const int64_t chunk = (rows + R - 1) / R;
    zs_pass_kernel<MODE><<<dim3((D / 4 + 63) / 64, R), dim3(256), 0, s>>>(X, stats, part, rows, D, chunk);
    zs_finish_kernel<MODE><<<dim3((D + 255) / 256), dim3(256), 0, s>>>(part, R, D, rows, stats);
    return hipGetLastError();
}

// ---- row distances ---------------------------------------------------------------------------------------------------------
// Rows [w * per, (w + 1) * per) belong to wave w; the two lane groups of a wave take rows r and r + 1.
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = KM_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int CPL>
__device__ __forceinline__ void load_chunks(const float *__restrict__ row, int D4, int l, f32x4 (&reg)[CPL]) {
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int ch = l + KM_LANES * i;
        reg[i] = ch < D4 ? ((const f32x4 *)row)[ch] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int CPL>
__device__ __forceinline__ double sq_dist(const f32x4 (&x)[CPL], const f32x4 (&c)[CPL]) {
    double acc = 0.0;  // zero-filled chunks past D add exact zeros
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = (double)x[i][e] - (double)c[i][e];
            acc += d * d;
        }
    return acc;
}

int kdist_blocks(int64_t rows) { return (int)std::min<int64_t>((rows + 255) / 256, 1024); }

template <int CPL, int K>
__global__ __launch_bounds__(256) void kdist_kernel(const float *__restrict__ X, int64_t rows, int D,
                                                    const float *__restrict__ cand, const double *__restrict__ closest,
                                                    double *__restrict__ dist, int64_t per) {
    const int D4 = D / 4, lane = threadIdx.x & 63, grp = lane / KM_LANES, l = lane % KM_LANES;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r0 = wave * per, r1 = std::min<int64_t>(rows, r0 + per);
    f32x4 c[K][CPL];
#pragma unroll
    for (int k = 0; k < K; ++k) load_chunks<CPL>(cand + (size_t)k * D, D4, l, c[k]);
    for (int64_t r = r0 + grp; r < r1; r += 64 / KM_LANES) {
        f32x4 x[CPL];
        load_chunks<CPL>(X + (size_t)r * D, D4, l, x);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double d = group_sum(sq_dist<CPL>(x, c[k]));
            if (closest) d = fmin(closest[r], d);
            if (l == 0) dist[(size_t)k * rows + r] = d;
        }
    }
}

// ---- Lloyd step ------------------------------------------------------------------------------------------------------------
// Per block: [2][D] fp64 cluster sums (the 2 lane groups of a wave combined by xor 32, the waves added in wave order in
// LDS) and 4 scalars, written to the workspace at the block's index. ASSIGN: labels, counts, inertia and changed only.
int lloyd_blocks(int64_t rows) { return (int)std::min<int64_t>((rows + 127) / 128, 1024); }

template <int CPL, bool ASSIGN>
__global__ __launch_bounds__(LLOYD_THREADS) void lloyd_kernel(const float *__restrict__ X, int64_t rows, int D,
                                                              const float *__restrict__ centers,
                                                              const int32_t *__restrict__ labels_old,
                                                              int32_t *__restrict__ labels, double *__restrict__ part,
                                                              double *__restrict__ part_scal, int64_t per) {
    __shared__ double lsum[ASSIGN ? 1 : 2 * KM_MAX_DIM];
    __shared__ double lscal[LLOYD_WAVES][LLOYD_SCAL];
    const int D4 = D / 4, lane = threadIdx.x & 63, w = threadIdx.x >> 6, grp = lane / KM_LANES, l = lane % KM_LANES;
    const int64_t wave = (int64_t)blockIdx.x * LLOYD_WAVES + w;
    const int64_t r0 = wave * per, r1 = std::min<int64_t>(rows, r0 + per);
    f32x4 c0[CPL], c1[CPL];
    load_chunks<CPL>(centers, D4, l, c0);
    load_chunks<CPL>(centers + D, D4, l, c1);
    double s0[CPL][4], s1[CPL][4];
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) s0[i][e] = s1[i][e] = 0.0;
    double n1 = 0.0, n0 = 0.0, inertia = 0.0, changed = 0.0;
    for (int64_t r = r0 + grp; r < r1; r += 64 / KM_LANES) {
        f32x4 x[CPL];
        load_chunks<CPL>(X + (size_t)r * D, D4, l, x);
        const double d0 = group_sum(sq_dist<CPL>(x, c0)), d1 = group_sum(sq_dist<CPL>(x, c1));
        const int lab = d1 < d0 ? 1 : 0;  // argmin, the lower index on a tie
        if (l == 0) labels[r] = lab;
        const bool ch = labels_old ? labels_old[r] != lab : true;
        changed = ch ? 1.0 : changed;
        n1 += (double)lab;
        n0 += (double)(1 - lab);
        inertia += lab ? d1 : d0;
        if (!ASSIGN) {
#pragma unroll
            for (int i = 0; i < CPL; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double v = (double)x[i][e];
                    s0[i][e] += lab ? 0.0 : v;
                    s1[i][e] += lab ? v : 0.0;
                }
        }
    }
    // the wave's two lane groups: g0 + g1 on every lane (xor partners add the same two values)
#pragma unroll
    for (int m = KM_LANES; m < 64; m <<= 1) {
        n0 += __shfl_xor(n0, m, 64);
        n1 += __shfl_xor(n1, m, 64);
        inertia += __shfl_xor(inertia, m, 64);
        changed = fmax(changed, __shfl_xor(changed, m, 64));
        if (!ASSIGN) {
#pragma unroll
            for (int i = 0; i < CPL; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s0[i][e] += __shfl_xor(s0[i][e], m, 64);
                    s1[i][e] += __shfl_xor(s1[i][e], m, 64);
                }
        }
    }
    if (lane == 0) {
        lscal[w][0] = n0;
        lscal[w][1] = n1;
        lscal[w][2] = inertia;
        lscal[w][3] = changed;
    }
    if (!ASSIGN) {
        // waves added in wave order: ((w0 + w1) + w2) + ...
        for (int ww = 0; ww < LLOYD_WAVES; ++ww) {
            if (w == ww && lane < KM_LANES) {
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const int ch = l + KM_LANES * i;
                    if (ch < D4) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int cc = ch * 4 + e;
                            lsum[cc] = ww == 0 ? s0[i][e] : lsum[cc] + s0[i][e];
                            lsum[D + cc] = ww == 0 ? s1[i][e] : lsum[D + cc] + s1[i][e];
                        }
                    }
                }
            }
            __syncthreads();
        }
        for (int cc = threadIdx.x; cc < 2 * D; cc += LLOYD_THREADS) part[(size_t)blockIdx.x * 2 * D + cc] = lsum[cc];
    } else {
        __syncthreads();
    }
    if (threadIdx.x < LLOYD_SCAL) {
        double v = lscal[0][threadIdx.x];
        for (int ww = 1; ww < LLOYD_WAVES; ++ww)
            v = threadIdx.x == 3 ? fmax(v, lscal[ww][threadIdx.x]) : v + lscal[ww][threadIdx.x];
        part_scal[(size_t)blockIdx.x * LLOYD_SCAL + threadIdx.x] = v;
    }
}

// sums[j][c] = sum over blocks (in block order) of part[b][j][c]; centers_new[j][c] = (float)(sums / count_j).
// 16 groups of 16 columns per workgroup, each group a contiguous sixteenth of the blocks, the sixteenths added in order in LDS.
__global__ __launch_bounds__(256) void lloyd_cols_kernel(const double *__restrict__ part, const double *__restrict__ part_scal,
                                                         int NB, int D, double *__restrict__ sums,
                                                         float *__restrict__ centers_new) {
    __shared__ double red[16][16];
    const int t = threadIdx.x & 15, gq = threadIdx.x >> 4;
    const int cc = blockIdx.x * 16 + t;
    const int per = (NB + 15) / 16, b0 = gq * per, b1 = min(NB, b0 + per);
    double s = 0.0;
    if (cc < 2 * D)
        for (int b = b0; b < b1; ++b) s += part[(size_t)b * 2 * D + cc];
    red[gq][t] = s;
    __syncthreads();
    if (gq == 0 && cc < 2 * D) {
        double v = red[0][t];
        for (int q = 1; q < 16; ++q) v += red[q][t];
        const int j = cc >= D ? 1 : 0;
        double n = 0.0;
        for (int b = 0; b < NB; ++b) n += part_scal[(size_t)b * LLOYD_SCAL + j];
        if (sums) sums[cc] = v;
        centers_new[cc] = n > 0.0 ? (float)(v / n) : 0.f;
    }
}

// info: [0] inertia against `centers`, [1] count0, [2] count1, [3] / [4] ||new - old||^2 per cluster (0 in assign mode),
// [5] 1 when a label differs from labels_old (always 1 without labels_old), [6] number of empty clusters.
__global__ __launch_bounds__(256) void lloyd_info_kernel(const double *__restrict__ part_scal, int NB, int D,
                                                         const float *__restrict__ centers,
                                                         const float *__restrict__ centers_new, double *__restrict__ info) {
    __shared__ double red[2][256];
    double sh[2] = {0.0, 0.0};
    if (centers_new)
        for (int c = threadIdx.x; c < D; c += 256)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double d = (double)centers_new[j * D + c] - (double)centers[j * D + c];
                sh[j] += d * d;
            }
    red[0][threadIdx.x] = sh[0];
    red[1][threadIdx.x] = sh[1];
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (threadIdx.x < m) {
            red[0][threadIdx.x] += red[0][threadIdx.x + m];
            red[1][threadIdx.x] += red[1][threadIdx.x + m];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double n0 = 0.0, n1 = 0.0, in = 0.0, ch = 0.0;
        for (int b = 0; b < NB; ++b) {
            n0 += part_scal[(size_t)b * LLOYD_SCAL + 0];
            n1 += part_scal[(size_t)b * LLOYD_SCAL + 1];
            in += part_scal[(size_t)b * LLOYD_SCAL + 2];
            ch = fmax(ch, part_scal[(size_t)b * LLOYD_SCAL + 3]);
        }
        info[0] = in;
        info[1] = n0;
        info[2] = n1;
        info[3] = red[0][0];
        info[4] = red[1][0];
        info[5] = ch;
        info[6] = (double)((n0 == 0.0) + (n1 == 0.0));
    }
}

int cpl_for(int D) {  // float4 chunks per lane: the smallest supported count covering D / 4 over 32 lanes
    const int need = (D / 4 + KM_LANES - 1) / KM_LANES;
    for (int c : {1, 2, 3, 4, 6, 8})
        if (c >= need) return c;
    return -1;
}

template <int K>
hipError_t launch_kdist(const float *X, int64_t rows, int D, const float *cand, const double *closest, double *dist,
                        hipStream_t s) {
    const int nb = kdist_blocks(rows);
    const int64_t per = (rows + nb * 4 - 1) / (nb * 4);
    const dim3 grid(nb), block(256);
    switch (cpl_for(D)) {
#define KD(C) case C: kdist_kernel<C, K><<<grid, block, 0, s>>>(X, rows, D, cand, closest, dist, per); break
        KD(1); KD(2); KD(3); KD(4); KD(6); KD(8);
#undef KD
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <bool ASSIGN>
hipError_t launch_lloyd(const float *X, int64_t rows, int D, const float *centers, const int32_t *labels_old,
                        int32_t *labels, double *part, double *part_scal, hipStream_t s) {
    const int nb = lloyd_blocks(rows);
    const int64_t per = (rows + (int64_t)nb * LLOYD_WAVES - 1) / ((int64_t)nb * LLOYD_WAVES);
    const dim3 grid(nb), block(LLOYD_THREADS);
    switch (cpl_for(D)) {
#define LL(C) case C: lloyd_kernel<C, ASSIGN><<<grid, block, 0, s>>>(X, rows, D, centers, labels_old, labels, part, \
                                                                     part_scal, per); break
        LL(1); LL(2); LL(3); LL(4); LL(6); LL(8);
#undef LL
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

int check_rows(int32_t S, int32_t dim) {
    if (S < 1) return fail(OCM_EINVAL, "S = %d < 1", S);
    if (dim < 4 || dim % 4 || dim > KM_MAX_DIM) return fail(OCM_EINVAL, "dim = %d (a multiple of 4 in 4..%d)", dim, KM_MAX_DIM);
    return OCM_OK;
}

}  // namespace

extern "C" int ocm_op_kmeans_features(const float *qkv, int32_t batch, int32_t heads, int32_t n_tokens, int32_t head_dim,
                                      int32_t image, int32_t grid, int32_t S, float *X, void *stream) {
    if (!qkv || !X) return fail(OCM_EINVAL, "null argument");
    if (S < 1) return fail(OCM_EINVAL, "S = %d < 1", S);
    if (batch < 1 || heads < 1 || head_dim < 4 || head_dim % 4 || heads * head_dim > KM_MAX_DIM)
        return fail(OCM_EINVAL, "bad qkv shape batch=%d heads=%d head_dim=%d (head_dim %% 4, heads * head_dim <= %d)", batch,
                    heads, head_dim, KM_MAX_DIM);
    if (image < 0 || image >= batch) return fail(OCM_EINVAL, "image %d out of range (batch %d)", image, batch);
    if (grid < 1 || (int64_t)grid * grid + 1 != n_tokens)
        return fail(OCM_EINVAL, "n_tokens = %d is not a %d x %d token grid plus CLS", n_tokens, grid, grid);
    const hipStream_t s = (hipStream_t)stream;
    const int64_t total = (int64_t)S * S * (heads * head_dim / 4);
    const unsigned nb = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 16384));
    kfeat_kernel<<<dim3(nb), dim3(256), 0, s>>>(qkv, X, batch, heads, n_tokens, head_dim, image, grid, S,
                                                (float)grid / (float)S);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" size_t ocm_kmeans_zscore_workspace_bytes(int32_t S, int32_t dim) {
    if (S < 1 || dim < 1) return 0;
    return (size_t)2 * zs_chunks((int64_t)S * S) * dim * sizeof(double);
}

extern "C" int ocm_op_kmeans_zscore(float *X, int32_t S, int32_t dim, double *stats, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    if (!X || !stats) return fail(OCM_EINVAL, "null argument");
    if (int rc = check_rows(S, dim)) return rc;
    const size_t need = ocm_kmeans_zscore_workspace_bytes(S, dim);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "kmeans_zscore workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)S * S;
    double *part = (double *)workspace;
    HIP_TRY(launch_zs<0>(X, stats, part, rows, dim, s));
    HIP_TRY(launch_zs<1>(X, stats, part, rows, dim, s));
    HIP_TRY(launch_zs<2>(X, stats, part, rows, dim, s));
    HIP_TRY(launch_zs<3>(X, stats, part, rows, dim, s));
    return OCM_OK;
}

extern "C" int ocm_op_kmeans_dist(const float *X, int32_t S, int32_t dim, const float *cand, int32_t n_cand,
                                  const double *closest, double *dist, void *stream) {
    if (!X || !cand || !dist) return fail(OCM_EINVAL, "null argument");
    if (int rc = check_rows(S, dim)) return rc;
    if (n_cand < 1 || n_cand > 64) return fail(OCM_EINVAL, "n_cand = %d (1..64)", n_cand);
    const hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)S * S;
    for (int k = 0; k < n_cand; k += 2) {
        const float *c = cand + (size_t)k * dim;
        double *d = dist + (size_t)k * rows;
        HIP_TRY(n_cand - k >= 2 ? launch_kdist<2>(X, rows, dim, c, closest, d, s)
                                : launch_kdist<1>(X, rows, dim, c, closest, d, s));
    }
    return OCM_OK;
}

extern "C" size_t ocm_kmeans_lloyd_workspace_bytes(int32_t S, int32_t dim) {
    if (S < 1 || dim < 1) return 0;
    return (size_t)lloyd_blocks((int64_t)S * S) * (2 * (size_t)dim + LLOYD_SCAL) * sizeof(double);
}

extern "C" int ocm_op_kmeans_lloyd(const float *X, int32_t S, int32_t dim, const float *centers, const int32_t *labels_old,
                                   int32_t *labels, float *centers_new, double *sums, double *info, int32_t assign_only,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    if (!X || !centers || !labels || !info || (!assign_only && !centers_new)) return fail(OCM_EINVAL, "null argument");
    if (int rc = check_rows(S, dim)) return rc;
    const size_t need = ocm_kmeans_lloyd_workspace_bytes(S, dim);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "kmeans_lloyd workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)S * S;
    const int nb = lloyd_blocks(rows);
    double *part = (double *)workspace, *part_scal = part + (size_t)nb * 2 * dim;
    if (assign_only) {
        HIP_TRY(launch_lloyd<true>(X, rows, dim, centers, labels_old, labels, part, part_scal, s));
        lloyd_info_kernel<<<dim3(1), dim3(256), 0, s>>>(part_scal, nb, dim, centers, nullptr, info);
    } else {
        HIP_TRY(launch_lloyd<false>(X, rows, dim, centers, labels_old, labels, part, part_scal, s));
        lloyd_cols_kernel<<<dim3((2 * dim + 15) / 16), dim3(256), 0, s>>>(part, part_scal, nb, dim, sums, centers_new);
        lloyd_info_kernel<<<dim3(1), dim3(256), 0, s>>>(part_scal, nb, dim, centers, centers_new, info);
    }
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
