// kernels_train.hip — the backward pass of LinearProbing's decoders (model.py:142-174) on a frozen encoder, and the
// BatchNorm batch statistics its training-mode forward needs:
//   wgrad_kernel / wgrad_reduce_kernel   dW[N][K] = sum_m dY[m][N] X[m][K] on MFMA, M split across workgroups, slabs summed
//                                        in slice order (no atomics: the same bits on every run)
//   chan_reduce_kernel / chan_finish     per-channel sums of a token-major [rows][C] fp32 tensor in a fixed order: bias
//                                        gradients, batch mean and (two-pass) variance, the ReLU + BatchNorm backward sums
//   bn_relu_bwd_kernel                   dy = g (u - mean(u) - xhat mean(u xhat)), u = dz [y g + h > 0]
//   pixel_shuffle_bwd_kernel             gather (B, c, H, W) -> (B*hp*wp, s*s*c), the exact inverse of pixel_shuffle_kernel
// and the pieces of the ViT encoder backward (SimMIM pre-training) other than the attention (kernels_train_attn.hip):
//   ln_bwd_kernel                        LayerNorm backward per row (two-pass statistics recomputed from x), + residual gradient
//   chan_reduce_kernel<3>                dgamma / dbeta of the LayerNorm as fixed-order column sums
//   gelu_kernel / gelu_bwd_kernel        erf GELU of the fp32 fc1 pre-activation (fc2's operand) and its backward
//   patch_unfold_kernel                  image -> [B*P][C*p*p] rows of the patch-embedding weight gradient
//   patch_grad_kernel / token_sum_kernel the mask blend's split of the token gradient, and the batch sum (cls / pos gradients)
// and finetune.py's loss:
//   dice_partial_kernel / dice_finish    sigmoid Dice loss: per-workgroup sums of p t, p and t, added in a fixed order
//   dice_bwd_kernel                      its gradient into the logits, elementwise
// The forward's BatchNorm-affine + ReLU operand writer is the AFFINE variant of im2col3x3_kernel (kernels_misc.hip).
#include "host_common.h"
#include "launch.h"

#define fail ocm_fail

namespace {

// ---- weight gradient ---------------------------------------------------------------------------------------------------
// One workgroup (4 waves, 2 x 2) owns a TN x 128 tile of dW and one slice of the M rows. Per stage it stages 32 rows of
// dY (32 x TN) and X (32 x 128) from HBM (fp32, row-major: both operands are strided along the contraction axis) into
// LDS in the operand type:
//   E 0 / 2 (bf16 / split pairs): [column block of 32][32 rows][32 columns] 16-bit images with 64-byte rows (hi and lo
//           images for split pairs); an MFMA fragment (eight consecutive rows of one column) is two ds_read_b64_tr_b16
//           (tr_read8, common.h), for A = dY^T as for B = X;
//   E 1 (fp32): plain [32 rows][columns] fp32 rows, one element per lane and k step of v_mfma_f32_32x32x2_f32.
// The next stage's global loads are issued before the current stage's MFMAs. Rows past the slice end and columns past
// N / K load as zeros (pad, don't mask: every lane takes part in the transposed reads).
constexpr int WG_TK = 128, WG_BM = 32;

template <int E, int TN>
struct WgradLds {
    static constexpr int ybytes = E == 1 ? WG_BM * TN * 4 : TN * 64;      // one image of dY (per half for split pairs)
    static constexpr int xbytes = E == 1 ? WG_BM * WG_TK * 4 : WG_TK * 64;
    static constexpr int halves = E == 2 ? 2 : 1;
    static constexpr int bytes = halves * (ybytes + xbytes);
};

template <int E, int COLS>
__device__ __forceinline__ void wgrad_stage_store(char *img, int imgbytes, int row, int col, const f32x4 &v) {
    if (E == 1) {
        *(f32x4 *)(img + (row * COLS + col) * 4) = v;
    } else {
        const int off = (col >> 5) * (WG_BM * 64) + row * 64 + (col & 31) * 2;
        bf16x4 hi, lo;
        if (E == 2) {
            split4(v, hi, lo);
            *(bf16x4 *)(img + imgbytes + off) = lo;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) hi[e] = (bf16)v[e];
        }
        *(bf16x4 *)(img + off) = hi;
    }
}

template <int E, int TN>
__global__ __launch_bounds__(256) void wgrad_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                    float *__restrict__ out, int M, int N, int K, int rows_per_slice,
                                                    size_t slab_elems) {
    using L = WgradLds<E, TN>;
    __shared__ __attribute__((aligned(16))) char smem[L::bytes];
    char *Ys = smem, *Xs = smem + L::halves * L::ybytes;
    constexpr int NI = TN / 64;                 // 32-row output sub-tiles per wave along N
    constexpr int YV = WG_BM * TN / 4 / 256;    // f32x4 loads per thread per stage
    constexpr int XV = WG_BM * WG_TK / 4 / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1, r = lane & 31, h = lane >> 5;
    const int k0 = blockIdx.x * WG_TK, n0 = blockIdx.y * TN;
    const int m_begin = blockIdx.z * rows_per_slice, m_end = min(M, m_begin + rows_per_slice);
    out += (size_t)blockIdx.z * slab_elems;

    f32x4 yv[YV], xv[XV];
    auto load = [&](int m0) {
#pragma unroll
        for (int i = 0; i < YV; ++i) {
            const int v = tid + 256 * i, row = v / (TN / 4), col = (v % (TN / 4)) * 4;
            const int m = m0 + row, n = n0 + col;
            yv[i] = (m < m_end && n < N) ? *(const f32x4 *)(dy + (size_t)m * N + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int v = tid + 256 * i, row = v / (WG_TK / 4), col = (v % (WG_TK / 4)) * 4;
            const int m = m0 + row, k = k0 + col;
            xv[i] = (m < m_end && k < K) ? *(const f32x4 *)(x + (size_t)m * K + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };

    f32x16 acc[NI][2];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // lane address of the transposed read inside one [32 rows][32 columns] block (the Swin V^T read: lane 4q + p of a
    // 16-lane group addresses row q, columns 4p .. 4p+3 of its half of the block)
    const int tr_lane = (8 * h + ((lane >> 2) & 3)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;

    if (m_begin < m_end) load(m_begin);
    for (int m0 = m_begin; m0 < m_end; m0 += WG_BM) {
        __syncthreads();  // the previous stage's reads are done
#pragma unroll
        for (int i = 0; i < YV; ++i) {
            const int v = tid + 256 * i;
            wgrad_stage_store<E, TN>(Ys, L::ybytes, v / (TN / 4), (v % (TN / 4)) * 4, yv[i]);
        }
#pragma unroll
        for (int i = 0; i < XV; ++i) {
            const int v = tid + 256 * i;
            wgrad_stage_store<E, WG_TK>(Xs, L::xbytes, v / (WG_TK / 4), (v % (WG_TK / 4)) * 4, xv[i]);
        }
        __syncthreads();
        if (m0 + WG_BM < m_end) load(m0 + WG_BM);  // in flight during the MFMAs below
        if (E == 1) {
            const float *Yf = (const float *)Ys, *Xf = (const float *)Xs;
#pragma unroll 4
            for (int t = 0; t < WG_BM / 2; ++t) {
                const int row = 2 * t + h;
                float a[NI], b[2];
#pragma unroll
                for (int i = 0; i < NI; ++i) a[i] = Yf[row * TN + wn * (TN / 2) + 32 * i + r];
#pragma unroll
                for (int j = 0; j < 2; ++j) b[j] = Xf[row * WG_TK + wk * 64 + 32 * j + r];
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = mfma32f(a[i], b[j], acc[i][j]);
            }
        } else {
#pragma unroll
            for (int s = 0; s < WG_BM / 16; ++s) {
                bf16x8 ah[NI], al[NI], bh[2], bl[2];
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const char *p = Ys + ((wn * (TN / 2) + 32 * i) >> 5) * (WG_BM * 64) + 16 * s * 64 + tr_lane;
                    ah[i] = tr_read8(p);
                    if (E == 2) al[i] = tr_read8(p + L::ybytes);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const char *p = Xs + ((wk * 64 + 32 * j) >> 5) * (WG_BM * 64) + 16 * s * 64 + tr_lane;
                    bh[j] = tr_read8(p);
                    if (E == 2) bl[j] = tr_read8(p + L::xbytes);
                }
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = E == 2 ? mfma32x3(ah[i], al[i], bh[j], bl[j], acc[i][j]) : mfma32(ah[i], bh[j], acc[i][j]);
            }
        }
    }
    // N and K are multiples of 32: a 32 x 32 sub-tile is wholly inside dW or wholly outside
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nb = n0 + wn * (TN / 2) + 32 * i, kb = k0 + wk * 64 + 32 * j;
            if (nb >= N || kb >= K) continue;
#pragma unroll
            for (int e = 0; e < 16; ++e) out[(size_t)(nb + acc_row32(e, h)) * K + kb + r] = acc[i][j][e];
        }
}

// dW = slab 0 + slab 1 + ... in slice order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ slabs, int slices, size_t n4,
                                                           float *__restrict__ dw) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 s = ((const f32x4 *)slabs)[i];
        for (int z = 1; z < slices; ++z) s += ((const f32x4 *)slabs)[(size_t)z * n4 + i];
        ((f32x4 *)dw)[i] = s;
    }
}

struct WgradPlan {
    int tn, slices, rows_per_slice;
};

// Shape-only decomposition (so that a given shape always sums in the same order): enough (tile, slice) workgroups to give
// the 256 CUs about four each, at least 256 rows per slice, at most 32 slices.
WgradPlan wgrad_plan(int M, int N, int K) {
    WgradPlan p;
    p.tn = N % 128 == 0 ? 128 : 64;
    const long tiles = (long)((N + p.tn - 1) / p.tn) * ((K + WG_TK - 1) / WG_TK);
    long s = (1024 + tiles - 1) / tiles;
    s = std::min<long>(s, (M + 255) / 256);
    s = std::max<long>(1, std::min<long>(s, 32));
    const int per = (int)(((M + s - 1) / s + WG_BM - 1) / WG_BM) * WG_BM;
    p.rows_per_slice = per;
    p.slices = (M + per - 1) / per;
    return p;
}

// ---- per-channel reductions ---------------------------------------------------------------------------------------------
// Rows are cut into R chunks (a function of the row count alone); a workgroup sums 64 channels of one chunk (4 row groups of
// 64 threads, rows strided by 4, combined in LDS in group order) and writes partial[k][chunk][c]; chan_finish_kernel adds
// the R partials of a channel in chunk order. Fixed order everywhere: the same bits on every run.
//   MODE 0: sum x                           MODE 1: sum (x - mean)^2  (the second pass of the variance)
//   MODE 2: sum u and sum u * xhat with u = dz [fma(y, g, h) > 0], xhat = (y - mean) * invstd
//   MODE 3: sum a and sum a * xhat with xhat = (y - mean[m]) * invstd[m]: per-ROW statistics (LayerNorm), `mean` = [rows][2]
int chan_chunks(int64_t rows) { return (int)std::min<int64_t>((rows + 255) / 256, 128); }

template <int MODE>
__global__ __launch_bounds__(256) void chan_reduce_kernel(const float *__restrict__ a, const float *__restrict__ y,
                                                          const float *__restrict__ mean, const float *__restrict__ invstd,
                                                          const float *__restrict__ scale, const float *__restrict__ shift,
                                                          float *__restrict__ part, int64_t rows, int C, int64_t chunk) {
    __shared__ float red[2][4][64];
    const int tc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tc, R = gridDim.y;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = std::min<int64_t>(rows, r0 + chunk);
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        const float mu = (MODE == 1 || MODE == 2) ? mean[c] : 0.f;
        const float is = MODE == 2 ? invstd[c] : 0.f, g = MODE == 2 ? scale[c] : 0.f, hh = MODE == 2 ? shift[c] : 0.f;
        for (int64_t m = r0 + rg; m < r1; m += 4) {
            const float v = a[m * C + c];
            if (MODE == 0) {
                s0 += v;
            } else if (MODE == 1) {
                const float d = v - mu;
                s0 = fmaf(d, d, s0);
            } else if (MODE == 3) {
                const float xh = (y[m * C + c] - mean[2 * m]) * mean[2 * m + 1];
                s0 += v;
                s1 = fmaf(v, xh, s1);
            } else {
                const float yv = y[m * C + c];
                const float u = bn_pre(yv, g, hh) > 0.f ? v : 0.f;
                s0 += u;
                s1 = fmaf(u, (yv - mu) * is, s1);
            }
        }
    }
    red[0][rg][tc] = s0;
    red[1][rg][tc] = s1;
    __syncthreads();
    if (rg == 0 && c < C) {
        part[(size_t)blockIdx.y * C + c] = ((red[0][0][tc] + red[0][1][tc]) + red[0][2][tc]) + red[0][3][tc];
        if (MODE >= 2)
            part[((size_t)R + blockIdx.y) * C + c] = ((red[1][0][tc] + red[1][1][tc]) + red[1][2][tc]) + red[1][3][tc];
    }
}

// out0[c] = sum_r part[0][r][c] (divided by `div` when div > 0), out1 likewise from part[1] when out1 != null
__global__ __launch_bounds__(256) void chan_finish_kernel(const float *__restrict__ part, int R, int C, float div,
                                                          float *__restrict__ out0, float *__restrict__ out1) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s0 = 0.f, s1 = 0.f;
    for (int r = 0; r < R; ++r) s0 += part[(size_t)r * C + c];
    out0[c] = div > 0.f ? s0 / div : s0;
    if (out1) {
        for (int r = 0; r < R; ++r) s1 += part[((size_t)R + r) * C + c];
        out1[c] = div > 0.f ? s1 / div : s1;
    }
}

template <int MODE>
hipError_t launch_chan_reduce(const float *a, const float *y, const float *mean, const float *invstd, const float *scale,
                              const float *shift, float *part, float *out0, float *out1, float div, int64_t rows, int C,
                              hipStream_t s) {
    const int R = chan_chunks(rows);
    const int64_t chunk = (rows + R - 1) / R;
    chan_reduce_kernel<MODE><<<dim3((C + 63) / 64, R), dim3(256), 0, s>>>(a, y, mean, invstd, scale, shift, part, rows, C,
                                                                           chunk);
    chan_finish_kernel<<<dim3((C + 255) / 256), dim3(256), 0, s>>>(part, R, C, div, out0, out1);
    return hipGetLastError();
}

// ---- ReLU + BatchNorm backward, elementwise part ----
__global__ __launch_bounds__(256) void bn_relu_bwd_kernel(const float *__restrict__ dz, const float *__restrict__ y,
                                                          const float *__restrict__ mean, const float *__restrict__ invstd,
                                                          const float *__restrict__ scale, const float *__restrict__ shift,
                                                          const float *__restrict__ dbeta, const float *__restrict__ dgamma,
                                                          float *__restrict__ dy, size_t n4, int C, float inv_rows) {
    const int c4 = C >> 2;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % c4) * 4;
        const f32x4 d = ((const f32x4 *)dz)[i], yv = ((const f32x4 *)y)[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float g = scale[c + e];
            const float u = bn_pre(yv[e], g, shift[c + e]) > 0.f ? d[e] : 0.f;
            const float xh = (yv[e] - mean[c + e]) * invstd[c + e];
            o[e] = g * (u - dbeta[c + e] * inv_rows - xh * (dgamma[c + e] * inv_rows));
        }
        ((f32x4 *)dy)[i] = o;
    }
}

// ---- PixelShuffle backward: one thread per element of the token-major gradient (coalesced stores) ----
__global__ __launch_bounds__(256) void pixel_shuffle_bwd_kernel(const float *__restrict__ gout, float *__restrict__ lin,
                                                                int hp, int wp, int c_out, int sh, size_t total) {
    const int O = c_out * sh * sh, Hs = hp * sh, Ws = wp * sh;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int o = (int)(i % O);
        const size_t row = i / O;
        const int x = (int)(row % wp);
        const size_t r2 = row / wp;
        const int y = (int)(r2 % hp), b = (int)(r2 / hp);
        const int jj = o % sh, ii = (o / sh) % sh, c = o / (sh * sh);
        lin[i] = gout[(((size_t)b * c_out + c) * Hs + y * sh + ii) * Ws + x * sh + jj];
    }
}

// ---- LayerNorm backward, per row: one wave per row, statistics recomputed in two passes from x (a row whose mean is large
// against its spread loses nothing to cancellation), the wave's partial sums combined by a fixed butterfly.
//   xhat = (x - mu) rstd,  dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) + dres
// stats[row] = (mu, rstd) for the column sums of dgamma / dbeta (chan_reduce_kernel<3>).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void ln_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x,
                                                     const float *__restrict__ gamma, const float *dres, float *dx,
                                                     float *__restrict__ stats, int64_t rows, int dim, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float *xr = x + row * dim, *gr = dy + row * dim;
    float s = 0.f;
    for (int c = lane; c < dim; c += 64) s += xr[c];
    const float mu = wave_sum(s) / dim;
    float v = 0.f;
    for (int c = lane; c < dim; c += 64) {
        const float d = xr[c] - mu;
        v = fmaf(d, d, v);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / dim + eps);
    float a = 0.f, bsum = 0.f;
    for (int c = lane; c < dim; c += 64) {
        const float g = gr[c] * gamma[c];
        a += g;
        bsum = fmaf(g, (xr[c] - mu) * rstd, bsum);
    }
    a = wave_sum(a) / dim;
    bsum = wave_sum(bsum) / dim;
    for (int c = lane; c < dim; c += 64) {
        const float xh = (xr[c] - mu) * rstd;
        float o = rstd * (gr[c] * gamma[c] - a - xh * bsum);
        if (dres) o += dres[row * dim + c];
        dx[row * dim + c] = o;
    }
    if (lane == 0) {
        stats[2 * row] = mu;
        stats[2 * row + 1] = rstd;
    }
}

// ---- erf GELU (nn.GELU(), dino/vision_transformer.py:53) of the fp32 fc1 pre-activation: fc2's operand in the operand type of
// the precision (E 0 bf16, 1 fp32, 2 split pairs: element i of a row-structured tensor at sp_off of its index), optionally fp32.
template <int E>
__global__ __launch_bounds__(256) void gelu_kernel(const float *__restrict__ hin, void *__restrict__ out,
                                                   float *__restrict__ out32, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const float g = gelu_erf(hin[i]);
        if (out32) out32[i] = g;
        if (E == 0) {
            ((bf16 *)out)[i] = (bf16)g;
        } else if (E == 1) {
            ((float *)out)[i] = g;
        } else {
            bf16 hi, lo;
            split1(g, hi, lo);
            char *p = (char *)out + (i >> 5) * 128 + (i & 31) * 2;
            *(bf16 *)p = hi;
            *(bf16 *)(p + 64) = lo;
        }
    }
}

// dh = dg * gelu'(h), gelu'(h) = Phi(h) + h phi(h); optionally g = gelu(h) in fp32 (fc2's weight-gradient input)
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float *dg, const float *__restrict__ hin, float *dh,
                                                       float *__restrict__ g32, size_t count) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const float x = hin[i];
        const float cdf = 0.5f * (1.0f + erf_as(x * 0.70710678118654752f));
        const float pdf = 0.3989422804014327f * __builtin_amdgcn_exp2f(-0.7213475204444817f * x * x);  // exp(-x^2/2)/sqrt(2pi)
        if (g32) g32[i] = x * cdf;
        dh[i] = dg[i] * fmaf(x, pdf, cdf);
    }
}

// ---- patch embedding (Conv2d(C, D, p, stride p)) backward ----
// cols[b*P + py*wp + px][c*p*p + ky*p + kx] = image[b][c][py*p + ky][px*p + kx]: the K order of the (D, C, p, p) weight
__global__ __launch_bounds__(256) void patch_unfold_kernel(const float *__restrict__ img, float *__restrict__ cols, int C,
                                                           int Hh, int Ww, int p, size_t total) {
    const int hp = Hh / p, wp = Ww / p, K = C * p * p;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int k = (int)(i % K);
        const size_t row = i / K;
        const int px = (int)(row % wp);
        const size_t r2 = row / wp;
        const int py = (int)(r2 % hp), b = (int)(r2 / hp);
        const int kx = k % p, ky = (k / p) % p, c = k / (p * p);
        cols[i] = img[(((size_t)b * C + c) * Hh + py * p + ky) * Ww + px * p + kx];
    }
}

// token gradient dT [B][N][D] of t = cat(cls, patch * (1 - w) + mask_token * w) + pos:
//   dpatch[b*P + p][d] = (1 - w) dT[b][1 + p][d],  wdt[b*P + p][d] = w dT[b][1 + p][d]  (w = 0 without a mask)
__global__ __launch_bounds__(256) void patch_grad_kernel(const float *__restrict__ dtok, const float *__restrict__ mask,
                                                         float *__restrict__ dpatch, float *__restrict__ wdt, int N, int D,
                                                         size_t total) {
    const int P = N - 1;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int d = (int)(i % D);
        const size_t bp = i / D;
        const int b = (int)(bp / P), pp = (int)(bp % P);
        const float v = dtok[((size_t)b * N + 1 + pp) * D + d];
        const float w = mask ? mask[bp] : 0.f;
        dpatch[i] = (1.0f - w) * v;
        wdt[i] = w * v;
    }
}

// out[n][d] = sum_b dT[b][n][d], images in order
__global__ __launch_bounds__(256) void token_sum_kernel(const float *__restrict__ dtok, float *__restrict__ out, int B,
                                                        size_t nd) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nd; i += (size_t)gridDim.x * 256) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dtok[(size_t)b * nd + i];
        out[i] = s;
    }
}

// ---- sigmoid Dice loss (utils.py:410-424: finetune.py's loss); the sigmoid is sigmoid_parts (common.h) ----
// The count is cut into G spans (a function of the count alone, every span a multiple of four elements); workgroup g sums
// p t, p and t over span g: per thread in index order, the wave by the fixed butterfly, the four waves in wave order, and
// writes part[k][g]. dice_finish_kernel adds the G partials of each sum (lane l takes g = l, l + 64, ..., then the same
// butterfly) and writes the three sums and the loss. Fixed order everywhere: the same bits on every run. VEC: 16-byte
// loads (both pointers 16-byte aligned), the last span's tail of fewer than four elements scalar.
constexpr int DICE_SPAN = 4096, DICE_MAX_WG = 1024;

struct DicePlan {
    size_t span;
    int groups;
};

DicePlan dice_plan(size_t count) {
    const size_t g0 = std::min<size_t>((count + DICE_SPAN - 1) / DICE_SPAN, DICE_MAX_WG);
    DicePlan p;
    p.span = ((count + g0 - 1) / g0 + 3) / 4 * 4;
    p.groups = (int)((count + p.span - 1) / p.span);
    return p;
}

template <bool VEC>
__global__ __launch_bounds__(256) void dice_partial_kernel(const float *__restrict__ x, const float *__restrict__ t,
                                                           float *__restrict__ part, size_t count, size_t span) {
    __shared__ float red[3][4];
    const size_t begin = (size_t)blockIdx.x * span, end = std::min<size_t>(count, begin + span);
    const size_t n = end - begin, nv = VEC ? n / 4 : 0;
    const float *xs = x + begin, *ts = t + begin;
    float s_pt = 0.f, s_p = 0.f, s_t = 0.f;
    for (size_t i = threadIdx.x; i < nv; i += 256) {
        const f32x4 xv = ((const f32x4 *)xs)[i], tv = ((const f32x4 *)ts)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float p, pq;
            sigmoid_parts(xv[e], p, pq);
            s_pt = fmaf(p, tv[e], s_pt);
            s_p += p;
            s_t += tv[e];
        }
    }
    for (size_t i = 4 * nv + threadIdx.x; i < n; i += 256) {
        float p, pq;
        sigmoid_parts(xs[i], p, pq);
        s_pt = fmaf(p, ts[i], s_pt);
        s_p += p;
        s_t += ts[i];
    }
    s_pt = wave_sum(s_pt);
    s_p = wave_sum(s_p);
    s_t = wave_sum(s_t);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = s_pt;
        red[1][wave] = s_p;
        red[2][wave] = s_t;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const float *r = red[threadIdx.x];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
}

__global__ __launch_bounds__(64) void dice_finish_kernel(const float *__restrict__ part, int G, float smooth,
                                                         float *__restrict__ sums, float *__restrict__ loss) {
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float a = 0.f;
        for (int g = threadIdx.x; g < G; g += 64) a += part[(size_t)k * G + g];
        s[k] = wave_sum(a);
    }
    if (threadIdx.x == 0) {
        sums[0] = s[0];
        sums[1] = s[1];
        sums[2] = s[2];
        *loss = 1.0f - (2.0f * s[0] + smooth) / (s[1] + s[2] + smooth);
    }
}

// dx = -g (2 t S - (2 I + s)) / S^2 p (1 - p) with S = sum p + sum t + s: c1 t + c0 times p (1 - p), c1 = -2 g / S,
// c0 = g (2 I + s) / S^2 (sums and g read from device memory by every thread: three cached words)
template <bool VEC>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float *__restrict__ x, const float *__restrict__ t,
                                                       const float *__restrict__ sums, const float *__restrict__ gloss,
                                                       float *__restrict__ dx, size_t count, float smooth) {
    const float g = *gloss, S = sums[1] + sums[2] + smooth;
    const float c1 = -2.0f * g / S, c0 = g * (2.0f * sums[0] + smooth) / (S * S);
    const size_t nv = VEC ? count / 4 : 0, stride = (size_t)gridDim.x * 256, tid = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t i = tid; i < nv; i += stride) {
        const f32x4 xv = ((const f32x4 *)x)[i], tv = ((const f32x4 *)t)[i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float p, pq;
            sigmoid_parts(xv[e], p, pq);
            o[e] = fmaf(c1, tv[e], c0) * pq;
        }
        ((f32x4 *)dx)[i] = o;
    }
    for (size_t i = 4 * nv + tid; i < count; i += stride) {
        float p, pq;
        sigmoid_parts(x[i], p, pq);
        dx[i] = fmaf(c1, t[i], c0) * pq;
    }
}

bool aligned16(const void *a, const void *b, const void *c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

size_t grid_of(size_t work, size_t cap) { return std::max<size_t>(1, std::min<size_t>((work + 255) / 256, cap)); }

int prec_ok(int32_t precision) {
    if (precision != OCM_PREC_BF16 && precision != OCM_PREC_FP32 && precision != OCM_PREC_BF16X3)
        return fail(OCM_EINVAL, "bad precision %d", precision);
    return OCM_OK;
}

}  // namespace

// ---- C ABI (include/ocm_vit.h, "decoder training") -----------------------------------------------------------------------
extern "C" size_t ocm_channel_reduce_workspace_bytes(int64_t rows, int32_t channels) {
    if (rows <= 0 || channels <= 0) return 0;
    return (size_t)2 * chan_chunks(rows) * channels * sizeof(float);
}

extern "C" size_t ocm_weight_grad_workspace_bytes(int32_t M, int32_t N, int32_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const WgradPlan p = wgrad_plan(M, N, K);
    const size_t slabs = p.slices > 1 ? (size_t)p.slices * N * K * sizeof(float) : 0;
    return std::max(slabs, ocm_channel_reduce_workspace_bytes(M, N));
}

extern "C" int ocm_op_weight_grad(int32_t precision, const float *dy, const float *x, float *dw, float *db, int32_t M,
                                  int32_t N, int32_t K, void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = prec_ok(precision)) return rc;
    if (!dy || !x || !dw) return fail(OCM_EINVAL, "null argument");
    if (M <= 0 || N <= 0 || K <= 0 || N % 32 || K % 32)
        return fail(OCM_EINVAL, "bad shape M=%d N=%d K=%d (N %% 32, K %% 32)", M, N, K);
    const size_t need = ocm_weight_grad_workspace_bytes(M, N, K);
    if (need && (!workspace || workspace_bytes < need))
        return fail(OCM_ENOMEM, "weight_grad workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const WgradPlan p = wgrad_plan(M, N, K);
    float *target = p.slices > 1 ? (float *)workspace : dw;
    const dim3 grid((K + WG_TK - 1) / WG_TK, (N + p.tn - 1) / p.tn, p.slices), block(256);
    const size_t slab = (size_t)N * K;
#define WGRAD(E, TN) wgrad_kernel<E, TN><<<grid, block, 0, s>>>(dy, x, target, M, N, K, p.rows_per_slice, slab)
    if (p.tn == 128) {
        if (precision == OCM_PREC_BF16) WGRAD(0, 128); else if (precision == OCM_PREC_FP32) WGRAD(1, 128); else WGRAD(2, 128);
    } else {
        if (precision == OCM_PREC_BF16) WGRAD(0, 64); else if (precision == OCM_PREC_FP32) WGRAD(1, 64); else WGRAD(2, 64);
    }
#undef WGRAD
    HIP_TRY(hipGetLastError());
    if (p.slices > 1) {
        wgrad_reduce_kernel<<<dim3((unsigned)grid_of(slab / 4, 4096)), dim3(256), 0, s>>>((const float *)workspace, p.slices,
                                                                                          slab / 4, dw);
        HIP_TRY(hipGetLastError());
    }
    // the bias gradient reuses the workspace once the slabs are consumed (stream order)
    if (db) HIP_TRY(launch_chan_reduce<0>(dy, nullptr, nullptr, nullptr, nullptr, nullptr, (float *)workspace, db, nullptr,
                                          0.f, M, N, s));
    return OCM_OK;
}

extern "C" int ocm_op_batch_stats(const float *x, float *mean, float *var, int64_t rows, int32_t channels, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    if (!x || !mean || !var) return fail(OCM_EINVAL, "null argument");
    if (rows <= 0 || channels <= 0) return fail(OCM_EINVAL, "bad shape rows=%lld channels=%d", (long long)rows, channels);
    const size_t need = ocm_channel_reduce_workspace_bytes(rows, channels);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "batch_stats workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    float *part = (float *)workspace;
    HIP_TRY(launch_chan_reduce<0>(x, nullptr, nullptr, nullptr, nullptr, nullptr, part, mean, nullptr, (float)rows, rows,
                                  channels, s));
    HIP_TRY(launch_chan_reduce<1>(x, nullptr, mean, nullptr, nullptr, nullptr, part, var, nullptr, (float)rows, rows, channels,
                                  s));
    return OCM_OK;
}

extern "C" int ocm_op_bn_relu_im2col3x3(int32_t precision, const float *y, const float *scale, const float *shift, void *out,
                                        int32_t batch, int32_t h, int32_t w, int32_t channels, void *stream) {
    if (int rc = prec_ok(precision)) return rc;
    if (!y || !scale || !shift || !out) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || h <= 0 || w <= 0 || channels <= 0 || channels % 32)
        return fail(OCM_EINVAL, "bad shape batch=%d h=%d w=%d channels=%d (channels %% 32)", batch, h, w, channels);
    HIP_TRY(launch_bn_relu_im2col3x3(precision, y, scale, shift, out, batch, h, w, channels, (hipStream_t)stream));
    return OCM_OK;
}

extern "C" int ocm_op_bn_relu_backward(const float *dz, const float *y, const float *mean, const float *invstd,
                                       const float *scale, const float *shift, float *dy, float *dgamma, float *dbeta,
                                       int64_t rows, int32_t channels, void *workspace, size_t workspace_bytes, void *stream) {
    if (!dz || !y || !mean || !invstd || !scale || !shift || !dy || !dgamma || !dbeta) return fail(OCM_EINVAL, "null argument");
    if (rows <= 0 || channels <= 0 || channels % 4)
        return fail(OCM_EINVAL, "bad shape rows=%lld channels=%d (channels %% 4)", (long long)rows, channels);
    const size_t need = ocm_channel_reduce_workspace_bytes(rows, channels);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "bn_relu_backward workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_chan_reduce<2>(dz, y, mean, invstd, scale, shift, (float *)workspace, dbeta, dgamma, 0.f, rows, channels, s));
    const size_t n4 = (size_t)rows * channels / 4;
    bn_relu_bwd_kernel<<<dim3((unsigned)grid_of(n4, 8192)), dim3(256), 0, s>>>(dz, y, mean, invstd, scale, shift, dbeta, dgamma,
                                                                              dy, n4, channels, 1.0f / (float)rows);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_pixel_shuffle_backward(const float *grad_out, float *grad_lin, int32_t batch, int32_t hp, int32_t wp,
                                             int32_t c_out, int32_t sh, void *stream) {
    if (!grad_out || !grad_lin) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || hp <= 0 || wp <= 0 || c_out <= 0 || sh <= 0) return fail(OCM_EINVAL, "bad shape");
    const size_t total = (size_t)batch * hp * wp * c_out * sh * sh;
    pixel_shuffle_bwd_kernel<<<dim3((unsigned)grid_of(total, 8192)), dim3(256), 0, (hipStream_t)stream>>>(
        grad_out, grad_lin, hp, wp, c_out, sh, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

// ---- C ABI (include/ocm_vit.h, "ViT encoder training") -------------------------------------------------------------------
extern "C" size_t ocm_layernorm_backward_workspace_bytes(int64_t rows, int32_t dim) {
    if (rows <= 0 || dim <= 0) return 0;
    return ocm_channel_reduce_workspace_bytes(rows, dim) + (size_t)2 * rows * sizeof(float);
}

extern "C" int ocm_op_layernorm_backward(const float *dy, const float *x, const float *gamma, const float *dres, float *dx,
                                         float *dgamma, float *dbeta, int64_t rows, int32_t dim, float eps, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    if (!dy || !x || !gamma || !dx || !dgamma || !dbeta) return fail(OCM_EINVAL, "null argument");
    if (rows <= 0 || dim <= 0) return fail(OCM_EINVAL, "bad shape rows=%lld dim=%d", (long long)rows, dim);
    const size_t need = ocm_layernorm_backward_workspace_bytes(rows, dim);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "layernorm_backward workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    float *stats = (float *)workspace, *part = stats + 2 * rows;
    ln_bwd_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s>>>(dy, x, gamma, dres, dx, stats, rows, dim, eps);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_chan_reduce<3>(dy, x, stats, nullptr, nullptr, nullptr, part, dbeta, dgamma, 0.f, rows, dim, s));
    return OCM_OK;
}

extern "C" int ocm_op_gelu(int32_t precision, const float *h, void *out, float *out_f32, size_t count, void *stream) {
    if (int rc = prec_ok(precision)) return rc;
    if (!h || !out) return fail(OCM_EINVAL, "null argument");
    if (count == 0 || (precision == OCM_PREC_BF16X3 && count % 32)) return fail(OCM_EINVAL, "bad count %zu", count);
    const dim3 grid((unsigned)grid_of(count, 8192)), block(256);
    const hipStream_t s = (hipStream_t)stream;
    if (precision == OCM_PREC_BF16) gelu_kernel<0><<<grid, block, 0, s>>>(h, out, out_f32, count);
    else if (precision == OCM_PREC_FP32) gelu_kernel<1><<<grid, block, 0, s>>>(h, out, out_f32, count);
    else gelu_kernel<2><<<grid, block, 0, s>>>(h, out, out_f32, count);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_gelu_backward(const float *dg, const float *h, float *dh, float *g_f32, size_t count, void *stream) {
    if (!dg || !h || !dh) return fail(OCM_EINVAL, "null argument");
    if (count == 0) return fail(OCM_EINVAL, "bad count");
    gelu_bwd_kernel<<<dim3((unsigned)grid_of(count, 8192)), dim3(256), 0, (hipStream_t)stream>>>(dg, h, dh, g_f32, count);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_patch_unfold(const float *image, float *cols, int32_t batch, int32_t channels, int32_t height,
                                   int32_t width, int32_t patch, void *stream) {
    if (!image || !cols) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || channels <= 0 || patch <= 0 || height <= 0 || width <= 0 || height % patch || width % patch)
        return fail(OCM_EINVAL, "bad shape batch=%d channels=%d %dx%d patch=%d", batch, channels, height, width, patch);
    const size_t total = (size_t)batch * (height / patch) * (width / patch) * channels * patch * patch;
    patch_unfold_kernel<<<dim3((unsigned)grid_of(total, 8192)), dim3(256), 0, (hipStream_t)stream>>>(image, cols, channels,
                                                                                                    height, width, patch, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" size_t ocm_patch_embed_backward_workspace_bytes(int32_t batch, int32_t n_tokens, int32_t dim) {
    if (batch <= 0 || n_tokens <= 1 || dim <= 0) return 0;
    const int64_t rows = (int64_t)batch * (n_tokens - 1);
    return (size_t)rows * dim * sizeof(float) + ocm_channel_reduce_workspace_bytes(rows, dim);
}

extern "C" int ocm_op_patch_embed_backward(const float *dtok, const float *mask, float *dpatch, float *dmask_token,
                                           float *dpos, int32_t batch, int32_t n_tokens, int32_t dim, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    if (!dtok || !dpatch || !dpos || (mask && !dmask_token)) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || n_tokens <= 1 || dim <= 0)
        return fail(OCM_EINVAL, "bad shape batch=%d n_tokens=%d dim=%d", batch, n_tokens, dim);
    const size_t need = ocm_patch_embed_backward_workspace_bytes(batch, n_tokens, dim);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "patch_embed_backward workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const int64_t rows = (int64_t)batch * (n_tokens - 1);
    const size_t total = (size_t)rows * dim;
    float *wdt = (float *)workspace, *part = wdt + total;
    patch_grad_kernel<<<dim3((unsigned)grid_of(total, 8192)), dim3(256), 0, s>>>(dtok, mask, dpatch, wdt, n_tokens, dim, total);
    HIP_TRY(hipGetLastError());
    if (mask)
        HIP_TRY(launch_chan_reduce<0>(wdt, nullptr, nullptr, nullptr, nullptr, nullptr, part, dmask_token, nullptr, 0.f, rows,
                                      dim, s));
    const size_t nd = (size_t)n_tokens * dim;
    token_sum_kernel<<<dim3((unsigned)grid_of(nd, 4096)), dim3(256), 0, s>>>(dtok, dpos, batch, nd);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

// ---- C ABI (include/ocm_vit.h, "Dice loss") ------------------------------------------------------------------------------
extern "C" size_t ocm_dice_loss_workspace_bytes(size_t count) {
    if (count == 0) return 0;
    return (size_t)3 * dice_plan(count).groups * sizeof(float);
}

extern "C" int ocm_op_dice_loss(const float *logits, const float *targets, float *loss_out, float *sums_out, size_t count,
                                float smooth, void *workspace, size_t workspace_bytes, void *stream) {
    if (!logits || !targets || !loss_out || !sums_out) return fail(OCM_EINVAL, "null argument");
    if (count == 0) return fail(OCM_EINVAL, "bad count");
    const size_t need = ocm_dice_loss_workspace_bytes(count);
    if (!workspace || workspace_bytes < need)
        return fail(OCM_ENOMEM, "dice_loss workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const DicePlan p = dice_plan(count);
    float *part = (float *)workspace;
    if (aligned16(logits, targets))
        dice_partial_kernel<true><<<dim3(p.groups), dim3(256), 0, s>>>(logits, targets, part, count, p.span);
    else
        dice_partial_kernel<false><<<dim3(p.groups), dim3(256), 0, s>>>(logits, targets, part, count, p.span);
    HIP_TRY(hipGetLastError());
    dice_finish_kernel<<<dim3(1), dim3(64), 0, s>>>(part, p.groups, smooth, sums_out, loss_out);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_dice_loss_backward(const float *logits, const float *targets, const float *sums, const float *grad_loss,
                                         float *dlogits, size_t count, float smooth, void *stream) {
    if (!logits || !targets || !sums || !grad_loss || !dlogits) return fail(OCM_EINVAL, "null argument");
    if (count == 0) return fail(OCM_EINVAL, "bad count");
    const dim3 grid((unsigned)grid_of((count + 3) / 4, 4096)), block(256);
    const hipStream_t s = (hipStream_t)stream;
    if (aligned16(logits, targets, dlogits))
        dice_bwd_kernel<true><<<grid, block, 0, s>>>(logits, targets, sums, grad_loss, dlogits, count, smooth);
    else
        dice_bwd_kernel<false><<<grid, block, 0, s>>>(logits, targets, sums, grad_loss, dlogits, count, smooth);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
