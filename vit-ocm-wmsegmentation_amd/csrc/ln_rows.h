// ln_rows.h — the row arithmetic of nn.LayerNorm on a row that already sits in registers: statistics, affine, store in the
// output kind. One statement of it, shared by the kernels that own rows this way (kernels_misc.hip: layernorm_kernel /
// layernorm_v4_kernel; kernels_drop_path.hip: the drop-path + LayerNorm kernels), so that all of them form the same bits
// from the same row values.
// OUT: 0 = fp32, 1 = bf16, 2 = split-bf16 pairs (common.h: sp32 rows)
#pragma once
#include "common.h"

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

constexpr int LN_MAXV = 8;  // generic rows: float2 per lane per 128 columns, dim <= 1024

// One wavefront per row, lane `lane` holding columns lane * 2 + i * 128 (+ 1) in v[i] where they are below dim: mean and
// biased variance in two in-register passes (same two-pass form as ATen's CPU kernel), fp32 statistics.
template <int OUT>
__device__ __forceinline__ void ln_row(const f32x2 (&v)[LN_MAXV], const float *__restrict__ gamma,
                                       const float *__restrict__ beta, void *__restrict__ y, int64_t row, int dim, int lane,
                                       float eps) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane * 2 + i * 128;
        if (c < dim) s += v[i][0] + v[i][1];
    }
    const float mean = wave_sum(s) / (float)dim;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane * 2 + i * 128;
        if (c < dim) {
            const float a = v[i][0] - mean, b = v[i][1] - mean;
            q += a * a + b * b;
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)dim + eps);
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane * 2 + i * 128;
        if (c < dim) {
            const f32x2 g = *(const f32x2 *)(gamma + c), b = *(const f32x2 *)(beta + c);
            const float o0 = (v[i][0] - mean) * rstd * g[0] + b[0];
            const float o1 = (v[i][1] - mean) * rstd * g[1] + b[1];
            if (OUT == 1) {
                bf16x2 o;
                o[0] = (bf16)o0;
                o[1] = (bf16)o1;
                *(bf16x2 *)((bf16 *)y + row * dim + c) = o;
            } else if (OUT == 2) {
                bf16 h0, l0, h1, l1;
                split1(o0, h0, l0);
                split1(o1, h1, l1);
                bf16x2 hi, lo;
                hi[0] = h0; hi[1] = h1; lo[0] = l0; lo[1] = l1;
                char *rp = (char *)y + row * dim * 4 + sp_off(c);
                *(bf16x2 *)rp = hi;
                *(bf16x2 *)(rp + 64) = lo;
            } else {
                f32x2 o = {o0, o1};
                *(f32x2 *)((float *)y + row * dim + c) = o;
            }
        }
    }
}

// dim = NV * 128: half a wavefront per row, lane `sub` (0 .. 31) of the half holding columns sub * 4 + i * 128 .. + 3 in v[i];
// 8-byte bf16 / 16-byte fp32 stores.
template <int OUT, int NV>
__device__ __forceinline__ void ln_row_v4(const f32x4 (&v)[NV], const float *__restrict__ gamma,
                                          const float *__restrict__ beta, void *__restrict__ y, int64_t row, int sub,
                                          float eps) {
    constexpr int dim = NV * 128;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s * (1.0f / dim);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = v[i][e] - mean;
            q = fmaf(d, d, q);
        }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = 1.0f / sqrtf(q * (1.0f / dim) + eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = sub * 4 + i * 128;
        const f32x4 g = *(const f32x4 *)(gamma + c), b = *(const f32x4 *)(beta + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (v[i][e] - mean) * rstd * g[e] + b[e];
        if (OUT == 1) {
            bf16x4 ob;
#pragma unroll
            for (int e = 0; e < 4; ++e) ob[e] = (bf16)o[e];
            *(bf16x4 *)((bf16 *)y + row * dim + c) = ob;
        } else if (OUT == 2) {
            bf16x4 hi, lo;
            split4(o, hi, lo);
            char *rp = (char *)y + row * dim * 4 + sp_off(c);
            *(bf16x4 *)rp = hi;
            *(bf16x4 *)(rp + 64) = lo;
        } else {
            *(f32x4 *)((float *)y + row * dim + c) = o;
        }
    }
}
