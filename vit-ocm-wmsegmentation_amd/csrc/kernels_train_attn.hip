// kernels_train_attn.hip — backward of softmax(q k^T * scale) v (dino/vision_transformer.py:83-87) for heads of 64 or 128
// channels: the hot part of the ViT backward that SimMIM pre-training (model.py:55-83, mim.py) runs.
//
// Inputs are fp32 in every precision mode: q / k / v as the qkv_f32 tensor [3][B][H][N][hd] that ocm_op_qkv_proj_hd writes,
// lse2 [B*H][N] from ocm_op_attention_hd, the context gradient dO = dctx [B][N][H*hd] and delta = rowsum(dO o O) [B*H][N]
// (attn_bwd_delta_kernel). All products run on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate) for all three
// set_precision modes: the probabilities are recomputed as P = exp2(s * scale * log2e - lse2) from fp32 q and k; N x N is never
// materialised. Outputs go straight into the fp32 [B*N][3*H*hd] dqkv matrix in the (3, H, hd) column order of qkv.weight.
//
// Reproducibility: no atomics. Two kernels, each owning its outputs:
//   attn_bwd_dkdv_kernel  key-block-major: a workgroup owns 128 keys (four waves of 32) and walks every query tile in order,
//                         dV += P^T dO, dK += dS^T Q (dS = P o (dP - delta), dP = dO V^T);
//   attn_bwd_dq_kernel    query-block-major: a workgroup owns 128 queries and walks every key tile in order, dQ += dS K.
// The scores and dP are computed twice (once per kernel) instead of handing dS from one to the other: the ordered hand-off
// needs a cross-workgroup protocol, the split needs none and every sum has one fixed order by construction.
//
// Tile mechanics (both kernels): the 32-token tile that is walked is staged in LDS with rows padded to hd + 1 floats (a row-
// strided MFMA operand read then hits 32 different banks); the owned rows of the wave's A operands (K and V, or Q and dO) are
// loaded once per kernel into per-lane arrays. With 64-wide heads those stay in registers. With 128-wide heads the S / dP loop
// (unroll 8) indexes them at run time and the compiler keeps them in scratch (528 bytes per lane, reloaded inside the loop from
// L1 / L2): a full unroll keeps them in registers but drops occupancy from 2 to 1 wave per SIMD and measured slower, 9.85 ms
// against 7.27 ms for both kernels at (B 16, H 3, N 2305, hd 128). P^T / dS pass from the accumulator layout to the A-operand
// layout through a per-wave 32 x 33 LDS tile. Rows past N (the edge tile, padded heads) load as zeros and their probabilities are forced to 0, so nothing from
// outside [0, N) enters a sum.
#include "host_common.h"
#include "launch.h"

#define fail ocm_fail

namespace {

constexpr float AB_LOG2E = 1.4426950408889634f;
constexpr int AB_T = 32;  // tokens per tile: one MFMA block
constexpr int AB_W = 4;   // waves per workgroup, 32 owned tokens each

template <int HD>
struct AbLds {
    static constexpr int ld = HD + 1;                       // padded row (floats)
    static constexpr int tile = AB_T * ld;                  // one staged 32-token tile
    static constexpr int tr = AB_T * 33;                    // one wave's transpose tile
    static constexpr int dkdv_bytes = (2 * tile + 2 * AB_T + 2 * AB_W * tr) * 4;
    static constexpr int dq_bytes = (2 * tile + AB_W * tr) * 4;
};

template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dkdv_kernel(const float *__restrict__ qkv, const float *__restrict__ lse2,
                                                            const float *__restrict__ dctx, const float *__restrict__ delta,
                                                            float *__restrict__ dqkv, int B, int N, int H, float c2,
                                                            float scale) {
    using L = AbLds<HD>;
    constexpr int LD = L::ld, NJ = HD / 32, KT = HD / 2;
    extern __shared__ __attribute__((aligned(16))) float ab_smem[];
    float *Qs = ab_smem, *Os = Qs + L::tile, *Ls = Os + L::tile, *Ds = Ls + AB_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    float *Ps = Ds + AB_T + wave * 2 * L::tr, *Ss = Ps + L::tr;
    const int bh = blockIdx.y, b = bh / H, hh = bh - b * H, D = H * HD;
    const size_t plane = (size_t)B * H * N * HD;
    const float *Q = qkv + (size_t)bh * N * HD, *K = Q + plane, *V = K + plane;
    const float *dO = dctx + (size_t)b * N * D + hh * HD;
    const int key0 = blockIdx.x * (AB_W * AB_T) + wave * AB_T, key = key0 + r;

    float kr[KT], vr[KT];  // A operands: row `key`, columns 2t + h
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        kr[t] = key < N ? K[(size_t)key * HD + 2 * t + h] : 0.f;
        vr[t] = key < N ? V[(size_t)key * HD + 2 * t + h] : 0.f;
    }
    f32x16 dk[NJ], dv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) dk[j][e] = dv[j][e] = 0.f;

    for (int q0 = 0; q0 < N; q0 += AB_T) {
        __syncthreads();  // the previous tile's reads are done
        for (int i = tid; i < AB_T * HD; i += 256) {
            const int row = i / HD, col = i - row * HD, q = q0 + row;
            Qs[row * LD + col] = q < N ? Q[(size_t)q * HD + col] : 0.f;
            Os[row * LD + col] = q < N ? dO[(size_t)q * D + col] : 0.f;
        }
        if (tid < AB_T) {
            const int q = q0 + tid;
            Ls[tid] = q < N ? lse2[(size_t)bh * N + q] : 0.f;
            Ds[tid] = q < N ? delta[(size_t)bh * N + q] : 0.f;
        }
        __syncthreads();
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll 8
        for (int t = 0; t < KT; ++t) {
            s = mfma32f(kr[t], Qs[r * LD + 2 * t + h], s);    // S^T[key][q] = K Q^T
            dp = mfma32f(vr[t], Os[r * LD + 2 * t + h], dp);  // dP^T[key][q] = V dO^T
        }
        // accumulator element e: key key0 + acc_row32(e, h), query q0 + r
        const bool qok = q0 + r < N;
        const float l = Ls[r], dl = Ds[r];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int kk = acc_row32(e, h);
            const float p = (qok && key0 + kk < N) ? fast_exp2(s[e] * c2 - l) : 0.f;
            Ps[kk * 33 + r] = p;
            Ss[kk * 33 + r] = p * (dp[e] - dl);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < AB_T / 2; ++t) {
            const int qq = 2 * t + h;
            const float pa = Ps[r * 33 + qq], sa = Ss[r * 33 + qq];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                dv[j] = mfma32f(pa, Os[qq * LD + 32 * j + r], dv[j]);  // dV[key][d] += P^T dO
                dk[j] = mfma32f(sa, Qs[qq * LD + 32 * j + r], dk[j]);  // dK[key][d] += dS^T Q
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int kk = key0 + acc_row32(e, h);
            if (kk >= N) continue;
            float *row = dqkv + ((size_t)b * N + kk) * 3 * D + hh * HD + 32 * j + r;
            row[D] = dk[j][e] * scale;
            row[2 * D] = dv[j][e];
        }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float *__restrict__ qkv, const float *__restrict__ lse2,
                                                          const float *__restrict__ dctx, const float *__restrict__ delta,
                                                          float *__restrict__ dqkv, int B, int N, int H, float c2,
                                                          float scale) {
    using L = AbLds<HD>;
    constexpr int LD = L::ld, NJ = HD / 32, KT = HD / 2;
    extern __shared__ __attribute__((aligned(16))) float ab_smem[];
    float *Ks = ab_smem, *Vs = Ks + L::tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    float *Ss = Vs + L::tile + wave * L::tr;
    const int bh = blockIdx.y, b = bh / H, hh = bh - b * H, D = H * HD;
    const size_t plane = (size_t)B * H * N * HD;
    const float *Q = qkv + (size_t)bh * N * HD, *K = Q + plane, *V = K + plane;
    const float *dO = dctx + (size_t)b * N * D + hh * HD;
    const int q0 = blockIdx.x * (AB_W * AB_T) + wave * AB_T, query = q0 + r;

    float qr[KT], orr[KT];  // A operands: row `query`, columns 2t + h
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        qr[t] = query < N ? Q[(size_t)query * HD + 2 * t + h] : 0.f;
        orr[t] = query < N ? dO[(size_t)query * D + 2 * t + h] : 0.f;
    }
    float lr[16], dr[16];  // per accumulator row
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int qq = q0 + acc_row32(e, h);
        lr[e] = qq < N ? lse2[(size_t)bh * N + qq] : 0.f;
        dr[e] = qq < N ? delta[(size_t)bh * N + qq] : 0.f;
    }
    f32x16 dq[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) dq[j][e] = 0.f;

    for (int k0 = 0; k0 < N; k0 += AB_T) {
        __syncthreads();
        for (int i = tid; i < AB_T * HD; i += 256) {
            const int row = i / HD, col = i - row * HD, kk = k0 + row;
            Ks[row * LD + col] = kk < N ? K[(size_t)kk * HD + col] : 0.f;
            Vs[row * LD + col] = kk < N ? V[(size_t)kk * HD + col] : 0.f;
        }
        __syncthreads();
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll 8
        for (int t = 0; t < KT; ++t) {
            s = mfma32f(qr[t], Ks[r * LD + 2 * t + h], s);    // S[q][key] = Q K^T
            dp = mfma32f(orr[t], Vs[r * LD + 2 * t + h], dp);  // dP[q][key] = dO V^T
        }
        // accumulator element e: query q0 + acc_row32(e, h), key k0 + r
        const bool kok = k0 + r < N;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int qq = acc_row32(e, h);
            const float p = (kok && q0 + qq < N) ? fast_exp2(s[e] * c2 - lr[e]) : 0.f;
            Ss[qq * 33 + r] = p * (dp[e] - dr[e]);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < AB_T / 2; ++t) {
            const int kk = 2 * t + h;
            const float sa = Ss[r * 33 + kk];
#pragma unroll
            for (int j = 0; j < NJ; ++j) dq[j] = mfma32f(sa, Ks[kk * LD + 32 * j + r], dq[j]);  // dQ[q][d] += dS K
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int qq = q0 + acc_row32(e, h);
            if (qq < N) dqkv[((size_t)b * N + qq) * 3 * D + hh * HD + 32 * j + r] = dq[j][e] * scale;
        }
}

// delta[b*H + h][n] = sum_d dctx[b][n][h*hd + d] * ctx[b][n][h*hd + d] (ctx in the operand type E of the forward), one wave per
// token row, the 64 lanes' partial sums combined by a fixed butterfly; optionally ctx as fp32 (the proj weight gradient's input).
template <int E>
__device__ __forceinline__ float ctx_elem(const void *ctx, size_t row, int D, int c) {
    if (E == 0) return (float)((const bf16 *)ctx)[row * D + c];
    if (E == 1) return ((const float *)ctx)[row * D + c];
    const char *p = (const char *)ctx + row * (size_t)D * 4 + sp_off(c);
    return (float)*(const bf16 *)p + (float)*(const bf16 *)(p + 64);
}

template <int E>
__global__ __launch_bounds__(256) void attn_bwd_delta_kernel(const void *__restrict__ ctx, const float *__restrict__ dctx,
                                                             float *__restrict__ delta, float *__restrict__ ctx32, int rows,
                                                             int N, int H, int HD) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int D = H * HD, b = row / N, n = row - b * N;
    for (int hh = 0; hh < H; ++hh) {
        float acc = 0.f;
        for (int d = lane; d < HD; d += 64) {
            const int c = hh * HD + d;
            const float o = ctx_elem<E>(ctx, row, D, c);
            if (ctx32) ctx32[(size_t)row * D + c] = o;
            acc = fmaf(o, dctx[(size_t)row * D + c], acc);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (lane == 0) delta[((size_t)b * H + hh) * N + n] = acc;
    }
}

}  // namespace

// ---- C ABI (include/ocm_vit.h, "ViT encoder training") ---------------------------------------------------------------------
extern "C" int ocm_op_attention_backward_delta(int32_t precision, const void *ctx, const float *dctx, float *delta,
                                               float *ctx_f32, int32_t batch, int32_t n_tokens, int32_t heads,
                                               int32_t head_dim, void *stream) {
    if (precision != OCM_PREC_BF16 && precision != OCM_PREC_FP32 && precision != OCM_PREC_BF16X3)
        return fail(OCM_EINVAL, "bad precision %d", precision);
    if (!ctx || !dctx || !delta) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || n_tokens <= 0 || heads <= 0 || head_dim <= 0 || (heads * head_dim) % 32)
        return fail(OCM_EINVAL, "bad shape batch=%d n_tokens=%d heads=%d head_dim=%d (heads * head_dim %% 32)", batch, n_tokens,
                    heads, head_dim);
    const int rows = batch * n_tokens;
    const dim3 grid((rows + 3) / 4), block(256);
    const hipStream_t s = (hipStream_t)stream;
    if (precision == OCM_PREC_BF16)
        attn_bwd_delta_kernel<0><<<grid, block, 0, s>>>(ctx, dctx, delta, ctx_f32, rows, n_tokens, heads, head_dim);
    else if (precision == OCM_PREC_FP32)
        attn_bwd_delta_kernel<1><<<grid, block, 0, s>>>(ctx, dctx, delta, ctx_f32, rows, n_tokens, heads, head_dim);
    else
        attn_bwd_delta_kernel<2><<<grid, block, 0, s>>>(ctx, dctx, delta, ctx_f32, rows, n_tokens, heads, head_dim);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

template <int HD>
static int attention_backward(const float *qkv, const float *lse2, const float *dctx, const float *delta, float *dqkv, int B,
                              int N, int H, float scale, hipStream_t s) {
    using L = AbLds<HD>;
    static OptinMask done_kv, done_q;
    HIP_TRY(lds_optin((const void *)attn_bwd_dkdv_kernel<HD>, L::dkdv_bytes, done_kv));
    HIP_TRY(lds_optin((const void *)attn_bwd_dq_kernel<HD>, L::dq_bytes, done_q));
    const dim3 grid((N + AB_W * AB_T - 1) / (AB_W * AB_T), B * H), block(256);
    const float c2 = scale * AB_LOG2E;
    attn_bwd_dkdv_kernel<HD><<<grid, block, L::dkdv_bytes, s>>>(qkv, lse2, dctx, delta, dqkv, B, N, H, c2, scale);
    HIP_TRY(hipGetLastError());
    attn_bwd_dq_kernel<HD><<<grid, block, L::dq_bytes, s>>>(qkv, lse2, dctx, delta, dqkv, B, N, H, c2, scale);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_attention_backward(const float *qkv_f32, const float *lse2, const float *dctx, const float *delta,
                                         float *dqkv, int32_t batch, int32_t n_tokens, int32_t heads, int32_t head_dim,
                                         float scale, void *stream) {
    if (!qkv_f32 || !lse2 || !dctx || !delta || !dqkv) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || n_tokens <= 0 || heads <= 0) return fail(OCM_EINVAL, "bad shape");
    if ((int64_t)batch * heads > 65535) return fail(OCM_EINVAL, "batch * heads = %lld > 65535", (long long)batch * heads);
    const hipStream_t s = (hipStream_t)stream;
    if (head_dim == 64) return attention_backward<64>(qkv_f32, lse2, dctx, delta, dqkv, batch, n_tokens, heads, scale, s);
    if (head_dim == 128) return attention_backward<128>(qkv_f32, lse2, dctx, delta, dqkv, batch, n_tokens, heads, scale, s);
    return fail(OCM_EINVAL, "attention backward: head_dim %d (built for 64- and 128-wide heads)", head_dim);
}
