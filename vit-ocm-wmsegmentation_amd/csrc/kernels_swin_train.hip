// kernels_swin_train.hip — the Swin-specific pieces of SwinForImageClassification's backward (modeling_swin.py, the model
// Allen_data_Backbone/train.py fine-tunes). The rest of the Swin backward reuses the ViT training operators (ocm_op_linear for
// data gradients, ocm_op_weight_grad, ocm_op_layernorm_backward, ocm_op_gelu_backward, ocm_op_patch_unfold):
//   swin_wattn_bwd_kernel      (shifted-)window attention backward, one wavefront per (image, window, head): S = q k^T / sqrt(32)
//                              + bias + shift mask and P = softmax(S) recomputed in fp32 from the fp32 q | k | v; dQ, dK, dV of
//                              the window's tokens (each token lies in exactly one window: one writer per output) and the
//                              window's dS summed into the (2ws-1)^2 relative-position bins
//   swin_wattn_bwd_wide_kernel the same contract for windows of 8 to 12 (64 .. 144 positions): one workgroup of ceil(ws^2 / 32)
//                              wavefronts per (image, window, head), all five products on the exact-fp32 MFMA
//   swin_colsum_kernel         fixed-order column sums: the per-window bin partials -> the table gradient, in two levels
//   swin_merge_gather_kernel   SwinPatchMerging's 2 x 2 gather (x0 | x1 | x2 | x3) as fp32 rows: the merging LayerNorm's input
//   swin_merge_scatter_kernel  its inverse in gather form (a permutation: bit exact)
//   swin_crop_rows_kernel      the padded geometries: rows of a grid padded to the window back to the grid (the pad is the
//                              engine's swin_pad_rows_kernel), 16-byte pieces in any element format
//   swin_merge_gather_pad_kernel / _scatter_pad  the gather for any sides (an odd side gets a zero row / column) and its
//                              transpose, 16-byte pieces
//   swin_pool_kernel / _bwd    the token mean of the final LayerNorm's output and its broadcast backward
//   swin_drop_path_kernel      residual + per-image-scaled branch (SwinDropPath), and the branch's gradient
// No atomics anywhere: every sum has one order fixed by the shapes, so reruns give the same bits.
#include "../../include/ocm_swin.h"
#include "host_common.h"
#include "launch.h"
#include "swin_geom.h"

#define fail ocm_fail

namespace {

constexpr int WB_A = 49;      // positions of the largest window (7 x 7)
constexpr int WB_LD = 33;     // LDS row of one 32-wide head, padded: a lane-strided row read hits 32 different banks
constexpr int WB_CHUNK = 64;  // windows per first-level chunk of the table-gradient sum

// One wavefront (= workgroup) per (image, window, head); lane i owns query i in the first pass and key i in the second.
//   pass 1 (query rows): S_i. = q_i K^T scale + bias + mask (-100, transformers' additive mask), P_i. = softmax,
//                        o_i = P_i. V, delta_i = dO_i . o_i, dS_ij = P_ij (dO_i . v_j - delta_i), dQ_i = scale sum_j dS_ij k_j
//   pass 2 (key rows):   dK_j = scale sum_i dS_ij q_i,  dV_j = sum_i P_ij dO_i
//   pass 3 (bins):       part[window][bin][head] = sum of dS_ij over the pairs (i, j) of that relative offset
// Every sum runs in position order. q, k, v, dO of the window and P, dS live in LDS (44 KB); all products are fp32 FMAs.
__global__ __launch_bounds__(64) void swin_wattn_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ dctx,
                                                            const float *__restrict__ table, float *__restrict__ dqkv,
                                                            float *__restrict__ part, WinGeom g, float scale) {
    __shared__ float Qs[WB_A * WB_LD], Ks[WB_A * WB_LD], Vs[WB_A * WB_LD], Gs[WB_A * WB_LD];
    __shared__ float Ps[WB_A * WB_A], Ds[WB_A * WB_A];
    __shared__ size_t Tok[64];
    __shared__ int Rg[64];
    const int lane = threadIdx.x;
    const int id = blockIdx.x;
    const auto [head, b, wy, wx] = win_decode(g, id, g.heads);
    const int ws = g.ws, A = ws * ws, AP = A | 1, C = g.heads * 32, ld = 3 * C, nb = 2 * ws - 1;
    const bool masked = g.shift > 0;
    if (lane < A) {
        Tok[lane] = win_token(g, ws, b, wy, wx, lane);
        Rg[lane] = masked ? win_region(g, ws, wy, wx, lane) : 0;
    }
    __syncthreads();
    for (int idx = lane; idx < A * 32; idx += 64) {
        const int p = idx >> 5, d = idx & 31;
        const float *row = qkv + Tok[p] * ld + head * 32 + d;
        Qs[p * WB_LD + d] = row[0];
        Ks[p * WB_LD + d] = row[C];
        Vs[p * WB_LD + d] = row[2 * C];
        Gs[p * WB_LD + d] = dctx[Tok[p] * C + head * 32 + d];
    }
    __syncthreads();
    if (lane < A) {
        const int i = lane;
        float *prow = Ps + i * AP, *drow = Ds + i * AP;
        float mx = -INFINITY;
        for (int j = 0; j < A; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 32; ++d) s = fmaf(Qs[i * WB_LD + d], Ks[j * WB_LD + d], s);
            s = s * scale + table[rel_bias_index(ws, g.heads, i, j, head)];
            if (masked && Rg[j] != Rg[i]) s += -100.0f;
            prow[j] = s;
            mx = fmaxf(mx, s);
        }
        float l = 0.f;
        for (int j = 0; j < A; ++j) {
            const float e = expf(prow[j] - mx);
            prow[j] = e;
            l += e;
        }
        const float inv = 1.0f / l;
        float o[32];
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] = 0.f;
        for (int j = 0; j < A; ++j) {
            const float p = prow[j] * inv;
            prow[j] = p;
#pragma unroll
            for (int d = 0; d < 32; ++d) o[d] = fmaf(p, Vs[j * WB_LD + d], o[d]);
        }
        float delta = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) delta = fmaf(Gs[i * WB_LD + d], o[d], delta);
        float dq[32];
#pragma unroll
        for (int d = 0; d < 32; ++d) dq[d] = 0.f;
        for (int j = 0; j < A; ++j) {
            float dp = 0.f;
#pragma unroll
            for (int d = 0; d < 32; ++d) dp = fmaf(Gs[i * WB_LD + d], Vs[j * WB_LD + d], dp);
            const float ds = prow[j] * (dp - delta);
            drow[j] = ds;
#pragma unroll
            for (int d = 0; d < 32; ++d) dq[d] = fmaf(ds, Ks[j * WB_LD + d], dq[d]);
        }
        float *dst = dqkv + Tok[i] * ld + head * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4)
            *(f32x4 *)(dst + d) = f32x4{dq[d] * scale, dq[d + 1] * scale, dq[d + 2] * scale, dq[d + 3] * scale};
    }
    __syncthreads();
    if (lane < A) {
        const int j = lane;
        float dk[32], dv[32];
#pragma unroll
        for (int d = 0; d < 32; ++d) dk[d] = dv[d] = 0.f;
        for (int i = 0; i < A; ++i) {
            const float ds = Ds[i * AP + j], p = Ps[i * AP + j];
#pragma unroll
            for (int d = 0; d < 32; ++d) {
                dk[d] = fmaf(ds, Qs[i * WB_LD + d], dk[d]);
                dv[d] = fmaf(p, Gs[i * WB_LD + d], dv[d]);
            }
        }
        float *dst = dqkv + Tok[j] * ld + head * 32;
#pragma unroll
        for (int d = 0; d < 32; d += 4) {
            *(f32x4 *)(dst + C + d) = f32x4{dk[d] * scale, dk[d + 1] * scale, dk[d + 2] * scale, dk[d + 3] * scale};
            *(f32x4 *)(dst + 2 * C + d) = f32x4{dv[d], dv[d + 1], dv[d + 2], dv[d + 3]};
        }
    }
    const int nbb = nb * nb;
    float *prt = part + ((size_t)b * g.nW + wy * g.nWx + wx) * nbb * g.heads + head;
    for (int bin = lane; bin < nbb; bin += 64) {
        const int ry = bin / nb - (ws - 1), rx = bin % nb - (ws - 1);  // yi - yj, xi - xj
        float s = 0.f;
        for (int i = 0; i < A; ++i) {
            const int yi = i / ws, xi = i - yi * ws, yj = yi - ry, xj = xi - rx;
            if (yj >= 0 && yj < ws && xj >= 0 && xj < ws) s += Ds[i * AP + yj * ws + xj];
        }
        prt[(size_t)bin * g.heads] = s;
    }
}

// out[r][c] = sum of in[row][c] over rows [r * chunk, min(rows, (r + 1) * chunk)), in row order
__global__ __launch_bounds__(256) void swin_colsum_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t rows,
                                                          int cols, int64_t chunk) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    float s = 0.f;
    for (int64_t r = r0; r < r1; ++r) s += in[r * cols + c];
    out[(size_t)blockIdx.y * cols + c] = s;
}

// ---- windows of 8 to 12 (A = ws^2 = 64 .. 144 positions): swin_wattn_bwd_wide_kernel ---------------------------------------
// One workgroup of NT = ceil(A / 32) wavefronts (2, 3, 4, 4, 5) per (image, window, head), the contract of swin_wattn_bwd_kernel.
// All five products run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) in the lane layouts of swin_wide_kernel's fp32 path.
//   stage    q, k, v, dO of the window -> LDS once, [KP = 32 NT][33] floats each, rows >= A exact zeros; per key one int
//            (offset of the key inside the bin grid | mask region << 16, negative for a padding key) and the head's table
//   phase 1  wave w owns queries 32 w .. 32 w + 31 (lane & 31 = query, registers = keys): S^T = K Q^T and dP^T = V dO^T for all
//            NT key tiles stay in 2 x NT x 16 accumulators; scale + bias + the additive -100 mask, the exact two-pass softmax
//            and delta_i = sum_j P_ij dP_ij run on them (in-register sums, one lane <-> lane + 32 exchange each); P of padding
//            keys and padding queries is an exact zero; dS = P (dP - delta) in place; dQ^T = K^T dS^T feeds from the registers
//   phase 2  dK and dV sum over queries, which span the waves: for q = 0 .. NT - 1 wave q writes its P rows ([32 queries]
//            [KP + 1] floats) into one half of the row buffer; after the barrier wave w adds query tile q to key tile w,
//            dV^T += dO^T P (keys on the lanes). A second walk does the same with dS: dK^T += Q^T dS, and thread (ry, rx) adds
//            the tile's dS entries of its up to four relative-position bins, queries in order. (Two walks, not one, so that P's
//            registers are free before dK's are taken: NT = 5 has 256 registers a wave.) The halves alternate from step to
//            step: a wave that writes a half has passed the barrier all waves reached after last reading it.
// Every sum has one order fixed by the shapes. LDS: 4 x KP x 132 + 2 x 32 x (KP + 1) x 4 + KP x 8 + 2 176 bytes.
constexpr int WW_BINS = 544;  // floats of the head's table in LDS: (2 ws - 1)^2 <= 529
static inline int wwide_lds(int nt) {
    const int kp = nt * 32;
    return 4 * kp * WB_LD * 4 + 2 * 32 * (kp + 1) * 4 + kp * 8 + WW_BINS * 4;
}

// registers of key tile t that hold padding keys in both lane halves (acc_row32(e, 1) = acc_row32(e, 0) + 4): compile-time zeros
constexpr bool wwide_dead(int A, int t, int e) { return t * 32 + (e & 3) + 8 * (e >> 2) >= A; }

// WS is a template argument: the divisions by the window become multiplies and the 16 registers of ws 12's last key tile that
// hold only padding keys (keys 144 .. 159) drop out, which is what lets NT = 5 fit its 256 registers a wave.
template <int WS>
__global__ __launch_bounds__((WS * WS + 31) / 32 * 64) void swin_wattn_bwd_wide_kernel(
    const float *__restrict__ qkv, const float *__restrict__ dctx, const float *__restrict__ table, float *__restrict__ dqkv,
    float *__restrict__ part, WinGeom g, float scale) {
    constexpr int NT = (WS * WS + 31) / 32, KP = NT * 32, NTHR = NT * 64, LDR = KP + 1, ws = WS, A = WS * WS;
    extern __shared__ __attribute__((aligned(16))) char wwide_smem[];
    int *Tok = (int *)wwide_smem;  // [KP] token of each window position (the host bounds tokens * 96 * heads by 2^31)
    int *Kinfo = Tok + KP;         // [KP]
    float *Tb = (float *)(Kinfo + KP);  // [WW_BINS] the head's table x log2(e)
    float *Qs = Tb + WW_BINS, *Ks = Qs + KP * WB_LD, *Vs = Ks + KP * WB_LD, *Gs = Vs + KP * WB_LD;
    float *Rb = Gs + KP * WB_LD;  // the row buffer: two halves of [32 queries][LDR], P or dS of one query tile each
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int id = blockIdx.x;
    const auto [head, b, wy, wx] = win_decode(g, id, g.heads);
    const int C = g.heads * 32, ld = 3 * C;
    constexpr int nb = 2 * ws - 1, nbb = nb * nb;
    const bool masked = win_masked(g, ws, wy, wx);

    for (int j = tid; j < KP; j += NTHR) {
        int info = (int)0x80000000;
        int tok = 0;
        if (j < A) {
            const int py = j / ws, px = j - py * ws;
            info = (py * nb + px) | (masked ? win_region(g, ws, wy, wx, j) << 16 : 0);
            tok = (int)win_token(g, ws, b, wy, wx, j);
        }
        Kinfo[j] = info;
        Tok[j] = tok;
    }
    constexpr float LOG2E = 1.4426950408889634f;  // scores in the log2 domain, as swin_wide_kernel keeps them
    for (int i = tid; i < WW_BINS; i += NTHR) Tb[i] = i < nbb ? table[(size_t)i * g.heads + head] * LOG2E : 0.f;
    __syncthreads();
    for (int idx = tid; idx < KP * 8; idx += NTHR) {
        const int p = idx >> 3, ch = (idx & 7) * 4;
        f32x4 q4 = {0.f, 0.f, 0.f, 0.f}, k4 = q4, v4 = q4, g4 = q4;
        if (p < A) {
            const float *row = qkv + Tok[p] * ld + head * 32 + ch;
            q4 = *(const f32x4 *)row;
            k4 = *(const f32x4 *)(row + C);
            v4 = *(const f32x4 *)(row + 2 * C);
            g4 = *(const f32x4 *)(dctx + Tok[p] * C + head * 32 + ch);
        }
        const int o = p * WB_LD + ch;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            Qs[o + e] = q4[e];
            Ks[o + e] = k4[e];
            Vs[o + e] = v4[e];
            Gs[o + e] = g4[e];
        }
    }
    __syncthreads();

    // phase 1: the wave's 32 query rows against all keys
    const int qi = wave * 32 + r, qc = min(qi, A - 1);
    const bool qlive = qi < A;
    f32x16 S[NT], D[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) S[t][e] = 0.f;
        const float *kr = Ks + (t * 32 + r) * WB_LD + h, *qr = Qs + qi * WB_LD + h;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) S[t] = mfma32f(kr[2 * kk], qr[2 * kk], S[t]);
    }
    {
        const int qy = qc / ws, qx = qc - qy * ws;
        const int qoff = (qy + ws - 1) * nb + qx + ws - 1;  // bin(query, key) = qoff - off(key): rel_bias_index without the head
        const int myreg = (Kinfo[qc] >> 16) & 0xff;
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ki = Kinfo[t * 32 + acc_row32(e, h)];
                float v = fmaf(S[t][e], scale * LOG2E, Tb[ki < 0 ? 0 : qoff - (ki & 0xffff)]);
                if (masked && ((ki >> 16) & 0xff) != myreg) v += -100.0f * LOG2E;
                if (ki < 0) v = -1e30f;
                S[t][e] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float l = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const bool pad = wwide_dead(A, t, e) || t * 32 + acc_row32(e, h) >= A;
                const float p = pad ? 0.f : fast_exp2(S[t][e] - mx);
                S[t][e] = p;
                l += p;
            }
        l += __shfl_xor(l, 32, 64);
        const float inv = qlive ? 1.0f / l : 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {  // dP^T only now: the softmax above runs with half the accumulators live
#pragma unroll
            for (int e = 0; e < 16; ++e) D[t][e] = 0.f;
            const float *vr = Vs + (t * 32 + r) * WB_LD + h, *gr = Gs + qi * WB_LD + h;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) D[t] = mfma32f(vr[2 * kk], gr[2 * kk], D[t]);
        }
        float delta = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                S[t][e] *= inv;
                if (!wwide_dead(A, t, e)) delta = fmaf(S[t][e], D[t][e], delta);
            }
        delta += __shfl_xor(delta, 32, 64);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) D[t][e] = wwide_dead(A, t, e) ? 0.f : S[t][e] * (D[t][e] - delta);
    }
    {
        f32x16 O;
#pragma unroll
        for (int e = 0; e < 16; ++e) O[e] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (!wwide_dead(A, t, e)) O = mfma32f(Ks[(t * 32 + acc_row32(e, h)) * WB_LD + r], D[t][e], O);
        if (qlive) {
            const int dst = Tok[qi] * ld + head * 32 + 4 * h;
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                *(f32x4 *)(dqkv + dst + 8 * gq) =
                    f32x4{O[4 * gq] * scale, O[4 * gq + 1] * scale, O[4 * gq + 2] * scale, O[4 * gq + 3] * scale};
        }
    }

    // phase 2: key tile `wave`, query tile by query tile; the two halves of the row buffer alternate, so one barrier a step
    const int kj = wave * 32 + r;
    const int kdst = Tok[kj] * ld + head * 32 + 4 * h;  // (Tok of a padding key is 0: not written)
    {
        f32x16 dV;
#pragma unroll
        for (int e = 0; e < 16; ++e) dV[e] = 0.f;
        for (int q = 0; q < NT; ++q) {
            float *buf = Rb + (q & 1) * (32 * LDR);
            if (wave == q) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) buf[r * LDR + t * 32 + acc_row32(e, h)] = S[t][e];
            }
            __syncthreads();
            const float *gr = Gs + (q * 32 + h) * WB_LD + r, *pr = buf + h * LDR + wave * 32 + r;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) dV = mfma32f(gr[2 * kk * WB_LD], pr[2 * kk * LDR], dV);
        }
        if (kj < A) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                *(f32x4 *)(dqkv + kdst + 2 * C + 8 * gq) = f32x4{dV[4 * gq], dV[4 * gq + 1], dV[4 * gq + 2], dV[4 * gq + 3]};
        }
    }
    // Bins: thread (ry, rx) in [0, ws)^2 owns the offsets dy in {ry, ry - ws} x dx in {rx, rx - ws} — up to four bins that share
    // exactly A (query, key) pairs: query (yi, xi) meets key ((yi - ry) mod ws, (xi - rx) mod ws), and whether a coordinate
    // wrapped says which of the four. Every thread reads one entry per query, none is skipped, each bin sums in query order.
    const int ry = tid / ws, rx = tid - ry * ws;
    float b00 = 0.f, b01 = 0.f, b10 = 0.f, b11 = 0.f;  // [dy wrapped][dx wrapped]
    {
        f32x16 dK;
#pragma unroll
        for (int e = 0; e < 16; ++e) dK[e] = 0.f;
        for (int q = 0; q < NT; ++q) {
            float *buf = Rb + ((NT + q) & 1) * (32 * LDR);
            if (wave == q) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) buf[r * LDR + t * 32 + acc_row32(e, h)] = D[t][e];
            }
            __syncthreads();
            const float *qr = Qs + (q * 32 + h) * WB_LD + r, *dr = buf + h * LDR + wave * 32 + r;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) dK = mfma32f(qr[2 * kk * WB_LD], dr[2 * kk * LDR], dK);
            const int i1 = min(A, q * 32 + 32);
            if (tid < A) {
                int yi = (q * 32) / ws, xi = q * 32 - yi * ws;
#pragma unroll 8
                for (int i = q * 32; i < i1; ++i) {
                    const bool wy = yi < ry, wx = xi < rx;
                    const int yj = yi - ry + (wy ? ws : 0), xj = xi - rx + (wx ? ws : 0);
                    const float v = buf[(i - q * 32) * LDR + yj * ws + xj];
                    b00 += !wy && !wx ? v : 0.f;
                    b01 += !wy && wx ? v : 0.f;
                    b10 += wy && !wx ? v : 0.f;
                    b11 += wy && wx ? v : 0.f;
                    if (++xi == ws) xi = 0, ++yi;
                }
            }
        }
        if (kj < A) {
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                *(f32x4 *)(dqkv + kdst + C + 8 * gq) =
                    f32x4{dK[4 * gq] * scale, dK[4 * gq + 1] * scale, dK[4 * gq + 2] * scale, dK[4 * gq + 3] * scale};
        }
    }
    float *prt = part + ((size_t)b * g.nW + wy * g.nWx + wx) * nbb * g.heads + head;
    if (tid < A) {  // bin = (dy + ws - 1) (2 ws - 1) + dx + ws - 1; the wrapped offsets exist for ry, rx >= 1
        const int by = ry + ws - 1, bx = rx + ws - 1;
        prt[(size_t)(by * nb + bx) * g.heads] = b00;
        if (rx) prt[(size_t)(by * nb + bx - ws) * g.heads] = b01;
        if (ry) prt[(size_t)((by - ws) * nb + bx) * g.heads] = b10;
        if (ry && rx) prt[(size_t)((by - ws) * nb + bx - ws) * g.heads] = b11;
    }
}

// y[(b, i, j)][q * C + c] = x[b][2i + (q & 1)][2j + (q >> 1)][c]: the x0 | x1 | x2 | x3 order of SwinPatchMerging
__global__ __launch_bounds__(256) void swin_merge_gather_kernel(const float *__restrict__ x, float *__restrict__ y, int H, int W,
                                                                int C, size_t total) {
    const int H2 = H / 2, W2 = W / 2, C4 = 4 * C;
    for (size_t n = (size_t)blockIdx.x * 256 + threadIdx.x; n < total; n += (size_t)gridDim.x * 256) {
        const int k = (int)(n % C4);
        const size_t t = n / C4;
        const int j = (int)(t % W2), i = (int)((t / W2) % H2);
        const size_t b = t / ((size_t)W2 * H2);
        const int q = k / C, c = k - q * C;
        y[n] = x[((b * H + 2 * i + (q & 1)) * W + 2 * j + (q >> 1)) * C + c];
    }
}

// dx[b][y][x][c] = dy[(b, y / 2, x / 2)][((x & 1) * 2 + (y & 1)) * C + c]
__global__ __launch_bounds__(256) void swin_merge_scatter_kernel(const float *__restrict__ dy, float *__restrict__ dx, int H,
                                                                 int W, int C, size_t total) {
    const int H2 = H / 2, W2 = W / 2;
    for (size_t n = (size_t)blockIdx.x * 256 + threadIdx.x; n < total; n += (size_t)gridDim.x * 256) {
        const int c = (int)(n % C);
        const size_t t = n / C;
        const int xx = (int)(t % W), yy = (int)((t / W) % H);
        const size_t b = t / ((size_t)W * H);
        const int q = (xx & 1) * 2 + (yy & 1);
        dx[n] = dy[((b * H2 + yy / 2) * W2 + xx / 2) * (size_t)(4 * C) + q * C + c];
    }
}

// pooled[b][c] = (sum_l x[b][l][c]) / L, tokens in order
__global__ __launch_bounds__(256) void swin_pool_kernel(const float *__restrict__ x, float *__restrict__ pooled, int L, int C,
                                                        int total) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= total) return;
    const int c = n % C, b = n / C;
    const float *src = x + (size_t)b * L * C + c;
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += src[(size_t)l * C];
    pooled[n] = s / (float)L;
}

// dx[b][l][c] = dpooled[b][c] / L
__global__ __launch_bounds__(256) void swin_pool_bwd_kernel(const float *__restrict__ dp, float *__restrict__ dx, int L, int C,
                                                            size_t total) {
    for (size_t n = (size_t)blockIdx.x * 256 + threadIdx.x; n < total; n += (size_t)gridDim.x * 256) {
        const int c = (int)(n % C);
        const size_t b = n / ((size_t)L * C);
        dx[n] = dp[b * C + c] / (float)L;
    }
}

// out = x + branch * scale[image] (out may alias x); the backward passes x = nullptr: out = branch * scale[image]
__global__ __launch_bounds__(256) void swin_drop_path_kernel(const float *x, const float *__restrict__ branch,
                                                             const float *__restrict__ scale, float *out, size_t per_image,
                                                             size_t total) {
    for (size_t n = (size_t)blockIdx.x * 256 + threadIdx.x; n < total; n += (size_t)gridDim.x * 256) {
        const float v = branch[n] * scale[n / per_image];
        out[n] = x ? x[n] + v : v;
    }
}

// SwinLayer.maybe_pad's inverse: rows (B, Hp, Wp, row) -> (B, H, W, row) in 16-byte pieces (the pad itself is kernels_swin.hip's
// swin_pad_rows_kernel, which the engine runs too)
__global__ __launch_bounds__(256) void swin_crop_rows_kernel(const f32x4 *__restrict__ src, f32x4 *__restrict__ dst, int H, int W,
                                                             int Hp, int Wp, int chunks, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / chunks;
        const int c = (int)(i - row * chunks);
        const size_t b = row / ((size_t)H * W);
        const int rem = (int)(row - b * H * W), y = rem / W, xx = rem - y * W;
        dst[i] = src[((b * Hp + y) * Wp + xx) * (size_t)chunks + c];
    }
}

// swin_merge_gather_kernel for any sides (SwinPatchMerging.maybe_pad: an odd side gets one zero row / column), in 16-byte
// pieces: C4 = C / 4 pieces per channel row, zeros where the 2 x 2 neighbourhood leaves the grid
__global__ __launch_bounds__(256) void swin_merge_gather_pad_kernel(const f32x4 *__restrict__ x, f32x4 *__restrict__ y, int H,
                                                                    int W, int C4, size_t total) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2, K4 = 4 * C4;
    for (size_t n = (size_t)blockIdx.x * 256 + threadIdx.x; n < total; n += (size_t)gridDim.x * 256) {
        const int k = (int)(n % K4);
        const size_t t = n / K4;
        const int j = (int)(t % W2), i = (int)((t / W2) % H2);
        const size_t b = t / ((size_t)W2 * H2);
        const int q = k / C4, c = k - q * C4;
        const int yy = 2 * i + (q & 1), xx = 2 * j + (q >> 1);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (yy < H && xx < W) v = x[((b * H + yy) * W + xx) * (size_t)C4 + c];
        y[n] = v;
    }
}

// its transpose in gather form: every dx element has exactly one source; what dy holds at the appended row / column is not read
__global__ __launch_bounds__(256) void swin_merge_scatter_pad_kernel(const f32x4 *__restrict__ dy, f32x4 *__restrict__ dx, int H,
                                                                     int W, int C4, size_t total) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2;
    for (size_t n = (size_t)blockIdx.x * 256 + threadIdx.x; n < total; n += (size_t)gridDim.x * 256) {
        const int c = (int)(n % C4);
        const size_t t = n / C4;
        const int xx = (int)(t % W), yy = (int)((t / W) % H);
        const size_t b = t / ((size_t)W * H);
        const int q = (xx & 1) * 2 + (yy & 1);
        dx[n] = dy[((b * H2 + yy / 2) * W2 + xx / 2) * (size_t)(4 * C4) + q * C4 + c];
    }
}

unsigned grid_for(size_t work) {
    const size_t g = (work + 255) / 256;
    return (unsigned)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

int wb_geometry_ok(int batch, int height, int width, int window, int shift, int heads) {
    if (batch <= 0 || heads <= 0 || window < 2 || window > 7 || height <= 0 || width <= 0 || height % window ||
        width % window || shift < 0 || shift >= window)
        return fail(OCM_EINVAL, "bad window geometry (batch %d, %d x %d, window %d, shift %d, heads %d)", batch, height, width,
                    window, shift, heads);
    if ((int64_t)batch * height * width * heads * 96 > 0x7fffffffLL) return fail(OCM_EINVAL, "too many tokens");
    return OCM_OK;
}

int shape_ok(int batch, int tokens, int channels) {
    if (batch <= 0 || tokens <= 0 || channels <= 0)
        return fail(OCM_EINVAL, "bad shape batch=%d tokens=%d channels=%d", batch, tokens, channels);
    return OCM_OK;
}

int merge_ok(int batch, int height, int width, int channels) {
    if (batch <= 0 || height <= 0 || width <= 0 || height % 2 || width % 2 || channels <= 0)
        return fail(OCM_EINVAL, "bad patch-merging geometry (batch %d, %d x %d, %d channels): even sides only", batch, height,
                    width, channels);
    return OCM_OK;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int rows_ok(const void *src, const void *dst, int batch, int height, int width, int height_pad, int width_pad,
            size_t row_bytes) {
    if (!src || !dst) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || height <= 0 || width <= 0 || height_pad < height || width_pad < width || row_bytes == 0 ||
        row_bytes % 16 || row_bytes > 0x7fffffffu)
        return fail(OCM_EINVAL, "bad padded-row geometry (batch %d, %d x %d in %d x %d, rows of %zu bytes: a positive multiple "
                    "of 16)", batch, height, width, height_pad, width_pad, row_bytes);
    if ((int64_t)height_pad * width_pad > 0x7fffffffLL) return fail(OCM_EINVAL, "too many positions per image");
    if (!aligned16(src) || !aligned16(dst)) return fail(OCM_EINVAL, "rows must be 16-byte aligned");
    return OCM_OK;
}

int merge_pad_ok(const void *a, const void *b, int batch, int height, int width, int channels) {
    if (!a || !b) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || height <= 0 || width <= 0 || channels <= 0 || channels % 4)
        return fail(OCM_EINVAL, "bad patch-merging geometry (batch %d, %d x %d, %d channels): positive sides, channels a "
                    "multiple of 4", batch, height, width, channels);
    if (!aligned16(a) || !aligned16(b)) return fail(OCM_EINVAL, "rows must be 16-byte aligned");
    return OCM_OK;
}

}  // namespace

// ---- C ABI (include/ocm_swin.h, training) ------------------------------------------------------------------------------
extern "C" size_t ocm_swin_window_attention_backward_workspace_bytes(int32_t batch, int32_t height, int32_t width,
                                                                     int32_t window, int32_t heads) {
    if (batch <= 0 || height <= 0 || width <= 0 || window < 2 || window > 7 || heads <= 0) return 0;
    const int64_t nwin = (int64_t)batch * (height / window) * (width / window);
    const int64_t cols = (int64_t)(2 * window - 1) * (2 * window - 1) * heads;
    const int64_t R = (nwin + WB_CHUNK - 1) / WB_CHUNK;
    return (size_t)((nwin + R) * cols) * sizeof(float);
}

extern "C" int ocm_op_swin_window_attention_backward(const float *qkv, const float *dctx, const float *rel_table, float *dqkv,
                                                     float *dtable, int32_t batch, int32_t height, int32_t width, int32_t window,
                                                     int32_t shift, int32_t heads, void *workspace, size_t workspace_bytes,
                                                     void *stream) {
    if (!qkv || !dctx || !rel_table || !dqkv || !dtable || !workspace) return fail(OCM_EINVAL, "null argument");
    if (int rc = wb_geometry_ok(batch, height, width, window, shift, heads)) return rc;
    const size_t need = ocm_swin_window_attention_backward_workspace_bytes(batch, height, width, window, heads);
    if (workspace_bytes < need)
        return fail(OCM_EINVAL, "window attention backward workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const WinGeom g{height, width, window, shift, width / window, (height / window) * (width / window), heads};
    const int64_t nwin = (int64_t)batch * g.nW, total = nwin * heads;
    const int cols = (2 * window - 1) * (2 * window - 1) * heads;
    const int64_t R = (nwin + WB_CHUNK - 1) / WB_CHUNK;
    if (total > 0x7fffffffLL || R > 65535) return fail(OCM_EINVAL, "too many (window, head) pairs");
    float *part = (float *)workspace, *part2 = part + nwin * cols;
    swin_wattn_bwd_kernel<<<dim3((unsigned)total), dim3(64), 0, s>>>(qkv, dctx, rel_table, dqkv, part, g, 0.17677669529663687f);
    HIP_TRY(hipGetLastError());
    const unsigned cx = (unsigned)((cols + 255) / 256);
    swin_colsum_kernel<<<dim3(cx, (unsigned)R), dim3(256), 0, s>>>(part, part2, nwin, cols, WB_CHUNK);
    HIP_TRY(hipGetLastError());
    swin_colsum_kernel<<<dim3(cx, 1), dim3(256), 0, s>>>(part2, dtable, R, cols, R);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

template <int WS>
static hipError_t launch_wattn_bwd_wide(const float *qkv, const float *dctx, const float *table, float *dqkv, float *part,
                                        const WinGeom &g, unsigned total, hipStream_t s) {
    static OptinMask optin;
    constexpr int NT = (WS * WS + 31) / 32;
    auto kern = swin_wattn_bwd_wide_kernel<WS>;
    if (hipError_t e = lds_optin((const void *)kern, wwide_lds(NT), optin); e != hipSuccess) return e;
    kern<<<dim3(total), dim3(NT * 64), wwide_lds(NT), s>>>(qkv, dctx, table, dqkv, part, g, 0.17677669529663687f);
    return hipGetLastError();
}

extern "C" size_t ocm_swin_window_attention_backward_wide_workspace_bytes(int32_t batch, int32_t height, int32_t width,
                                                                          int32_t window, int32_t heads) {
    if (batch <= 0 || height <= 0 || width <= 0 || window < 8 || window > 12 || heads <= 0) return 0;
    const int64_t nwin = (int64_t)batch * (height / window) * (width / window);
    const int64_t cols = (int64_t)(2 * window - 1) * (2 * window - 1) * heads;
    const int64_t R = (nwin + WB_CHUNK - 1) / WB_CHUNK;
    return (size_t)((nwin + R) * cols) * sizeof(float);
}

extern "C" int ocm_op_swin_window_attention_backward_wide(const float *qkv, const float *dctx, const float *rel_table,
                                                          float *dqkv, float *dtable, int32_t batch, int32_t height,
                                                          int32_t width, int32_t window, int32_t shift, int32_t heads,
                                                          void *workspace, size_t workspace_bytes, void *stream) {
    if (!qkv || !dctx || !rel_table || !dqkv || !dtable || !workspace) return fail(OCM_EINVAL, "null argument");
    if (batch <= 0 || heads <= 0 || window < 8 || window > 12 || height <= 0 || width <= 0 || height % window ||
        width % window || shift < 0 || shift >= window)
        return fail(OCM_EINVAL, "bad wide window geometry (batch %d, %d x %d, window %d of 8 to 12, shift %d, heads %d)", batch,
                    height, width, window, shift, heads);
    if ((int64_t)batch * height * width * heads * 96 > 0x7fffffffLL) return fail(OCM_EINVAL, "too many tokens");
    if (!aligned16(qkv) || !aligned16(dctx) || !aligned16(dqkv)) return fail(OCM_EINVAL, "rows must be 16-byte aligned");
    const size_t need = ocm_swin_window_attention_backward_wide_workspace_bytes(batch, height, width, window, heads);
    if (workspace_bytes < need)
        return fail(OCM_EINVAL, "wide window attention backward workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    const hipStream_t s = (hipStream_t)stream;
    const WinGeom g{height, width, window, shift, width / window, (height / window) * (width / window), heads};
    const int64_t nwin = (int64_t)batch * g.nW, total = nwin * heads;
    const int cols = (2 * window - 1) * (2 * window - 1) * heads;
    const int64_t R = (nwin + WB_CHUNK - 1) / WB_CHUNK;
    if (total > 0x7fffffffLL || R > 65535) return fail(OCM_EINVAL, "too many (window, head) pairs");
    float *part = (float *)workspace, *part2 = part + nwin * cols;
    switch (window) {
        case 8: HIP_TRY(launch_wattn_bwd_wide<8>(qkv, dctx, rel_table, dqkv, part, g, (unsigned)total, s)); break;
        case 9: HIP_TRY(launch_wattn_bwd_wide<9>(qkv, dctx, rel_table, dqkv, part, g, (unsigned)total, s)); break;
        case 10: HIP_TRY(launch_wattn_bwd_wide<10>(qkv, dctx, rel_table, dqkv, part, g, (unsigned)total, s)); break;
        case 11: HIP_TRY(launch_wattn_bwd_wide<11>(qkv, dctx, rel_table, dqkv, part, g, (unsigned)total, s)); break;
        default: HIP_TRY(launch_wattn_bwd_wide<12>(qkv, dctx, rel_table, dqkv, part, g, (unsigned)total, s)); break;
    }
    const unsigned cx = (unsigned)((cols + 255) / 256);
    swin_colsum_kernel<<<dim3(cx, (unsigned)R), dim3(256), 0, s>>>(part, part2, nwin, cols, WB_CHUNK);
    HIP_TRY(hipGetLastError());
    swin_colsum_kernel<<<dim3(cx, 1), dim3(256), 0, s>>>(part2, dtable, R, cols, R);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_merge_gather(const float *x, float *y, int32_t batch, int32_t height, int32_t width, int32_t channels,
                                        void *stream) {
    if (!x || !y) return fail(OCM_EINVAL, "null argument");
    if (int rc = merge_ok(batch, height, width, channels)) return rc;
    const size_t total = (size_t)batch * height * width * channels;
    swin_merge_gather_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(x, y, height, width, channels, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_merge_scatter(const float *dy, float *dx, int32_t batch, int32_t height, int32_t width,
                                         int32_t channels, void *stream) {
    if (!dy || !dx) return fail(OCM_EINVAL, "null argument");
    if (int rc = merge_ok(batch, height, width, channels)) return rc;
    const size_t total = (size_t)batch * height * width * channels;
    swin_merge_scatter_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(dy, dx, height, width, channels,
                                                                                            total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_pad_rows(const void *src, void *dst, int32_t batch, int32_t height, int32_t width, int32_t height_pad,
                                    int32_t width_pad, size_t row_bytes, void *stream) {
    if (int rc = rows_ok(src, dst, batch, height, width, height_pad, width_pad, row_bytes)) return rc;
    HIP_TRY(launch_swin_pad_rows(src, dst, batch, height, width, height_pad, width_pad, row_bytes, (hipStream_t)stream));
    return OCM_OK;
}

extern "C" int ocm_op_swin_crop_rows(const void *src, void *dst, int32_t batch, int32_t height, int32_t width,
                                     int32_t height_pad, int32_t width_pad, size_t row_bytes, void *stream) {
    if (int rc = rows_ok(src, dst, batch, height, width, height_pad, width_pad, row_bytes)) return rc;
    const int chunks = (int)(row_bytes / 16);
    const size_t total = (size_t)batch * height * width * chunks;
    swin_crop_rows_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(
        (const f32x4 *)src, (f32x4 *)dst, height, width, height_pad, width_pad, chunks, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_merge_gather_pad(const float *x, float *y, int32_t batch, int32_t height, int32_t width,
                                            int32_t channels, void *stream) {
    if (int rc = merge_pad_ok(x, y, batch, height, width, channels)) return rc;
    const size_t total = (size_t)batch * ((height + 1) / 2) * ((width + 1) / 2) * channels;  // 4 * (channels / 4) pieces a row
    swin_merge_gather_pad_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(
        (const f32x4 *)x, (f32x4 *)y, height, width, channels / 4, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_merge_scatter_pad(const float *dy, float *dx, int32_t batch, int32_t height, int32_t width,
                                             int32_t channels, void *stream) {
    if (int rc = merge_pad_ok(dy, dx, batch, height, width, channels)) return rc;
    const size_t total = (size_t)batch * height * width * (channels / 4);
    swin_merge_scatter_pad_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(
        (const f32x4 *)dy, (f32x4 *)dx, height, width, channels / 4, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_pool(const float *x, float *pooled, int32_t batch, int32_t tokens, int32_t channels, void *stream) {
    if (!x || !pooled) return fail(OCM_EINVAL, "null argument");
    if (int rc = shape_ok(batch, tokens, channels)) return rc;
    if ((int64_t)batch * channels > 0x7fffffffLL) return fail(OCM_EINVAL, "too many outputs");
    const int total = batch * channels;
    swin_pool_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream>>>(x, pooled, tokens, channels,
                                                                                                   total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_pool_backward(const float *dpooled, float *dx, int32_t batch, int32_t tokens, int32_t channels,
                                         void *stream) {
    if (!dpooled || !dx) return fail(OCM_EINVAL, "null argument");
    if (int rc = shape_ok(batch, tokens, channels)) return rc;
    const size_t total = (size_t)batch * tokens * channels;
    swin_pool_bwd_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(dpooled, dx, tokens, channels, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_drop_path(const float *x, const float *branch, const float *scale, float *out, int32_t batch,
                                     int32_t tokens, int32_t channels, void *stream) {
    if (!x || !branch || !scale || !out) return fail(OCM_EINVAL, "null argument");
    if (int rc = shape_ok(batch, tokens, channels)) return rc;
    const size_t per = (size_t)tokens * channels, total = per * batch;
    swin_drop_path_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(x, branch, scale, out, per, total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}

extern "C" int ocm_op_swin_drop_path_backward(const float *dout, const float *scale, float *dbranch, int32_t batch,
                                              int32_t tokens, int32_t channels, void *stream) {
    if (!dout || !scale || !dbranch) return fail(OCM_EINVAL, "null argument");
    if (int rc = shape_ok(batch, tokens, channels)) return rc;
    const size_t per = (size_t)tokens * channels, total = per * batch;
    swin_drop_path_kernel<<<dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream>>>(nullptr, dout, scale, dbranch, per,
                                                                                        total);
    HIP_TRY(hipGetLastError());
    return OCM_OK;
}
