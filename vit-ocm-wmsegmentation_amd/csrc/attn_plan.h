// attn_plan.h — which flash-attention kernel launch_attention (kernels_attn.hip) runs for a shape, on what grid and with how much
// dynamic LDS, as a pure host function of integers. Plain C++17: no HIP, no element types. The launcher computes an AttnPlan and
// executes it with one switch from plan to template instantiation; ocm_attention_plan (include/ocm_vit.h) reports the same answer
// to tests and tools through the very same call, so a threshold is written — and asserted — in exactly one place
// (tests/test_attn_plan_host.py). A plan is a function of the shape and the workspace on offer alone.
#pragma once
#include <cstddef>

enum AttnKernel : int {
    ATTN_BF16_WHOLE = 0,     // attn_small_kernel: single bf16, the whole key range of one (image, head) in LDS
    ATTN_BF16_STREAM = 1,    // attn_fwd_kernel: single bf16, 64-key tiles, double-buffered
    ATTN_F32_STREAM = 2,     // attn_fwd_f32_kernel: exact-fp32 MFMA, double-buffered
    ATTN_X3_WS = 3,          // attn_fwd_x3_ws_kernel: split-bf16, the keys of one 32-query tile split over four waves
    ATTN_X3_PP = 4,          // attn_fwd_x3_pp_kernel: split-bf16, software-pipelined, three-slot K and V^T rings
    ATTN_X3_DMA = 5,         // attn_fwd_x3_dma_kernel: split-bf16, LDS-DMA ring
    ATTN_X3_DMA_KSPLIT = 6,  // ... with the key range cut into grid.z slices, then attn_merge_x3_kernel
};

struct AttnPlan {
    AttnKernel kernel;
    int waves;    // wavefronts per workgroup (32 query rows each, except ATTN_BF16_WHOLE and ATTN_X3_WS: see the kernels)
    int stages;   // LDS buffers per operand: the ring depth; 1: the whole sequence resident
    int kslices;  // key slices (grid z), 1: none
    unsigned grid_x, grid_y, grid_z;
    int lds_bytes;          // dynamic LDS of the launch (static __shared__ arrays are the kernels' own)
    size_t workspace_need;  // bytes of key-slice workspace this plan writes (0 unless ATTN_X3_DMA_KSPLIT)
};

// ---- constants the decisions rest on -----------------------------------------------------------------------------------
constexpr int ATTN_QTILE = 32;               // query rows per wavefront, keys per split-bf16 tile
constexpr int ATTN_BF16_WHOLE_MAX_N = 256;   // single bf16, 64-wide heads: the whole-sequence kernel up to here
// split-bf16, 64-wide heads: above this many tokens 8 waves per workgroup share each K / V^T tile (half the L2 -> LDS traffic
// per query; the dozen workgroups of a one-tile call at N = 197 stay on four waves: eight measured 0.65 -> 0.68 ms per forward)
constexpr int ATTN_X3_WIDE_MIN_N = 1024;
// ... and below it, fewer four-wave workgroups than this go to the wave-split kernel (one 32-query tile per workgroup)
constexpr int ATTN_X3_WS_MAX_WGS = 128;
// Key split (long sequence, few workgroups — one ViT-S/8 window per call: 60 of them, 73 key tiles each): up to four slices per
// workgroup while the grid is at most 64 / 96 / 128 workgroups (eight slices of 9-10 tiles measure slower than four of 18-19:
// 36.6 + 7.4 us against 34.3 + 5.1 us with the merge)
constexpr int ATTN_KSPLIT_MAX = 4, ATTN_KSPLIT_WGS_4 = 64, ATTN_KSPLIT_WGS_3 = 96, ATTN_KSPLIT_WGS_2 = 128;
constexpr int ATTN_KSPLIT_ROW_FLOATS = 64 + 4;  // a slice's row in the workspace: context, maximum, sum, pad (fp32)
constexpr int ATTN_WS_LDS = 4 * 2 * 2 * 8192;   // wave-split: four waves x two slots of K | V^T
constexpr int ATTN_F32_LDS_PER_CHANNEL = 4 * 256;  // fp32 streaming: K[2] | Vt[2] of 64 keys x 4 bytes, per head channel

constexpr int attn_qtiles(int n_tokens) { return (n_tokens + ATTN_QTILE - 1) / ATTN_QTILE; }
// workgroups of the 8-wave LDS-DMA kernel, which the key split goes by
constexpr long attn_wide_wgs(int batch, int n_tokens, int heads) { return (long)((attn_qtiles(n_tokens) + 7) / 8) * batch * heads; }
constexpr size_t attn_ksplit_slice_bytes(int batch, int n_tokens, int heads) {
    return (size_t)batch * heads * n_tokens * ATTN_KSPLIT_ROW_FLOATS * sizeof(float);
}

// bytes of key-slice workspace a caller should offer at this size (0: the shape never splits the key range): room for the
// deepest split, whichever depth the plan then takes
constexpr size_t attn_plan_workspace_bytes(int prec, int batch, int n_tokens, int heads, int head_dim) {
    if (prec != 2 || head_dim != 64 || n_tokens <= ATTN_X3_WIDE_MIN_N) return 0;
    if (attn_wide_wgs(batch, n_tokens, heads) > ATTN_KSPLIT_WGS_2) return 0;
    return ATTN_KSPLIT_MAX * attn_ksplit_slice_bytes(batch, n_tokens, heads);
}

// prec: 0 bf16, 1 fp32, 2 split-bf16 pairs; head_dim 64 or 128 (the caller checks); workspace_bytes: what the caller offers for
// key slices (0: none).
inline AttnPlan attn_plan(int prec, int batch, int n_tokens, int heads, int head_dim, size_t workspace_bytes) {
    const int qtiles = attn_qtiles(n_tokens);
    const unsigned bh = (unsigned)(batch * heads), gx4 = (unsigned)((qtiles + 3) / 4);
    if (prec == 0) {
        // 128-wide heads: the streaming kernel at every sequence length; 64-wide: the whole-sequence kernel up to 256 tokens
        if (head_dim == 64 && n_tokens <= ATTN_BF16_WHOLE_MAX_N) return AttnPlan{ATTN_BF16_WHOLE, 8, 1, 1, bh, 1, 1, 0, 0};
        return AttnPlan{ATTN_BF16_STREAM, 4, 2, 1, gx4, bh, 1, 0, 0};
    }
    if (prec == 1) return AttnPlan{ATTN_F32_STREAM, 4, 2, 1, gx4, bh, 1, ATTN_F32_LDS_PER_CHANNEL * head_dim, 0};
    // 128-wide heads (model.py:93-103): four wavefronts, two stages
    if (head_dim == 128) return AttnPlan{ATTN_X3_DMA, 4, 2, 1, gx4, bh, 1, 0, 0};
    if (n_tokens > ATTN_X3_WIDE_MIN_N) {
        const unsigned gx8 = (unsigned)((qtiles + 7) / 8);
        if (workspace_bytes) {
            const long wgs = (long)gx8 * bh;
            const int want = wgs <= ATTN_KSPLIT_WGS_4 ? 4 : wgs <= ATTN_KSPLIT_WGS_3 ? 3 : wgs <= ATTN_KSPLIT_WGS_2 ? 2 : 1;
            const int per = (qtiles + want - 1) / want, nslice = (qtiles + per - 1) / per;  // every slice owns >= 1 tile
            const size_t need = (size_t)nslice * attn_ksplit_slice_bytes(batch, n_tokens, heads);
            if (nslice > 1 && need <= workspace_bytes) return AttnPlan{ATTN_X3_DMA_KSPLIT, 8, 3, nslice, gx8, bh, (unsigned)nslice, 0, need};
        }
        return AttnPlan{ATTN_X3_DMA, 8, 3, 1, gx8, bh, 1, 0, 0};
    }
    // a handful of workgroups (one tile per call): the keys of a 32-query tile split over the four waves of a workgroup;
    // otherwise the software-pipelined kernel
    if ((long)gx4 * bh < ATTN_X3_WS_MAX_WGS) return AttnPlan{ATTN_X3_WS, 4, 2, 1, (unsigned)qtiles, bh, 1, ATTN_WS_LDS, 0};
    return AttnPlan{ATTN_X3_PP, 4, 3, 1, gx4, bh, 1, 0, 0};
}
