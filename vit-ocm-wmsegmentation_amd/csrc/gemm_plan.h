// gemm_plan.h — which tile, main loop, ring depth and K-step count every GEMM launcher of gemm_kernels.h / kernels_conv.hip runs,
// as pure host functions of integers. Plain C++17: no HIP, no element types. The launchers compute a GemmPlan and execute it
// with one switch from plan to template instantiation; ocm_gemm_plan (include/ocm_vit.h) reports the same answer to tests and
// tools through the very same call, so a threshold is written — and asserted — in exactly one place
// (tests/test_gemm_plan_host.py). A plan is a function of the problem's shape alone: nothing forces a variant.
#pragma once

// ---- tiles -------------------------------------------------------------------------------------------------------------
// One value per GemmCfg<BM, BN, WAVES_M, WAVES_N, MF16> (gemm_core.h) the library launches; gemm_kernels.h derives its Cfg*
// typedefs from GEMM_TILES, where the measurements behind each shape are noted.
enum GemmTile : int {
    T64x64, T64x128, T64x128w, T64x256w, T64x384w, T128x96, T128x128, T128x128q, T128x128q16, T128x192, T160x128q16,
    T256x256, T256x256m16, GEMM_TILE_COUNT
};
struct GemmTileInfo {
    int bm, bn, waves_m, waves_n;
    int mf16;  // 1: split-bf16 products on v_mfma_f32_16x16x32_bf16 (GemmCfg::MF16), 0: the 32 x 32 MFMA shapes
    int max_stages;  // the deepest LDS ring any plan gives this tile
};
constexpr GemmTileInfo GEMM_TILES[GEMM_TILE_COUNT] = {
    {64, 64, 2, 2, 0, 4},   // T64x64
    {64, 128, 2, 2, 0, 4},  // T64x128
    {64, 128, 2, 4, 0, 4},  // T64x128w: eight waves for the one-tile-per-call forwards; the full-row tile of D = 128
    {64, 256, 2, 4, 0, 2},  // T64x256w: full rows of the fused residual + LayerNorm GEMM
    {64, 384, 2, 4, 0, 2},  // T64x384w
    {128, 96, 4, 1, 0, 2},  // T128x96
    {128, 128, 2, 2, 0, 2}, // T128x128
    {128, 128, 2, 4, 0, 2}, // T128x128q: eight waves
    {128, 128, 2, 4, 1, 2}, // T128x128q16
    {128, 192, 4, 2, 0, 3}, // T128x192
    {160, 128, 2, 4, 1, 3}, // T160x128q16: two stages under the two-per-CU mlp.fc1, three under the one-per-CU mlp.fc2
    {256, 256, 2, 4, 0, 2}, // T256x256
    {256, 256, 2, 4, 1, 2}, // T256x256m16
};
// every tile fits a CU: at most 16 wavefronts, and the deepest ring — stages x (BM + BN) x 128 bytes of operands plus the
// epilogues' row / column tables of (BM + BN) x 8 — within the 160 KiB of LDS
constexpr bool gemm_tiles_fit() {
    for (const GemmTileInfo &t : GEMM_TILES)
        if (t.waves_m * t.waves_n > 16 || t.max_stages * (t.bm + t.bn) * 128 + (t.bm + t.bn) * 8 > 160 * 1024) return false;
    return true;
}
static_assert(gemm_tiles_fit(), "a tile of GEMM_TILES exceeds the CU");

// ---- the plan ----------------------------------------------------------------------------------------------------------
enum GemmLoop : int { GEMM_LOOP_REG = 0, GEMM_LOOP_DMA = 1 };  // register-staged (gemm_mainloop) / LDS-DMA ring (gemm_mainloop_dma)
struct GemmPlan {
    GemmTile tile;
    GemmLoop loop;
    int stages;  // LDS buffers of (BM + BN) * 128 bytes: the ring depth of the LDS-DMA loop, 2 on the register-staged loop
    int ksteps;  // compile-time K-step count of the kernel, 0: the run-time loop
    int splitk;  // K slices (launch.h: StatsOut::part), 1: none
};
// what a launcher's switch goes by on the LDS-DMA loop
constexpr int gemm_dma_key(GemmTile tile, int stages) { return (int)tile * 16 + stages; }

// elements of one 128-byte operand row = one K step (gemm_core.h: Elem<E>::KROW), by precision: 0 bf16, 1 fp32, 2 split-bf16 pairs
constexpr int gemm_krow(int prec) { return prec == 0 ? 64 : 32; }

// ---- K depths with a compile-time step count ---------------------------------------------------------------------------
// A kernel that knows its step count unrolls gemm_mainloop's two-step prefetch; any other depth runs the generic one-step
// pipeline. Every entry is a kernel per (tile, element type, epilogue) in the library: each family lists only the depths it runs.
struct KsLinearReg {  // the K extents of ViT-S/B (D and 4 D, and the patch embedding); 2, 3: Swin stages 0 - 1 (K = 96 padded, 192 bf16 / 96 fp32)
    static constexpr int n = 8, v[n] = {2, 3, 4, 6, 12, 24, 48, 96};
};
struct KsLinearDma {  // 96: ViT-B mlp.fc2
    static constexpr int n = 5, v[n] = {6, 12, 24, 48, 96};
};
struct KsQkvReg {
    static constexpr int n = 3, v[n] = {6, 12, 24};
};
struct KsQkvDma {
    static constexpr int n = 2, v[n] = {12, 24};
};
struct KsConv3x3 {  // the 3x3 layers of the U-Net in fp32 / split pairs (C = 64, 128, 256: 18, 36, 72 steps of 32) and their bf16 forms
    static constexpr int n = 3, v[n] = {18, 36, 72};
};
struct KsNone {  // every other A loader of kernels_conv.hip
    static constexpr int n = 0, v[1] = {0};
};
template <class List>
constexpr int gemm_ct_steps(int steps) {
    for (int i = 0; i < List::n; ++i)
        if (List::v[i] == steps) return steps;
    return 0;
}

// ---- constants the decisions rest on -----------------------------------------------------------------------------------
// LDS-DMA ring depth of the 64 x 128 tiles that serve the one-tile-per-call forwards (M <= 1024 rows: a handful of
// workgroups whose K loop is a chain of L2 round trips — three steps in flight instead of one)
constexpr int OCM_SMALLM_STAGES = 4;
// ... and up to how many rows they are chosen: 4096 covers one ViT-S/8 window of 384^2 per call (2305 rows, 111 .. 444
// workgroups). With FOUR waves per tile the register-staged loop was faster there (attn.qkv 18.8 against 21.8 us, mlp.fc1 16.2
// against 17.5); with eight the LDS-DMA loop wins (the one-window forward 1.42 -> 1.28 ms)
constexpr int OCM_SMALLM_ROWS = 4096;
// Split-K (launch.h: StatsOut::part): slices, and up to how many rows (at 2305 rows, one ViT-S/8 window, the split form measures
// the same as the plain kernel). The kernel is built for slices of 12 steps: K = 4 x 384 (ViT-S mlp.fc2); other depths: no split
constexpr int OCM_SPLITK = 4, OCM_SPLITK_MAX_ROWS = 512, OCM_SPLITK_STEPS = 12;
// Ring depth of the 160 x 128 tile where it runs ONE workgroup per CU (mlp.fc2, below): 3 x 36 KiB = 108 KiB, two K steps in
// flight and no room for a second workgroup on the CU (four stages, 144 KiB, measured slower: 53.9 against 52.1 us, below)
constexpr int OCM_TALL_N384_STAGES = 3;

// 256 x 256 tiles: 8 waves, one workgroup per CU: half the L2->LDS bytes per output element of 128x128. Pays off once the
// problem has at least two full rounds of such tiles (ViT-B at 384^2, the ViT-S/8 slab windows); below
// that the idle CUs of the last round cost more than the traffic saves, and with K = 384 (six steps) the
// exposed prologue of a lone workgroup does (measured: ViT-S/8 slab fc1 +7 % slower, ViT-B GEMMs 13 % faster).
constexpr bool big_tiles_pay(int M, int N, int K) {
    return K >= 768 && N % 256 == 0 && (long)((M + 255) / 256) * (N / 256) >= 512;
}
// share of the workgroup slots that `tiles` workgroups fill, in rounds of `slots`, the last round counted by its fill
constexpr double gemm_round_fill(long tiles, long slots) { return (double)tiles / (double)(slots * ((tiles + slots - 1) / slots)); }

// a plan on either loop; `steps` K steps get a compile-time count where the family's List names it
template <class List>
constexpr GemmPlan gemm_plan_reg(GemmTile tile, int steps) { return GemmPlan{tile, GEMM_LOOP_REG, 2, gemm_ct_steps<List>(steps), 1}; }
template <class List>
constexpr GemmPlan gemm_plan_dma(GemmTile tile, int stages, int steps) {
    return GemmPlan{tile, GEMM_LOOP_DMA, stages, gemm_ct_steps<List>(steps), 1};
}

// ---- the register-staged tail every family shares ----------------------------------------------------------------------
// Tile choice: fill >= 2 workgroups per CU (256 CUs) when the problem allows it: 128 x 128 from 512 such tiles on, 64 x 128 for
// widths that are multiples of 128 with more than one row tile, else 64 x 64.
template <class List>
constexpr GemmPlan gemm_plan_reg_tail(int M, int N, int steps) {
    const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
    if (N % 128 == 0 && t128 >= 512) return gemm_plan_reg<List>(T128x128, steps);
    if (N % 128 == 0 && M > 64) return gemm_plan_reg<List>(T64x128, steps);
    return gemm_plan_reg<List>(T64x64, steps);
}

// ---- nn.Linear (launch_linear_epi, and the split-K test of launch_linear_e) --------------------------------------------
// prec 0 / 1 / 2 as above; K a multiple of gemm_krow(prec). epilogue: the MODE of EpiLinear (0 .. 4). stats_epilogue: the
// statistics-producing residual epilogue (EpiResidStats, BN_MULT = 64: tile widths that are multiples of 64 only).
// splitk_offered: the caller holds a split-K workspace and what the finishing kernel needs (a residual; pairs with the sums).
inline GemmPlan gemm_plan_linear(int prec, int epilogue, int M, int N, int K, bool stats_epilogue, bool splitk_offered) {
    const int steps = K / gemm_krow(prec);
    if (prec == 2 && epilogue == 1 && splitk_offered && M <= OCM_SPLITK_MAX_ROWS && N % 64 == 0 && steps == OCM_SPLITK * OCM_SPLITK_STEPS)
        // (the eight-wave 64 x 128 tile halves the workgroups: 0.628 -> 0.641 ms per one-tile forward)
        return GemmPlan{T64x64, GEMM_LOOP_DMA, 4, OCM_SPLITK_STEPS, OCM_SPLITK};
    const auto dma = [steps](GemmTile tile, int stages) { return gemm_plan_dma<KsLinearDma>(tile, stages, steps); };
    if (prec == 2) {
        // Split-bf16 operands, >= 512 tiles of 128x128 (fc1): LDS-DMA staging, two workgroups per CU. Inside the forward
        // (ViT-S/16, B = 64, same box, alternating runs) fc1 62 -> 57 us; the 64x128 shapes (proj, fc2) and the qkv
        // projection measure the same either way (their stand-alone gains of 10 % do not survive cold operands), so
        // they stay on the register-staged loop.
        // Few rows (the reference's one-tile-per-call loops, M = 197 .. 785): everything is L2-resident and a launch is a
        // handful of workgroups, so the LDS-DMA loop's shorter prologue shows (stand-alone, M = 197: fc1 9.4 -> 7.9 us,
        // fc2 23.1 -> 16.7 us on 64x64 tiles with a 4-deep ring, proj 8.3 -> 7.6 us)
        if (M <= OCM_SMALLM_ROWS) {
            if (K >= 1024 && N % 64 == 0) return dma(T64x64, 4);
            if (N % 128 == 0) return dma(T64x128w, OCM_SMALLM_STAGES);
        }
        // mlp.fc1 at K = 384 and tens of thousands of rows (the 4096^2 slab sweep: 48 k rows; Swin-T stage 2 at batch 256: 50 k):
        // the same 256 x 256 tile although its K loop is only twelve steps (round 4, against the eight-wave 128 x 128 tile,
        // alternating on one box: slab sweep 534.6 -> 530.6 ms, Swin-T 10.35 -> 10.27 ms; attn.qkv LOSES on it: 534.6 -> 558 ms)
        if (K == 384 && N % 256 == 0 && N >= 1024 && M >= 16384) return dma(T256x256m16, 2);
        // ViT-B at 384^2: 256x256 tiles, one 8-wave workgroup per CU (fc1 1020 -> 944 us), on v_mfma_f32_16x16x32_bf16 since
        // round 4 (B = 128, alternating runs: fc1 965 -> 870 us, fc2 903 -> 820, proj 281 -> 256)
        if (big_tiles_pay(M, N, K)) return dma(T256x256m16, 2);
        const long rb = (M + 127) / 128, t128 = rb * (N / 128);  // (t128: where N is a multiple of 128)
        // mlp.fc2 of ViT-S (N = 384, K >= 768: 24 K steps and more) in a single round of workgroups: 160 x 128 tiles on a
        // THREE-stage ring when they put the launch on at least 10 % more CUs than 128 x 192 tiles would — at 12 608 rows
        // (ViT-S/16, B = 64) 79 x 3 = 237 workgroups of 0.83 x the MFMA work per K step instead of 99 x 2 = 198. Both tilings
        // must be one round (<= 256 workgroups: up to 13 600 rows); 108 KiB of LDS keep a second workgroup off the CU.
        // In the forward, alternating on one box, the 160-row tile at each ring depth against 128 x 192: fc2 55.2 us
        // on 128 x 192 -> 61.8 on two stages, 61.9 on two stages with the LDS request padded to one workgroup per CU, 52.1 on
        // three, 53.9 on four (another box: 52.1 -> 62.6 / 61.4 / 49.6 / 50.8): the ring depth, not workgroups pairing up, was
        // what the two-stage trial of round 4 lost. Libraries alternating, twelve rounds: 2.230 -> 2.200 ms per step.
        // Rows (bench.py --batch 21 / 32 / 69 = 4 137 / 6 304 / 13 593 rows): fc2 43.6 -> 42.0, 46.0 -> 43.3, 57.3 -> 55.3 us,
        // so the rule starts where the few-row branch ends. Only the statistics-producing residual epilogue (the engine's
        // fc2) was measured and is covered; attn.proj (12 steps) stays on 128 x 192.
        if (N == 384 && steps >= 24 && epilogue == 1 && stats_epilogue && M > OCM_SMALLM_ROWS) {
            const long t160 = (long)((M + 159) / 160) * 3, t192 = rb * 2;
            if (t160 <= 256 && t192 <= 256 && 10 * t160 >= 11 * t192) return dma(T160x128q16, OCM_TALL_N384_STAGES);
        }
        // Narrow outputs (attn.proj / mlp.fc2 of ViT-S: N = 384) with too few rows for 512 tiles of 128 x 128: 128 x 192
        // tiles, one 8-wave workgroup per CU on a three-stage LDS-DMA ring. Per K step 40 KiB of operands for 1152 cycles
        // of MFMA per SIMD (56 KiB for the 64 x 384 full-row tile, 64 KiB for two 64 x 128 tiles): ViT-S/16 at B = 64,
        // in the forward, mlp.fc2 64 -> 49 us, attn.proj 28.5 -> 21.5 us against the full-row GEMM + LayerNorm kernels
        // Past 512 tiles of 128 x 128 the choice goes by how full the last round is: at 48 405 rows (the 4096^2 slab sweep) 1137
        // tiles of 128 x 128 are 2.2 rounds of 512 slots, 758 of 128 x 192 are 2.96 rounds of 256 (sweep 557.7 -> 551.3 ms); at
        // 50 176 rows (Swin-T stage 2) both shapes fill 77 % of their last round and the two-per-CU tile wins (183 against 215 us).
        if (N % 192 == 0 && N / 192 <= 2 && M >= 4096) {
            const long t192 = rb * (N / 192), t128c = rb * ((N + 127) / 128);
            if (t128c < 512 || gemm_round_fill(t192, 256) > 1.1 * gemm_round_fill(t128c, 512)) return dma(T128x192, 3);
        }
        if (N % 128 == 0 && t128 >= 512) {
            // wide outputs (mlp.fc1): the same tile on eight wavefronts, four per SIMD with two workgroups per CU (58.0 -> 56.2 us
            // in the forward on one box, 53.0 -> 51.8 on another; the N = 384 layers lose on it: fc2 56 -> 62, proj 26 -> 27, and
            // so does mlp.fc1 at 48 k rows: slab sweep 530 -> 533 ms)
            // (round 4, on the 16 x 16 MFMA shape: at 48 k rows too — slab sweep 541.8 -> 538.7 ms against the four-wave tile, which
            // on the 32 x 32 shape had been the faster one there; the four-wave tile on the 16 x 16 shape: 542.9 ms)
            // (round 4: narrower outputs that reach this branch — Swin-T stages 2 - 3, N = 384 / 768 at 50 k / 12 k rows — also
            // run faster on it than on the four-wave 32 x 32-shape tile: Swin-T at batch 256 10.35 -> 10.17 ms)
            if (epilogue == 2 || epilogue == 3) {  // (the activation-output epilogues: any tile height)
                // 160-row tiles when they fill the two-per-CU slots better: rounds of 512 workgroups, last one counted by its fill
                // (at 12 608 rows, ViT-S/16 B = 64, mlp.fc1 is 79 x 12 = 948 of these = 1.85 rounds instead of 1 188 = 2.32)
                const long t160 = (long)((M + 159) / 160) * (N / 128);
                if (N >= 1024 && K == 384 && gemm_round_fill(t160, 512) > 1.1 * gemm_round_fill(t128, 512))
                    return dma(T160x128q16, 2);
            }
            return dma(T128x128q16, 2);
        }
        // Swin-T's narrow stages (N = 96, 192, 288, 576 at 2e5 .. 8e5 rows): tiles that divide N exactly on the LDS-DMA
        // loop instead of 64 x 64 register-staged tiles with a ragged last column (these GEMMs are bound by the 4-byte
        // activations they stream, not by the matrix pipe)
        if (N % 128 != 0 && M >= 4096) {
            if (N % 192 == 0) return dma(T128x192, 3);
            if (N % 96 == 0 && !stats_epilogue) return dma(T128x96, 2);  // 96 is no multiple of BN_MULT
        }
    }
    if (prec == 0 && big_tiles_pay(M, N, K)) return gemm_plan_reg<KsLinearReg>(T256x256, steps);  // (bf16 only on this loop)
    return gemm_plan_reg_tail<KsLinearReg>(M, N, steps);
}

// ---- qkv projection (launch_qkv_e): M = B * n_tokens rows, K = D, N = 3 D ----------------------------------------------
inline GemmPlan gemm_plan_qkv(int prec, int M, int D) {
    const int steps = D / gemm_krow(prec);
    if (prec == 0 && D % 256 == 0 && big_tiles_pay(M, 3 * D, D)) return gemm_plan_reg<KsQkvReg>(T256x256, steps);
    const long t128 = (long)((M + 127) / 128) * (3 * D / 128);
    if (prec == 2 && D % 128 == 0 && M > 64) {
        const auto dma = [steps](GemmTile tile, int stages) { return gemm_plan_dma<KsQkvDma>(tile, stages, steps); };
        // few rows (one tile per call): the DMA loop's shorter prologue shows (B = 1 forward 1.03 -> 1.01 ms)
        if (M <= OCM_SMALLM_ROWS) return dma(T64x128w, OCM_SMALLM_STAGES);
        // ViT-B sizes: 256 x 256 tiles halve the bytes through L2 (384^2 B = 128: 755 -> 715 us per launch)
        // (on v_mfma_f32_16x16x32_bf16 since round 4: 717 -> 670 us)
        if (D % 256 == 0 && big_tiles_pay(M, 3 * D, D)) return dma(T256x256m16, 2);
        // the 8-wave 128 x 128 tile on the LDS-DMA loop (ViT-S/16 B = 64: 46.6 -> 41.8 us per launch, +2 % end
        // to end; ViT-B/16 384^2 B = 128: 805 -> 759 us; alternating runs on one box). The 4-wave form of the
        // same tile measures like the register-staged kernel.
        // ... on v_mfma_f32_16x16x32_bf16 (43.1 -> 41.6 us; GemmCfg::MF16)
        if (t128 >= 512) return dma(T128x128q16, 2);
    }
    // register-staged: the 128 x 128 tile runs on 8 waves here (32x64 MFMA sub-tiles per wave): two waves per SIMD inside one
    // workgroup overlap its heavier scatter epilogue with the other waves' MFMAs (29.0 -> 25.8 us at ViT-S, B=64)
    if (D % 128 == 0 && t128 >= 512) return gemm_plan_reg<KsQkvReg>(T128x128q, steps);
    if (D % 128 == 0) return gemm_plan_reg<KsQkvReg>(T64x128, steps);
    return gemm_plan_reg<KsQkvReg>(T64x64, steps);
}

// ---- nn.Linear with explicit row strides (launch_linear_ld_mode; Swin: bf16 / fp32, N not a multiple of the tile) ------
inline GemmPlan gemm_plan_linear_ld(int prec, int M, int N, int K) {
    const int steps = K / gemm_krow(prec);
    if (M >= 2048 && N > 64) return gemm_plan_reg<KsLinearReg>(T128x128, steps);
    if (M > 64 && N > 64) return gemm_plan_reg<KsLinearReg>(T64x128, steps);
    return gemm_plan_reg<KsLinearReg>(T64x64, steps);
}

// ---- conv / up-conv GEMMs (kernels_conv.hip: conv_gemm) ----------------------------------------------------------------
// M = B h w rows; N GEMM columns (O, or 4 O for the up-convolution); K the real contraction length (9 C, 27 or C): the loaders
// pad the last step with zeros. The tile goes by rows and width as in the register-staged tail above; only the 3x3 loader
// (Conv3x3Loader) gets compile-time depths.
inline GemmPlan gemm_plan_conv(int prec, int M, int N, int K, bool loader3x3) {
    const int krow = gemm_krow(prec), steps = (K + krow - 1) / krow;
    return loader3x3 ? gemm_plan_reg_tail<KsConv3x3>(M, N, steps) : gemm_plan_reg_tail<KsNone>(M, N, steps);
}

// ---- fused residual + LayerNorm (launch_resid_ln_d): full rows, D in {128, 256, 384} -----------------------------------
// One 8-wave workgroup per CU (wave tile 32 x D / 4) on the register-staged loop (two-step prefetch of both operands).
inline GemmPlan gemm_plan_resid_ln(int prec, int D, int K) {
    const GemmTile tile = D == 128 ? T64x128w : D == 256 ? T64x256w : T64x384w;
    const int steps = K / gemm_krow(prec);
    return gemm_plan_reg<KsLinearReg>(tile, steps);
}
