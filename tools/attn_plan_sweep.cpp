// attn_plan_sweep.cpp — a host-only sweep of csrc/attn_plan.h, meant to be built with sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I vit-ocm-wmsegmentation_amd/csrc
//         tools/attn_plan_sweep.cpp -o attn_plan_sweep && ./attn_plan_sweep        (one command line)
// Over N = 1 .. 4100, the (image, head) counts of the attention tests, every precision and head width, with no workspace, the
// workspace attn_plan_workspace_bytes names, exactly the plan's need and one float less: at least one key slice, every slice owns
// at least one tile, a planned split needs no more than the reported workspace bytes, and the grid covers every query tile.
// Exit status 0 and the last line "ok" when all of it holds.
#include <cstdio>
#include <cstdlib>

#include "attn_plan.h"

static long g_plans = 0, g_splits = 0;

static void fail(const char *what, int prec, int bh, int n, int hd, size_t ws, const AttnPlan &p) {
    std::fprintf(stderr, "FAILED %s: prec %d bh %d N %d head_dim %d workspace %zu -> kernel %d waves %d stages %d slices %d grid %u x %u x %u need %zu\n",
                 what, prec, bh, n, hd, ws, (int)p.kernel, p.waves, p.stages, p.kslices, p.grid_x, p.grid_y, p.grid_z, p.workspace_need);
    std::exit(1);
}

static AttnPlan check(int prec, int batch, int n, int heads, int hd, size_t ws, size_t reported) {
    const AttnPlan p = attn_plan(prec, batch, n, heads, hd, ws);
    const int bh = batch * heads, qtiles = attn_qtiles(n);
    ++g_plans;
    if (p.kslices < 1 || p.grid_z != (unsigned)p.kslices) fail("nslice >= 1", prec, bh, n, hd, ws, p);
    if (p.kernel == ATTN_X3_DMA_KSPLIT) {
        ++g_splits;
        const int per = (qtiles + p.kslices - 1) / p.kslices;  // what the kernel computes from gridDim.z
        if (p.kslices < 2 || (p.kslices - 1) * per >= qtiles) fail("every slice owns a tile", prec, bh, n, hd, ws, p);
        if (p.workspace_need > reported || p.workspace_need > ws) fail("need <= workspace bytes", prec, bh, n, hd, ws, p);
        if (p.workspace_need != (size_t)p.kslices * bh * n * 68 * 4) fail("need = slices x rows x 68 floats", prec, bh, n, hd, ws, p);
    } else if (p.kslices != 1 || p.workspace_need != 0) {
        fail("no split, no need", prec, bh, n, hd, ws, p);
    }
    const long rows_per_wg = p.kernel == ATTN_BF16_WHOLE ? n : p.kernel == ATTN_X3_WS ? 32 : 32L * p.waves;
    const long wgs_per_head = p.kernel == ATTN_BF16_WHOLE ? 1 : p.grid_x;
    if (wgs_per_head * rows_per_wg < n || (long)(p.kernel == ATTN_BF16_WHOLE ? p.grid_x : p.grid_y) != bh)
        fail("grid covers the queries", prec, bh, n, hd, ws, p);
    if (p.waves * 64 > 1024 || p.lds_bytes < 0 || p.lds_bytes > 160 * 1024) fail("fits a CU", prec, bh, n, hd, ws, p);
    return p;
}

int main() {
    const int counts[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 3}, {1, 6}, {2, 6}, {13, 1}, {8, 2}, {5, 4}, {13, 2}, {32, 2}, {127, 1}, {64, 2}, {131, 1}, {64, 6}};
    for (int prec = 0; prec < 3; ++prec)
        for (int hd = 64; hd <= 128; hd += 64)
            for (const auto &c : counts)
                for (int n = 1; n <= 4100; ++n) {
                    const size_t reported = attn_plan_workspace_bytes(prec, c[0], n, c[1], hd);
                    check(prec, c[0], n, c[1], hd, 0, reported);
                    if (!reported) {
                        check(prec, c[0], n, c[1], hd, (size_t)1 << 40, (size_t)1 << 40);  // nothing asked for: whatever is offered, no split may need it
                        continue;
                    }
                    const AttnPlan p = check(prec, c[0], n, c[1], hd, reported, reported);
                    if (p.kernel != ATTN_X3_DMA_KSPLIT) fail("a reported workspace is used", prec, c[0] * c[1], n, hd, reported, p);
                    check(prec, c[0], n, c[1], hd, p.workspace_need, reported);
                    const AttnPlan s = check(prec, c[0], n, c[1], hd, p.workspace_need - sizeof(float), reported);
                    if (s.kernel != ATTN_X3_DMA) fail("one float short: unsplit", prec, c[0] * c[1], n, hd, p.workspace_need - 4, s);
                }
    std::printf("%ld plans, %ld of them key splits\nok\n", g_plans, g_splits);
    return 0;
}
