"""The shapes of tests/test_attention_tiles_gpu.py with the kernel each is meant for, shared with tests/test_attn_plan_host.py:
the GPU file asserts every row through ocm_attention_plan before it launches anything, the host file asserts the same rows
without a GPU. A plan is (kernel, waves, ring stages, key slices, grid x, y, z, dynamic LDS bytes); every value was derived by
hand from the branches of launch_attention as they stood before the decision moved into csrc/attn_plan.h:

  split-bf16, 64-wide heads, qtiles = ceil(N / 32), bh = B * H:
    N <= 1024, ceil(qtiles / 4) * bh <  128  wave-split   4 waves, 2 slots, grid (qtiles, bh), 128 KiB of dynamic LDS
    N <= 1024, ceil(qtiles / 4) * bh >= 128  pipelined    4 waves, 3 slots, grid (ceil(qtiles / 4), bh)
    N >  1024                                LDS-DMA      8 waves, 3 stages, grid (ceil(qtiles / 8), bh)
    ... a workspace offered and wgs = ceil(qtiles / 8) * bh <= 128: want = 4 / 3 / 2 slices at wgs <= 64 / 96 / 128,
        per = ceil(qtiles / want), nslice = ceil(qtiles / per), need = nslice * bh * N * 68 * 4 bytes; split when
        nslice > 1 and need <= the offered bytes: grid z = nslice
  split-bf16, 128-wide heads: LDS-DMA, 4 waves, 2 stages, grid (ceil(qtiles / 4), bh) at every N
"""
from vit_ocm_wmsegmentation_amd import _lib

WS, PP, DMA, KSPLIT = _lib.OCM_ATTN_X3_WAVE_SPLIT, _lib.OCM_ATTN_X3_PIPELINED, _lib.OCM_ATTN_X3_DMA, _lib.OCM_ATTN_X3_DMA_KSPLIT
WS_LDS = 128 * 1024
ROW_BYTES = 68 * 4  # one query row of one key slice in the workspace: 64 context floats, maximum, sum, two of padding


def ws_plan(qtiles, bh):
    return (WS, 4, 2, 1, qtiles, bh, 1, WS_LDS)


def pp_plan(gx, bh):
    return (PP, 4, 3, 1, gx, bh, 1, 0)


def dma_plan(gx, bh, waves=8, stages=3):
    return (DMA, waves, stages, 1, gx, bh, 1, 0)


def ksplit_plan(gx, bh, nslice):
    return (KSPLIT, 8, 3, nslice, gx, bh, nslice, 0)


# ---- the software-pipelined kernel: (B, N, H) -> plan. B * H = 128 (64 x 2) puts one workgroup per (image, head) on it up to 128 tokens
PP_ONE_WG = [(64, N, 2) for N in (1, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128)]  # nt = 1..4, first_pad 1, 31 and 32
PP_CASES = {shape: pp_plan(1, 128) for shape in PP_ONE_WG}
PP_CASES.update({
    (32, 129, 2): pp_plan(2, 64),   # two workgroups per head, the second with one row in wave 0 and waves 1-3 inactive
    (32, 160, 2): pp_plan(2, 64),   # ... with a full wave 0
    (8, 1024, 2): pp_plan(8, 16),   # nt = 32, first_pad 32
    (8, 1023, 2): pp_plan(8, 16),   # first_pad 31
    (8, 993, 2): pp_plan(8, 16),    # first_pad 1
    (131, 97, 1): pp_plan(1, 131),  # a workgroup count that is no multiple of the eight XCDs
})
PP_SAME_INPUT = [(64, 96, 2), (64, 97, 2)]  # every (b, h) on the same q, k, v: bit-identical outputs
# deferred-maximum spikes: (B, N, H, spike key)
PP_SPIKES = [(64, 97, 2, 0), (64, 97, 2, 64), (64, 97, 2, 96), (8, 1024, 2, 1000)]

# ---- the key-split operator: (B, N, H) -> (plan with the workspace ocm_attention_workspace_bytes names, slices)
KSPLIT_CASES = {
    (1, 1025, 1): ksplit_plan(5, 1, 4),    # 5 workgroups: four slices of 9, 9, 9 and 6 tiles
    (13, 1025, 1): ksplit_plan(5, 13, 3),  # 65 workgroups: three slices of 11 tiles
    (5, 1025, 4): ksplit_plan(5, 20, 2),   # 100 workgroups: two slices of 17 and 16 tiles
    (13, 1025, 2): dma_plan(5, 26),        # 130 workgroups: no split, no workspace
    (2, 1056, 1): ksplit_plan(5, 2, 4),    # no padding key
    (1, 2305, 6): ksplit_plan(10, 6, 4),   # one ViT-S/8 window: 73 tiles in slices of 19, 19, 19 and 16
}
# spikes at (1, 1025, 1): {key: height}; slices own keys 0-287, 288-575, 576-863, 864-1024. Height 2 where there is one spike: with
# a single (image, head) pair the jump rests on one query's norm (|q|^2 = 11 in this draw against the 16 expected: 14.4 log2 units
# at height 1, short of the 16 the input must reach)
KSPLIT_SPIKES = {
    "third_slice": {700: 2.0},
    "lone_last_key": {1024: 2.0},
    "one_per_slice": {100: 0.5, 400: 1.0, 700: 2.0, 1000: 1.5},
    # scores of ~120 (170 log2 units) in the third slice: 2^(m_s - m) overflows fp32 unless m is the maximum over ALL slices
    "tall_third_slice": {700: 10.0},
}

# ---- 128-wide heads at (2, N, 3) and the wave-split kernel at (1, N, 2)
HD128_CASES = {(2, N, 3): dma_plan(gx, 6, waves=4, stages=2) for N, gx in ((1, 1), (33, 1), (64, 1), (96, 1), (97, 1), (1025, 9))}
WS_CASES = {(1, 128, 2): ws_plan(4, 2), (1, 129, 2): ws_plan(5, 2)}  # one tile per wave, then wave 0 with two


def workspace_need(shape, nslice):
    B, N, H = shape
    return nslice * B * H * N * ROW_BYTES
