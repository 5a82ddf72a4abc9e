"""The kernel dispatch of the flash-attention operators (csrc/attn_plan.h), asked through ocm_attention_plan: a host function, no GPU.

Every row is (precision, B, N, H, head_dim, offered workspace bytes) -> (kernel, waves, ring stages, key slices, grid x, y, z,
dynamic LDS bytes). The expected values were derived by hand from the branches of launch_attention and launch_attention_bf16 as
they stood before the decision moved into attn_plan.h (the rules are written out in tests/attn_tile_cases.py and in the comments
below); none was produced by running the plan function. A changed threshold fails here instead of silently moving a shape of the
GPU operator tests (test_ops_x3_gpu.py, test_ops_gpu.py, test_attention_tiles_gpu.py) to another kernel.

qtiles = ceil(N / 32), bh = B * H throughout.
"""
import ctypes as C

import pytest

from tests import attn_tile_cases as T
from tests.attn_tile_cases import WS, PP, DMA, KSPLIT, ROW_BYTES, dma_plan, ksplit_plan, pp_plan, ws_plan
from vit_ocm_wmsegmentation_amd import _lib

BF16, FP32, X3 = _lib.OCM_PREC_BF16, _lib.OCM_PREC_FP32, _lib.OCM_PREC_BF16X3
WHOLE, STREAM, F32 = _lib.OCM_ATTN_BF16_WHOLE, _lib.OCM_ATTN_BF16_STREAM, _lib.OCM_ATTN_FP32_STREAM
FIELDS = [name for name, _ in _lib.OcmAttentionPlanInfo._fields_]


def plan_info(lib, precision, B, N, H, head_dim=64, workspace=0):
    out = _lib.OcmAttentionPlanInfo()
    rc = lib.ocm_attention_plan(precision, B, N, H, head_dim, workspace, C.byref(out))
    assert rc == _lib.OCM_OK, lib.ocm_last_error()
    return out


def plan(lib, precision, B, N, H, head_dim=64, workspace=0):
    out = plan_info(lib, precision, B, N, H, head_dim, workspace)
    return tuple(getattr(out, name) for name in FIELDS[:8])


def offered(lib, B, N, H, head_dim=64):
    return lib.ocm_attention_workspace_bytes(X3, B, N, H, head_dim)


def whole_plan(bh):  # single bf16, N <= 256: one 8-wave workgroup per (image, head), the sequence resident in LDS
    return (WHOLE, 8, 1, 1, bh, 1, 1, 0)


def stream_plan(gx, bh):  # single bf16: four waves, K | V^T double-buffered
    return (STREAM, 4, 2, 1, gx, bh, 1, 0)


def f32_plan(gx, bh, head_dim=64):  # fp32: four waves, K[2] | Vt[2] of 64 keys = 1 KiB of dynamic LDS per head channel
    return (F32, 4, 2, 1, gx, bh, 1, 1024 * head_dim)


# test_ops_x3_gpu.py::test_attention_x3 and ::test_attention_x3_deferred_max_is_exact_when_the_maximum_jumps (no workspace)
OPS_X3 = {
    (2, 197, 6): ws_plan(7, 12),     # 2 x 12 = 24 four-wave workgroups < 128
    (1, 17, 2): ws_plan(1, 2),
    (1, 577, 3): ws_plan(19, 3),     # 5 x 3
    (1, 64, 1): ws_plan(2, 1),
    (1, 65, 1): ws_plan(3, 1),
    (1, 2305, 2): dma_plan(10, 2),   # 73 query tiles on eight waves
    (1, 5, 1): ws_plan(1, 1),
    (1, 32, 2): ws_plan(1, 2),
    (1, 33, 1): ws_plan(2, 1),
    (1, 1024, 1): ws_plan(32, 1),    # 8 x 1
    (1, 1025, 1): dma_plan(5, 1),
    (64, 197, 6): pp_plan(2, 384),   # 768 workgroups: the only pipelined shape of that file
    (3, 2305, 6): dma_plan(10, 18),
    (2, 197, 3): ws_plan(7, 6),      # the deferred-maximum shapes
    (2, 577, 2): ws_plan(19, 4),
    (1, 197, 1): ws_plan(7, 1),
}
# test_ops_x3_gpu.py::test_attention_x3_128_wide_heads
OPS_X3_HD128 = {(2, 65, 3): (1, 6), (1, 197, 3): (2, 3), (3, 300, 2): (3, 6), (1, 32, 1): (1, 1)}
# test_ops_gpu.py::test_attention (single bf16) and ::test_attention_fp32
OPS_BF16 = {
    (2, 197, 6): whole_plan(12), (1, 17, 2): whole_plan(2), (1, 577, 3): stream_plan(5, 3), (1, 64, 1): whole_plan(1),
    (1, 65, 1): whole_plan(1), (1, 2305, 2): stream_plan(19, 2), (64, 197, 6): whole_plan(384), (1, 256, 1): whole_plan(1),
    (1, 257, 1): stream_plan(3, 1), (1, 5, 1): whole_plan(1), (1, 33, 1): whole_plan(1),
}
OPS_FP32 = {
    (2, 197, 6): f32_plan(2, 12), (1, 17, 2): f32_plan(1, 2), (1, 577, 3): f32_plan(5, 3), (1, 65, 1): f32_plan(1, 1),
    (64, 197, 6): f32_plan(2, 384), (1, 2305, 2): f32_plan(19, 2), (2, 2305, 6): f32_plan(19, 12), (1, 5, 1): f32_plan(1, 1),
    (1, 33, 1): f32_plan(1, 1), (1, 1025, 1): f32_plan(9, 1),
}


@pytest.mark.parametrize("shape", sorted(OPS_X3))
def test_split_bf16_operator_shapes(lib, shape):
    assert plan(lib, X3, *shape) == OPS_X3[shape]


def test_split_bf16_128_wide_operator_shapes(lib):
    for shape, (gx, bh) in OPS_X3_HD128.items():
        assert plan(lib, X3, *shape, head_dim=128) == dma_plan(gx, bh, waves=4, stages=2), shape
        # test_attention_128_wide_heads_fp32_and_bf16 runs (2, 300, 2) where the split-bf16 test runs (3, 300, 2)
        B, N, H = (2, 300, 2) if shape == (3, 300, 2) else shape
        assert plan(lib, BF16, B, N, H, head_dim=128) == stream_plan(gx, B * H), shape  # streaming at every N, 256 and below too
        assert plan(lib, FP32, B, N, H, head_dim=128) == f32_plan(gx, B * H, 128), shape


@pytest.mark.parametrize("shape", sorted(OPS_BF16))
def test_single_bf16_operator_shapes(lib, shape):
    assert plan(lib, BF16, *shape) == OPS_BF16[shape]


@pytest.mark.parametrize("shape", sorted(OPS_FP32))
def test_fp32_operator_shapes(lib, shape):
    assert plan(lib, FP32, *shape) == OPS_FP32[shape]


def test_tile_test_shapes_without_a_workspace(lib):
    """Every shape of test_attention_tiles_gpu.py that runs through ocm_op_attention / ocm_op_attention_hd."""
    for shape, want in {**T.PP_CASES, **T.WS_CASES}.items():
        assert plan(lib, X3, *shape) == want, shape
    for shape in T.PP_SAME_INPUT + [s[:3] for s in T.PP_SPIKES]:
        assert plan(lib, X3, *shape)[0] == PP, shape
    for shape, want in T.HD128_CASES.items():
        assert plan(lib, X3, *shape, head_dim=128) == want, shape
        assert offered(lib, *shape, head_dim=128) == 0  # 128-wide heads never split
    for (B, N, H), want in T.KSPLIT_CASES.items():  # the same shapes through ocm_op_attention: the unsplit eight-wave kernel
        assert plan(lib, X3, B, N, H) == dma_plan(want[4], B * H), (B, N, H)


@pytest.mark.parametrize("shape", sorted(T.KSPLIT_CASES))
def test_tile_test_shapes_with_their_workspace(lib, shape):
    B, N, H = shape
    want = T.KSPLIT_CASES[shape]
    ws = offered(lib, B, N, H)
    info = plan_info(lib, X3, B, N, H, 64, ws)
    assert tuple(getattr(info, n) for n in FIELDS[:8]) == want
    if want[0] == KSPLIT:
        nslice = want[3]
        assert info.workspace_need == nslice * B * H * N * ROW_BYTES == T.workspace_need(shape, nslice)
        assert ws >= info.workspace_need and ws == 4 * B * H * N * ROW_BYTES  # room for the deepest split
        # exactly what the plan needs is enough; one float less and the call runs unsplit, needing nothing
        assert plan(lib, X3, B, N, H, 64, info.workspace_need) == want
        short = plan_info(lib, X3, B, N, H, 64, info.workspace_need - 4)
        assert (short.kernel, short.kslices, short.grid_z, short.workspace_need) == (DMA, 1, 1, 0)
        assert plan(lib, X3, B, N, H, 64, info.workspace_need - 4) == dma_plan(want[4], B * H)
    else:
        assert ws == 0 and info.workspace_need == 0
        assert plan(lib, X3, B, N, H, 64, 1 << 30) == want  # 130 workgroups: no split however much is offered


def test_thresholds_of_the_split_bf16_dispatch(lib):
    # 127 / 128 four-wave workgroups (N = 97: one workgroup of the pipelined kernel per head, four of the wave-split one)
    assert plan(lib, X3, 127, 97, 1) == ws_plan(4, 127)
    assert plan(lib, X3, 128, 97, 1) == pp_plan(1, 128)
    assert plan(lib, X3, 21, 197, 3) == ws_plan(7, 63)   # 2 x 63 = 126
    assert plan(lib, X3, 64, 197, 1) == pp_plan(2, 64)   # 2 x 64 = 128
    # N = 1024 / 1025: four waves up to 1024 tokens on either side of the 128-workgroup rule, eight above
    assert plan(lib, X3, 1, 1024, 1) == ws_plan(32, 1)
    assert plan(lib, X3, 4, 1024, 4) == pp_plan(8, 16)
    assert plan(lib, X3, 1, 1025, 1) == dma_plan(5, 1)
    assert plan(lib, X3, 4, 1025, 4) == dma_plan(5, 16)
    big = 1 << 40
    assert plan(lib, X3, 4, 1024, 4, 64, big) == pp_plan(8, 16)  # a workspace changes nothing at 1024 tokens
    # head_dim 64 / 128
    assert plan(lib, X3, 1, 197, 3, 64) == ws_plan(7, 3)
    assert plan(lib, X3, 1, 197, 3, 128) == dma_plan(2, 3, waves=4, stages=2)
    assert plan(lib, X3, 64, 197, 6, 128) == dma_plan(2, 384, waves=4, stages=2)
    assert plan(lib, X3, 1, 2305, 2, 128, big) == dma_plan(19, 2, waves=4, stages=2)
    assert plan(lib, BF16, 1, 197, 3, 64) == whole_plan(3)
    assert plan(lib, BF16, 1, 197, 3, 128) == stream_plan(2, 3)
    assert plan(lib, FP32, 1, 197, 3, 64) == f32_plan(2, 3, 64)
    assert plan(lib, FP32, 1, 197, 3, 128) == f32_plan(2, 3, 128)
    # single bf16, N = 256 / 257
    assert plan(lib, BF16, 3, 256, 2) == whole_plan(6)
    assert plan(lib, BF16, 3, 257, 2) == stream_plan(3, 6)
    # neither of the other precisions takes a workspace
    assert plan(lib, BF16, 1, 2305, 2, 64, big) == stream_plan(19, 2)
    assert plan(lib, FP32, 1, 2305, 2, 64, big) == f32_plan(19, 2)


# Key split with a workspace: (B, N, H) -> (eight-wave workgroups, slices). N = 2048 is 64 query tiles = 8 workgroups per head,
# N = 1025 is 33 = 5, N = 24 832 is 776 = 97, N = 11 008 is 344 = 43.
KSPLIT_THRESHOLDS = {
    (8, 2048, 1): (64, 4),    # per = 16
    (13, 1025, 1): (65, 3),   # per = 11
    (4, 2048, 3): (96, 3),    # per = 22: slices of 22, 22 and 20 tiles
    (1, 24832, 1): (97, 2),   # per = 388
    (2, 2048, 8): (128, 2),   # per = 32
    (3, 11008, 1): (129, 1),
}


@pytest.mark.parametrize("shape", sorted(KSPLIT_THRESHOLDS))
def test_key_split_thresholds(lib, shape):
    B, N, H = shape
    wgs, nslice = KSPLIT_THRESHOLDS[shape]
    gx = wgs // (B * H)
    ws = offered(lib, B, N, H)
    if nslice == 1:
        assert ws == 0
        assert plan(lib, X3, B, N, H, 64, 1 << 40) == dma_plan(gx, B * H)
        return
    assert ws == 4 * B * H * N * ROW_BYTES
    info = plan_info(lib, X3, B, N, H, 64, ws)
    assert tuple(getattr(info, n) for n in FIELDS[:8]) == ksplit_plan(gx, B * H, nslice)
    assert ws >= info.workspace_need == nslice * B * H * N * ROW_BYTES
    assert plan(lib, X3, B, N, H, 64, info.workspace_need - 4) == dma_plan(gx, B * H)
    assert plan(lib, X3, B, N, H, 64, 0) == dma_plan(gx, B * H)


def test_every_plan_covers_its_queries_and_fits_the_cu(lib):
    """Over a sweep of lengths and (image, head) counts: the grid covers every query row, slices own at least one tile each,
    a planned split fits the workspace the library asks for, and the launch fits a CU (1024 threads, 160 KiB of LDS)."""
    lengths = list(range(1, 131)) + [197, 255, 256, 257, 577, 992, 993, 1023, 1024, 1025, 1056, 1057, 2048, 2305, 4097, 24832]
    seen = set()
    for precision in (BF16, FP32, X3):
        for head_dim in (64, 128):
            for bh in (1, 2, 6, 12, 13, 16, 20, 26, 63, 64, 127, 128, 131, 384):
                for N in lengths:
                    ws = lib.ocm_attention_workspace_bytes(precision, bh, N, 1, head_dim)
                    for offer in {0, ws}:
                        info = plan_info(lib, precision, bh, N, 1, head_dim, offer)
                        p = tuple(getattr(info, n) for n in FIELDS[:8])
                        kernel, waves, stages, kslices, gx, gy, gz, lds = p
                        seen.add(kernel)
                        qtiles = (N + 31) // 32
                        assert waves in (4, 8) and 1 <= stages <= 3 and 0 <= lds <= 160 * 1024, (precision, head_dim, bh, N, p)
                        assert gz == kslices >= 1 and kslices <= 4
                        if kernel == WHOLE:
                            assert (gx, gy) == (bh, 1) and N <= 256
                        elif kernel == WS:
                            assert (gx, gy) == (qtiles, bh)
                        else:
                            assert gy == bh and gx * waves >= qtiles > (gx - 1) * waves
                        if kernel == KSPLIT:
                            per = -(-qtiles // kslices)
                            assert kslices > 1 and (kslices - 1) * per < qtiles  # the last slice owns a tile
                            assert offer == ws >= info.workspace_need == kslices * bh * N * ROW_BYTES
                        else:
                            assert info.workspace_need == 0
                        assert (kernel == KSPLIT) == (offer > 0 and ws > 0)  # whenever the library asks for a workspace, it splits
    assert seen == {WHOLE, STREAM, F32, WS, PP, DMA, KSPLIT}


def test_refuses_what_the_operators_refuse(lib):
    out = _lib.OcmAttentionPlanInfo()

    def rc(precision, B, N, H, head_dim=64, workspace=0):
        return lib.ocm_attention_plan(precision, B, N, H, head_dim, workspace, C.byref(out))

    assert rc(X3, 1, 197, 3) == _lib.OCM_OK
    assert rc(7, 1, 197, 3) == _lib.OCM_EINVAL and b"precision" in lib.ocm_last_error()
    assert rc(X3, 0, 197, 3) == _lib.OCM_EINVAL
    assert rc(X3, 1, 0, 3) == _lib.OCM_EINVAL
    assert rc(X3, 1, 197, 0) == _lib.OCM_EINVAL
    assert rc(X3, 1, 197, 3, 96) == _lib.OCM_EINVAL and b"head_dim" in lib.ocm_last_error()
    assert rc(BF16, 1, 197, 3, 32) == _lib.OCM_EINVAL
    assert lib.ocm_attention_plan(X3, 1, 197, 3, 64, 0, None) == _lib.OCM_EINVAL
    # ... and the workspace query answers 0 for them
    assert lib.ocm_attention_workspace_bytes(7, 1, 2305, 6, 64) == 0
    assert lib.ocm_attention_workspace_bytes(X3, 0, 2305, 6, 64) == 0
    assert lib.ocm_attention_workspace_bytes(X3, 1, 2305, 6, 96) == 0
    assert lib.ocm_attention_workspace_bytes(X3, 1, 2305, 6, 64) == 4 * 6 * 2305 * ROW_BYTES
    P = 0x10000  # a non-null, 16-byte aligned address: the argument checks never follow it
    for bad in [dict(precision=7), dict(q=None), dict(ctx=None, lse=None), dict(B=0), dict(N=0), dict(H=0), dict(head_dim=96),
                dict(workspace=P + 4)]:
        a = dict(precision=X3, q=P, k=P, vt=P, ctx=P, lse=P, B=1, N=1025, H=1, head_dim=64, workspace=P)
        a.update(bad)
        assert lib.ocm_op_attention_ws(a["precision"], a["q"], a["k"], a["vt"], a["ctx"], a["lse"], a["B"], a["N"], a["H"],
                                       a["head_dim"], 0.125, a["workspace"], 1 << 20, None) == _lib.OCM_EINVAL, bad
