"""The tile dispatch of the GEMM-shaped operators (csrc/gemm_plan.h), asked through ocm_gemm_plan: a host function, no GPU.

Every row is (family, precision, epilogue, flags, M, N, K) -> (bm, bn, waves, 16x16 MFMA, LDS-DMA loop, ring stages, compile-time
K steps, split-K slices). The expected values were derived by hand from the branches of launch_linear_epi, launch_qkv_e,
launch_linear_ld_mode, conv_gemm and launch_resid_ln_d as they stood before the decision moved into gemm_plan.h, and confirmed by a
kernel trace (tools/gemm_plan_trace.py); none was produced by running the plan functions. A changed threshold
fails here instead of silently moving a shape of the GPU operator tests (test_ops_x3_gpu.py, test_ops_gpu.py,
test_memcheck_gpu.py, test_conv_shapes_gpu.py) to another kernel.

The register-staged loop double-buffers its operands, so `stages` is 2 on it. ks = 0 is the run-time K loop.
"""
import ctypes as C

import pytest

from tests.conv_helpers import CONV, UPCONV
from vit_ocm_wmsegmentation_amd import _lib

BF16, FP32, X3 = _lib.OCM_PREC_BF16, _lib.OCM_PREC_FP32, _lib.OCM_PREC_BF16X3
LINEAR, QKV, LINEAR_LD, CONVF, RESID_LN = (_lib.OCM_GEMM_LINEAR, _lib.OCM_GEMM_QKV, _lib.OCM_GEMM_LINEAR_LD, _lib.OCM_GEMM_CONV,
                                           _lib.OCM_GEMM_RESID_LN)
STATS, SPLITK, C3X3 = _lib.OCM_PLAN_STATS_EPILOGUE, _lib.OCM_PLAN_SPLITK_OFFERED, _lib.OCM_PLAN_CONV3X3
REG, DMA = 0, 1
ALL, F32_OUT, ACT_OUT = (0, 1, 2, 3), (0, 1), (2, 3)  # epilogue modes (OCM_EPI_*)


def plan(lib, family, precision, epilogue, M, N, K, flags=0):
    out = _lib.OcmGemmPlanInfo()
    rc = lib.ocm_gemm_plan(family, precision, epilogue, M, N, K, flags, C.byref(out))
    assert rc == _lib.OCM_OK, lib.ocm_last_error()
    return tuple(getattr(out, name) for name, _ in _lib.OcmGemmPlanInfo._fields_)


def want(tile, waves, mfma16, loop, stages, ks, splitk=1):
    return tile + (waves, mfma16, loop, stages, ks, splitk)


# split-bf16 nn.Linear, no flags: ((M, N, K), epilogue modes, expected plan)
LINEAR_X3 = [
    ((1000, 384, 384), ALL, want((64, 128), 8, 0, DMA, 4, 12)),
    ((333, 384, 1536), ALL, want((64, 64), 4, 0, DMA, 4, 48)),
    ((70, 96, 192), ALL, want((64, 64), 4, 0, REG, 2, 6)),
    ((64, 192, 64), ALL, want((64, 64), 4, 0, REG, 2, 2)),
    ((12608, 1536, 384), F32_OUT, want((128, 128), 8, 1, DMA, 2, 12)),
    ((12608, 1536, 384), ACT_OUT, want((160, 128), 8, 1, DMA, 2, 12)),
    ((12609, 1536, 384), F32_OUT, want((128, 128), 8, 1, DMA, 2, 12)),
    ((12609, 1536, 384), ACT_OUT, want((160, 128), 8, 1, DMA, 2, 12)),
    ((12800, 1536, 384), F32_OUT, want((128, 128), 8, 1, DMA, 2, 12)),  # 80 full blocks of 160 rows: test_linear_x3's shape
    ((12800, 1536, 384), ACT_OUT, want((160, 128), 8, 1, DMA, 2, 12)),
    ((12608, 384, 384), ALL, want((128, 192), 8, 0, DMA, 3, 12)),
    ((24576, 384, 1536), ALL, want((128, 192), 8, 0, DMA, 3, 48)),
    ((32768, 1024, 768), ALL, want((256, 256), 8, 1, DMA, 2, 24)),
    ((16384, 512, 384), ALL, want((128, 128), 8, 1, DMA, 2, 12)),
    ((20000, 1024, 384), ALL, want((256, 256), 8, 1, DMA, 2, 12)),
    ((6000, 96, 384), ALL, want((128, 96), 4, 0, DMA, 2, 12)),
    ((6000, 288, 96), ALL, want((128, 96), 4, 0, DMA, 2, 0)),
    ((5000, 576, 192), ALL, want((128, 192), 8, 0, DMA, 3, 6)),
    ((5000, 192, 768), ALL, want((128, 192), 8, 0, DMA, 3, 24)),
]


@pytest.mark.parametrize("shape,modes,expected", LINEAR_X3, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and len(v) == 3 else None)
def test_linear_split_bf16(lib, shape, modes, expected):
    for epilogue in modes:
        assert plan(lib, LINEAR, X3, epilogue, *shape) == expected, (shape, epilogue)


def test_linear_split_bf16_flags(lib):
    # 128 x 96 is ruled out by the statistics epilogue's BN_MULT = 64: the row falls through to the register-staged tail
    assert plan(lib, LINEAR, X3, 1, 6000, 288, 96, STATS) == want((64, 64), 4, 0, REG, 2, 3)
    assert plan(lib, LINEAR, X3, 1, 6000, 288, 96) == want((128, 96), 4, 0, DMA, 2, 0)
    # mlp.fc2 of a one-tile-per-call forward: four K slices of twelve steps when a workspace is offered
    assert plan(lib, LINEAR, X3, 1, 197, 384, 1536, SPLITK) == want((64, 64), 4, 0, DMA, 4, 12, splitk=4)
    assert plan(lib, LINEAR, X3, 1, 197, 384, 1536) == want((64, 64), 4, 0, DMA, 4, 48)
    assert plan(lib, LINEAR, X3, 1, 197, 384, 1536, SPLITK | STATS) == want((64, 64), 4, 0, DMA, 4, 12, splitk=4)
    # ... and only then: other epilogues, other depths, more than 512 rows
    assert plan(lib, LINEAR, X3, 0, 197, 384, 1536, SPLITK) == want((64, 64), 4, 0, DMA, 4, 48)
    assert plan(lib, LINEAR, X3, 1, 197, 384, 768, SPLITK) == want((64, 128), 8, 0, DMA, 4, 24)
    assert plan(lib, LINEAR, X3, 1, 512, 384, 1536, SPLITK)[-1] == 4
    assert plan(lib, LINEAR, X3, 1, 513, 384, 1536, SPLITK) == want((64, 64), 4, 0, DMA, 4, 48)


@pytest.mark.parametrize("M,D,expected", [
    (12608, 384, want((128, 128), 8, 1, DMA, 2, 12)),
    (15002, 768, want((256, 256), 8, 1, DMA, 2, 24)),
    (591, 384, want((64, 128), 8, 0, DMA, 4, 12)),
    (250, 192, want((64, 64), 4, 0, REG, 2, 6)),
    (34, 128, want((64, 128), 4, 0, REG, 2, 0)),
])
def test_qkv_split_bf16(lib, M, D, expected):
    assert plan(lib, QKV, X3, 0, M, 3 * D, D) == expected


def test_single_bf16_and_fp32_stay_on_the_register_staged_loop(lib):
    for epilogue in ALL:  # 64 elements per K step
        assert plan(lib, LINEAR, BF16, epilogue, 12608, 1536, 384) == want((128, 128), 4, 0, REG, 2, 6)
        assert plan(lib, LINEAR, BF16, epilogue, 12608, 384, 384) == want((64, 128), 4, 0, REG, 2, 6)
        assert plan(lib, LINEAR, BF16, epilogue, 32768, 1024, 768) == want((256, 256), 8, 0, REG, 2, 12)
        # big tiles are bf16-only on that loop
        assert plan(lib, LINEAR, FP32, epilogue, 32768, 1024, 768) == want((128, 128), 4, 0, REG, 2, 24)
    # (launch_qkv_cfg's depths are 6, 12 and 24: 768 / 64 = 12 is one of them)
    assert plan(lib, QKV, BF16, 0, 15002, 3 * 768, 768) == want((256, 256), 8, 0, REG, 2, 12)
    assert plan(lib, QKV, BF16, 0, 12608, 3 * 384, 384) == want((128, 128), 8, 0, REG, 2, 6)


@pytest.mark.parametrize("precision", [BF16, FP32])
def test_strided_swin_launcher_thresholds(lib, precision):
    """M >= 2048 and N > 64 -> 128 x 128; M > 64 and N > 64 -> 64 x 128; otherwise 64 x 64. One row on each side of each threshold."""
    K = 128
    ks = K // (64 if precision == BF16 else 32)
    for M, N, tile in [(2048, 96, (128, 128)), (2047, 96, (64, 128)), (2048, 64, (64, 64)), (65, 96, (64, 128)), (64, 96, (64, 64)),
                       (65, 64, (64, 64))]:
        assert plan(lib, LINEAR_LD, precision, 0, M, N, K) == want(tile, 4, 0, REG, 2, ks), (M, N)


TILE = {"128x128": (128, 128), "64x128": (64, 128), "64x64": (64, 64)}


@pytest.mark.parametrize("case", sorted(CONV) + sorted(UPCONV))
def test_conv_rows(lib, case):
    """Every row of test_conv_shapes_gpu.py: the tile, the step count per precision and which depths are compile-time ones."""
    up = case in UPCONV
    (B, h, w, Cin, O), tile, steps = (UPCONV if up else CONV)[case]
    M, N, K = B * h * w, 4 * O if up else O, Cin if up else 9 * Cin
    for precision, st in ((FP32, steps[0]), (X3, steps[0]), (BF16, steps[1])):
        ks = st if not up and st in (18, 36, 72) else 0
        assert plan(lib, CONVF, precision, 0, M, N, K, 0 if up else C3X3) == want(TILE[tile], 4, 0, REG, 2, ks), (case, precision)
        # the same shape through another loader never gets a compile-time depth
        assert plan(lib, CONVF, precision, 0, M, N, K)[6] == 0


def test_conv_compile_time_depths_by_precision(lib):
    """C = 64, 128, 256, 512 on the 3x3 loader: 18 / 36 / 72 steps are compiled in, whichever precision reaches them."""
    got = {Cin: tuple(plan(lib, CONVF, p, 0, 81, 128, 9 * Cin, C3X3)[6] for p in (FP32, X3, BF16)) for Cin in (32, 64, 128, 256, 512)}
    assert got == {32: (0, 0, 0), 64: (18, 18, 0), 128: (36, 36, 18), 256: (72, 72, 36), 512: (0, 0, 72)}


@pytest.mark.parametrize("precision", [BF16, FP32, X3])
@pytest.mark.parametrize("D", [128, 256, 384])
def test_resid_ln_runs_full_rows_on_eight_waves(lib, precision, D):
    ks = 384 // (64 if precision == BF16 else 32)
    assert plan(lib, RESID_LN, precision, 0, 12608, D, 384) == want((64, D), 8, 0, REG, 2, ks)


# the tiles the shipped dispatch can name: (bm, bn, waves, 16x16 MFMA)
SHIPPED_TILES = {(64, 64, 4, 0), (64, 128, 4, 0), (64, 128, 8, 0), (64, 256, 8, 0), (64, 384, 8, 0), (128, 96, 4, 0), (128, 128, 4, 0),
                 (128, 128, 8, 0), (128, 128, 8, 1), (128, 192, 8, 0), (160, 128, 8, 1), (256, 256, 8, 0), (256, 256, 8, 1)}


def test_every_plan_fits_the_cu(lib):
    """Over a sweep that reaches every shipped tile: 64 lanes x waves <= 1024 threads, and the LDS the plan implies —
    stages x (bm + bn) x 128 bytes of operands plus the epilogues' row / column tables of (bm + bn) x 8 — within 160 KiB."""
    seen = set()
    rows = (1, 64, 65, 197, 512, 2305, 4096, 4097, 12608, 16384, 32768, 50176, 200000)
    widths = (32, 64, 96, 128, 192, 256, 288, 384, 576, 768, 1024, 1536, 3072)
    depths = (64, 192, 384, 768, 1536, 3072)
    calls = []
    for M in rows:
        for K in depths:
            for N in widths:
                for precision in (BF16, FP32, X3):
                    for epilogue in (0, 1, 2, 3, 4):
                        calls.append((LINEAR, precision, epilogue, M, N, K, 0))
                    calls.append((LINEAR, precision, 1, M, N, K, STATS | SPLITK))
                    calls.append((CONVF, precision, 0, M, N, K, 0))
                for precision in (BF16, FP32):
                    calls.append((LINEAR_LD, precision, 0, M, N, K, 0))
            for precision in (BF16, FP32, X3):
                calls.append((QKV, precision, 0, M, 3 * K, K, 0))
                for D in (128, 256, 384):
                    calls.append((RESID_LN, precision, 0, M, D, K, 0))
    for call in calls:
        bm, bn, waves, mfma16, loop, stages, ks, splitk = plan(lib, *call[:6], flags=call[6])
        seen.add((bm, bn, waves, mfma16))
        assert waves in (4, 8) and mfma16 in (0, 1) and loop in (REG, DMA) and splitk in (1, 4), call
        assert 2 <= stages <= 4 and (loop == DMA or stages == 2), call
        assert stages * (bm + bn) * 128 + (bm + bn) * 8 <= 160 * 1024, call
        assert ks == 0 or ks * (64 if call[1] == BF16 else 32) == call[5] or call[0] == LINEAR and splitk == 4, call
    assert seen == SHIPPED_TILES, seen ^ SHIPPED_TILES


def test_refuses_what_the_operators_refuse(lib):
    out = _lib.OcmGemmPlanInfo()

    def rc(family, precision, epilogue, M, N, K, flags=0):
        return lib.ocm_gemm_plan(family, precision, epilogue, M, N, K, flags, C.byref(out))

    assert rc(LINEAR, 7, 0, 10, 32, 64) == _lib.OCM_EINVAL and b"precision" in lib.ocm_last_error()
    assert rc(LINEAR, BF16, 0, 10, 33, 64) == _lib.OCM_EINVAL  # N % 32
    assert rc(LINEAR, BF16, 0, 10, 32, 96) == _lib.OCM_EINVAL  # K % 64 in bf16
    assert rc(LINEAR, FP32, 0, 10, 32, 96) == _lib.OCM_OK      # ... a multiple of the 32-element row of fp32
    assert rc(LINEAR, X3, 0, 10, 32, 48) == _lib.OCM_EINVAL
    assert rc(LINEAR, X3, 5, 10, 32, 64) == _lib.OCM_EINVAL    # epilogue
    assert rc(LINEAR, X3, 0, 0, 32, 64) == _lib.OCM_EINVAL
    assert rc(QKV, X3, 0, 10, 3 * 96, 96) == _lib.OCM_EINVAL   # D % 64
    assert rc(QKV, X3, 0, 10, 384, 384) == _lib.OCM_EINVAL     # N = 3 D
    assert rc(LINEAR_LD, X3, 0, 10, 32, 64) == _lib.OCM_EINVAL
    assert rc(RESID_LN, X3, 0, 10, 512, 384) == _lib.OCM_EINVAL
    assert rc(RESID_LN, X3, 0, 10, 384, 96) == _lib.OCM_EINVAL  # K % 64 in every precision
    assert rc(CONVF, X3, 0, 10, 32, 9 * 4128, C3X3) == _lib.OCM_EINVAL
    assert rc(9, X3, 0, 10, 32, 64) == _lib.OCM_EINVAL
    assert lib.ocm_gemm_plan(LINEAR, X3, 0, 10, 32, 64, 0, None) == _lib.OCM_EINVAL
