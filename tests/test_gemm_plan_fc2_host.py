"""The thresholds of the mlp.fc2 rule of csrc/gemm_plan.h (gemm_plan_linear), asked through ocm_gemm_plan: a host function, no GPU.

The rule: split-bf16 operands, the statistics-producing residual epilogue, N = 384, at least 24 K steps (K >= 768), more than 4096
rows (below that the few-row branch answers), t160 = ceil(M / 160) x 3 and t192 = ceil(M / 128) x 2 both <= 256 (one round of
workgroups each) and t160 >= 1.1 x t192 -> 160 x 128 tiles (eight waves, 16 x 16 MFMA) on a three-stage LDS-DMA ring; everything
else answers as before. Every expected row below was worked out by hand from that sentence and from the neighbouring branches; none
was produced by calling the plan. tests/test_gemm_plan_host.py guards the rows of the other branches.
"""
import ctypes as C

import pytest

from vit_ocm_wmsegmentation_amd import _lib

X3, LINEAR = _lib.OCM_PREC_BF16X3, _lib.OCM_GEMM_LINEAR
STATS = _lib.OCM_PLAN_STATS_EPILOGUE
REG, DMA = 0, 1
RESID = 1  # OCM_EPI_BIAS_RESID_F32

# (bm, bn, waves, 16x16 MFMA, loop, stages, compile-time K steps, split-K slices)
TALL = lambda ks: (160, 128, 8, 1, DMA, 3, ks, 1)
T192 = lambda ks: (128, 192, 8, 0, DMA, 3, ks, 1)


def plan(lib, M, N, K, epilogue=RESID, flags=STATS):
    out = _lib.OcmGemmPlanInfo()
    rc = lib.ocm_gemm_plan(LINEAR, X3, epilogue, M, N, K, flags, C.byref(out))
    assert rc == _lib.OCM_OK, lib.ocm_last_error()
    return tuple(getattr(out, name) for name, _ in _lib.OcmGemmPlanInfo._fields_)


@pytest.mark.parametrize("M,t160,t192", [(12608, 237, 198), (12800, 240, 200)])
def test_bench_rows_take_the_tall_tile(lib, M, t160, t192):
    """ViT-S/16 at B = 64 (12 608 rows: 79 x 3 against 99 x 2 workgroups) and 80 full row blocks of 160."""
    assert -(-M // 160) * 3 == t160 and -(-M // 128) * 2 == t192 and t160 <= 256 and 10 * t160 >= 11 * t192
    assert plan(lib, M, 384, 1536) == TALL(48)


def test_single_round_bound(lib):
    """85 row blocks of 160 are 255 workgroups, 86 are 258: 13 601 is the first row count at which either tiling leaves one round
    (128 x 192 is then 107 x 2 = 214)."""
    assert plan(lib, 13600, 384, 1536) == TALL(48)
    assert plan(lib, 13601, 384, 1536) == T192(48)
    assert plan(lib, 16384, 384, 1536) == T192(48)
    assert plan(lib, 24576, 384, 1536) == T192(48)  # (pinned by tests/test_gemm_plan_host.py as well)


def test_lower_row_bound(lib):
    """Up to 4096 rows the few-row branch answers (K >= 1024: 64 x 64 tiles on a four-stage ring); one row more is 26 x 3 = 78
    workgroups against 33 x 2 = 66, one row block of 128 more (4224 rows) 27 x 3 = 81 against 66."""
    assert plan(lib, 4096, 384, 1536) == (64, 64, 4, 0, DMA, 4, 48, 1)
    assert plan(lib, 3968, 384, 1536) == (64, 64, 4, 0, DMA, 4, 48, 1)
    assert plan(lib, 4097, 384, 1536) == TALL(48)
    assert plan(lib, 4224, 384, 1536) == TALL(48)
    assert plan(lib, 6304, 384, 1536) == TALL(48)  # ViT-S/16 at B = 32: 40 x 3 = 120 against 50 x 2 = 100


def test_the_ratio_decides_inside_the_row_range(lib):
    """t160 >= 1.1 x t192 cannot fail between the two row bounds: 30 ceil(M / 160) >= 0.1875 M and 22 ceil(M / 128) < 0.171875 M + 22,
    so the condition holds from 1408 rows on. Worked by hand where the rounding favours 128 x 192 most (M a multiple of 160 just past a
    multiple of 128) and at multiples of both."""
    for M, t160, t192 in [(4160, 78, 66), (4480, 84, 70), (5120, 96, 80), (8960, 168, 140), (12160, 228, 190), (13440, 252, 210)]:
        assert -(-M // 160) * 3 == t160 and -(-M // 128) * 2 == t192 and 10 * t160 >= 11 * t192
        assert plan(lib, M, 384, 1536) == TALL(48)


def test_step_count(lib):
    """K = 384 is twelve steps (attn.proj): stays on 128 x 192. K = 768 is 24 steps: admitted. K = 736 is 23 (run-time loop)."""
    assert plan(lib, 12608, 384, 384) == T192(12)
    assert plan(lib, 12608, 384, 768) == TALL(24)
    assert plan(lib, 12608, 384, 736) == T192(0)
    assert plan(lib, 12608, 384, 3072) == TALL(96)


def test_other_widths(lib):
    """N = 768: 99 x 6 = 594 tiles of 128 x 128 -> the eight-wave 16 x 16-shape tile; N = 192: one column of 128 x 192 tiles."""
    assert plan(lib, 12608, 768, 1536) == (128, 128, 8, 1, DMA, 2, 48, 1)
    assert plan(lib, 12608, 192, 1536) == T192(48)


def test_only_the_statistics_epilogue(lib):
    """The rule covers what was measured: the residual epilogue that also writes the pairs and the row sums. The plain epilogues of
    the same shape keep 128 x 192."""
    for epilogue in (0, 1, 2, 3):
        assert plan(lib, 12608, 384, 1536, epilogue, 0) == T192(48), epilogue
    for precision in (_lib.OCM_PREC_BF16, _lib.OCM_PREC_FP32):
        out = _lib.OcmGemmPlanInfo()
        assert lib.ocm_gemm_plan(LINEAR, precision, RESID, 12608, 384, 1536, STATS, C.byref(out)) == _lib.OCM_OK
        assert (out.bm, out.bn, out.lds_dma) == (64, 128, REG)
