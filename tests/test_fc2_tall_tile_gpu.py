"""mlp.fc2 on 160 x 128 tiles and a three-stage LDS-DMA ring (csrc/gemm_plan.h: the N = 384 rule), through ocm_op_linear_stats: the
residual epilogue that also writes the split pairs of x and the row sums of the next LayerNorm (gemm_kernels.h: EpiResidStats), as
three 64-row passes over a 160-row accumulator image whose last pass is half filled.

Rows: 4 100 = 25 full row blocks and a 100-row tail (the tail block's 32-row half band holds 4 valid rows, `m < M` cuts all three
passes), 4 160 = 26 exact blocks, 4 097 = one valid row in the last block. All are past the 4 096 rows of the few-row branch, so the
rule answers (asserted through ocm_gemm_plan below). K = 1 536 (48 steps) and K = 768 (24 steps, the least the rule admits).

Bounds. x and the pairs: the bound tests/test_ops_x3_gpu.py::test_linear_x3 applies to ocm_op_linear at the same data scales,
eps = 3e-5 * max(1, sqrt(K) / 8), against a float64 product of the split operands' own values. The sums are 128-column sums of
values that each sit within eps of the reference, so sum x is held to 128 eps and sum x^2 to 2 eps sum |x| + 128 eps^2 (first-order
propagation of the same eps; fp32 accumulation of 128 terms adds 128 * 2^-24 relative, two orders below that). shift is fp32
arithmetic on its inputs: 16 * 2^-24 of the magnitudes added.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.engine import from_split, to_operand

pytestmark = pytest.mark.gpu
X3 = _lib.OCM_PREC_BF16X3
N = 384
ROWS, DEPTHS = (4100, 4160, 4097), (1536, 768)
CASES = [(M, K, centred) for M in ROWS for K in DEPTHS for centred in (False, True)]


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


@functools.lru_cache(maxsize=None)
def _problem(M, K):
    """Inputs at test_linear_x3's scales and the float64 x they give, computed once per shape and never modified."""
    dev = torch.device("cuda:0")
    a, w = _rand((M, K), dev, 40), _rand((N, K), dev, 41, 0.05)
    bias, resid = _rand((N,), dev, 42, 0.1), _rand((M, N), dev, 43)
    a_s, w_s = to_operand(a, X3), to_operand(w, X3)
    x_ref = from_split(a_s).double() @ from_split(w_s).double().t() + bias.double() + resid.double()
    # a previous LayerNorm site: sums in six slots per row (three tiles' first slots carry them) and a shift per row
    prev_stats = _rand((M, N // 64, 2), dev, 44, 20.0)
    prev_shift = _rand((M,), dev, 45, 0.5)
    shift_ref = prev_shift.double() + prev_stats[:, :, 0].double().sum(1) / N
    shift_mag = prev_shift.abs().double() + prev_stats[:, :, 0].abs().double().sum(1) / N
    return dict(a_s=a_s, w_s=w_s, bias=bias, resid=resid, x_ref=x_ref, prev_stats=prev_stats, prev_shift=prev_shift,
                shift_ref=shift_ref, shift_mag=shift_mag)


def _run(lib, M, K, centred, pattern="nan"):
    """One launch into guard-banded buffers of exactly M rows, the outputs poisoned with `pattern`: (x, pairs, stats, shift), guards."""
    p = _problem(M, K)
    dev = p["resid"].device
    g = {"x": Guarded(M * N * 4, dev, pattern), "xs": Guarded(M * N * 4, dev, pattern),
         "stats": Guarded(M * (N // 64) * 8, dev, pattern), "shift": Guarded(M * 4, dev, pattern)}
    g["x"].payload(torch.float32, (M, N)).copy_(p["resid"])  # x is updated in place
    rc = lib.ocm_op_linear_stats(X3, p["a_s"].data_ptr(), p["w_s"].data_ptr(), p["bias"].data_ptr(), g["x"].ptr, g["xs"].ptr,
                                 g["stats"].ptr, g["shift"].ptr if centred else None,
                                 p["prev_stats"].data_ptr() if centred else None, p["prev_shift"].data_ptr() if centred else None,
                                 M, N, K, _s())
    assert rc == 0, lib.ocm_last_error().decode()
    torch.cuda.synchronize()
    out = (g["x"].payload(torch.float32, (M, N)), g["xs"].payload(torch.int32, (M, N)),
           g["stats"].payload(torch.float32, (M, N // 64, 2)), g["shift"].payload(torch.float32, (M,)))
    return out, g


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("K", DEPTHS)
def test_the_shapes_reach_the_tall_tile(lib, M, K):
    out = _lib.OcmGemmPlanInfo()
    assert lib.ocm_gemm_plan(_lib.OCM_GEMM_LINEAR, X3, 1, M, N, K, _lib.OCM_PLAN_STATS_EPILOGUE, C.byref(out)) == _lib.OCM_OK
    assert (out.bm, out.bn, out.waves, out.lds_dma, out.stages, out.ksteps) == (160, 128, 8, 1, 3, K // 32)


@pytest.mark.parametrize("M,K,centred", CASES)
def test_values_and_slots(lib, dev, M, K, centred):
    p = _problem(M, K)
    (x, xs, stats, shift), _ = _run(lib, M, K, centred)
    eps = 3e-5 * max(1.0, math.sqrt(K) / 8)
    x_ref = p["x_ref"]
    e_x = (x.double() - x_ref).abs().max().item()
    if centred:
        e_sh = ((shift.double() - p["shift_ref"]).abs() - 16 * 2.0 ** -24 * p["shift_mag"]).max().item()
        sh = p["shift_ref"][:, None]
    else:
        e_sh, sh = 0.0, torch.zeros((M, 1), dtype=torch.float64, device=dev)
    c_ref = x_ref - sh  # what the pairs and the sums are taken of
    e_xs = (from_split(xs.contiguous()).double() - c_ref).abs().max().item()
    tiles = c_ref.view(M, N // 128, 128)
    s1_ref, s2_ref, abs_ref = tiles.sum(2), (tiles * tiles).sum(2), tiles.abs().sum(2)
    carry = stats[:, 0::2].double()  # the first slot of each 128-column tile
    e_s1 = ((carry[:, :, 0] - s1_ref).abs() - 128 * eps).max().item()
    e_s2 = ((carry[:, :, 1] - s2_ref).abs() - (2 * eps * abs_ref + 128 * eps * eps)).max().item()
    print(f"M={M} K={K} centred={centred}: x {e_x:.3e} pairs {e_xs:.3e} (bound {eps:.3e}); beyond their bounds: sum {e_s1:.3e} "
          f"sum2 {e_s2:.3e} shift {e_sh:.3e}")
    assert e_x < eps and e_xs < eps
    assert e_s1 <= 0 and e_s2 <= 0 and e_sh <= 0
    # each row's first slot of a tile carries its sums, the tile's other slot is zero (launch.h: LnFold)
    assert torch.count_nonzero(stats[:, 1::2]).item() == 0
    assert bool(torch.isfinite(stats).all()) and bool((stats[:, 0::2, 1] > 0).all())
    if not centred:  # the shift output is not touched when no shift is asked for
        assert bool(torch.isnan(shift).all())


@pytest.mark.parametrize("M,K,centred", CASES)
def test_two_launches_give_the_same_bits(lib, dev, M, K, centred):
    first, _ = _run(lib, M, K, centred)
    second, _ = _run(lib, M, K, centred)
    for name, u, v in zip(("x", "pairs", "stats", "shift"), first, second):
        if name == "shift" and not centred:
            continue
        assert_same_bits(u, v, f"{name} M={M} K={K}", ("row",))


@pytest.mark.parametrize("M,K,centred", CASES)
def test_guards_and_poison(lib, dev, M, K, centred):
    """Buffers of exactly M rows between guard bands: the 160-row epilogue writes nothing beyond row M - 1, every output byte of the
    rows below M is written (no poison left), and what the poison is does not change a bit of the results."""
    outs = {}
    for pattern in ("nan", "unit"):
        out, g = _run(lib, M, K, centred, pattern)
        for name, buf in g.items():
            assert buf.check() is None, f"{name} (M={M} K={K} centred={centred}, poison {pattern}): {buf.check()}"
        outs[pattern] = out
    x, xs, stats, shift = outs["nan"]
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(stats).all())
    assert bool(torch.isfinite(from_split(xs.contiguous())).all())
    names = ("x", "pairs", "stats") + (("shift",) if centred else ())
    for name, u, v in zip(names, outs["nan"], outs["unit"]):
        assert_same_bits(u, v, f"{name} under two poisons, M={M} K={K}", ("row",))
    if centred:
        assert bool(torch.isfinite(shift).all())
    else:  # untouched: still the poison, bit for bit
        assert torch.equal(outs["unit"][3].view(torch.int32), torch.full((M,), 0x3F803F80, dtype=torch.int32, device=dev))
