"""The U-Net operators of kernels_conv.hip at the tiles and K depths build_unet dispatches (384^2, batch 8) and at degenerate grids,
through the C ABI, against torch on the CPU in float64. The method is test_conv_ops_gpu.py's (helpers in conv_helpers.py): every
activation argument is a column slice of a wider buffer, inputs among NaN columns, outputs among FILL columns that must survive;
every output element is compared; two runs give equal bits. Bounds: TOL, relative to max |reference|. Every figure is printed
(GPUTEST ...) before it is asserted.

Branches. KROW = 32 (fp32, split-bf16 "x3") or 64 (bf16); steps = ceil(K / KROW).
  conv_gemm (ocm_op_conv3x3: N = O, K = 9 C; ocm_op_upconv2x2: N = 4 O, K = C), t128 = ceil(M / 128) * (N / 128):
    N % 128 == 0 and t128 >= 512 -> 128 x 128;  N % 128 == 0 and M > 64 -> 64 x 128;  else 64 x 64
  conv_gemm_cfg: Conv3x3Loader with 18, 36 or 72 steps -> compile-time K, the two-step prefetch ("ct"); every other depth and
    every other loader -> the runtime-K one-step pipeline ("rt").
test_dispatch_table asserts the tile and step columns below against the library's own decision (ocm_gemm_plan, which answers from
the plan function conv_gemm launches by: csrc/gemm_plan.h gemm_plan_conv): a changed threshold fails there instead of moving a
case to another kernel. tests/test_gemm_plan_host.py asserts the same rows without a GPU.

ocm_op_conv3x3 (B, h, w, C, O), ReLU off and on               M      tile      t128  steps fp32, x3 / bf16   layers at 384^2, batch 8
  t128_c64    (3, 105, 104, 64, 256)                          32 760  128 x 128  512  18 ct / 9 rt           e2.conv1 (tiles span images)
  t128_c128   (1, 181, 181, 128, 256)                         32 761  128 x 128  512  36 ct / 18 ct          e2.conv2, e3.conv1, d3.conv2
  t128_c256   (1, 181, 181, 256, 256)                         32 761  128 x 128  512  72 ct / 36 ct          e3.conv2, e4.conv1, d2.conv2, d3.conv1
  t128_c512   (1, 181, 181, 512, 256)                         32 761  128 x 128  512  144 rt / 72 ct         e4.conv2, d2.conv1
  t64x128_c64   (1, 9, 9, 64, 128)                            81      64 x 128   1    18 ct / 9 rt
  t64x128_c128  (2, 9, 7, 128, 128)                           126     64 x 128   1    36 ct / 18 ct
  t64x128_c256  (1, 9, 9, 256, 256)  two N tiles              81      64 x 128   2    72 ct / 36 ct
  t64_c128    (2, 5, 7, 128, 64)                              70      64 x 64         36 ct / 18 ct
  t64_c256    (1, 5, 7, 256, 32)                              35      64 x 64         72 ct / 36 ct
  t64_c512    (1, 5, 7, 512, 64)   bf16 only                  35      64 x 64         - / 72 ct
  grid_1x1    (3, 1, 1, 32, 32)    only the centre tap exists        3       64 x 64         9 rt / 5 rt (W_TAIL)
  grid_1x9    (1, 1, 9, 64, 64)    top and bottom row cleared at once 9      64 x 64         18 ct / 9 rt
  grid_6x1    (2, 6, 1, 32, 64)    left and right column cleared at once 12  64 x 64         9 rt / 5 rt (W_TAIL)
  c4096       (1, 3, 3, 4096, 32)  the largest C: tap = (int)((k + 0.5f) * inv_c) has the least margin       1152 rt / 576 rt
  c4064       (1, 3, 3, 4064, 32)  a large C that is no power of two                                          1143 rt / 572 rt (W_TAIL)
ocm_op_upconv2x2 (B, h, w, C, O), into the left half of a 2 O-wide buffer          M       N     tile       steps fp32, x3 / bf16 (all rt)
  up_c96      (2, 3, 5, 96, 32)    bf16: C ends inside the second K step           30      128   64 x 64    3 / 2 (W_TAIL and k < C)
  up_1x1      (1, 1, 1, 32, 32)                                                    1       128   64 x 64    1 / 1
  up_d1       (1, 2, 2, 1024, 512) the network's d1 at 32x32 images                4       2048  64 x 64    32 / 16
  up_m70      (2, 7, 5, 64, 32)    two row tiles, an image boundary inside the first, one 128-wide tile over all four (i, j) groups
                                                                                   70      128   64 x 128   2 / 1
  up_n256     (1, 9, 9, 128, 64)   two N tiles of two groups each                  81      256   64 x 128   4 / 2
  up_t128     (3, 74, 74, 32, 128) 129 x 4 = 516 tiles                             16 428  512   128 x 128  1 / 1
ocm_op_linear_relu (M, N, K) = EpiLinear<4> with ldo = 2 N, through launch_linear_epi (gemm_kernels.h):
  split-bf16  (8, 1024, 9216), (37, 512, 2304)  M <= 4096, K >= 1024, N % 64 == 0: the four-stage LDS-DMA ring on 64 x 64 (b, d1 at 32x32)
  split-bf16  (16 300, 512, 288)   128 x 4 = 512 tiles: Cfg128x128q16 on the LDS-DMA loop, 9 steps, partial last row tile (e4, d1 at 384^2)
  split-bf16  (4100, 128, 1152)    M > 4096, 33 tiles: no LDS-DMA branch takes it; register-staged 64 x 128, 36 steps rt (b at 384^2:
                                   M = 4608, N = 1024, 288 tiles, lands on the same branch)
  fp32, bf16  (8, 1024, 9216)      M <= 64: register-staged 64 x 64, 288 / 144 steps rt (b at 32x32)
  fp32, bf16  (4100, 128, 1152)    register-staged 64 x 128, 36 / 18 steps rt (launch_gemm's compile-time depths are 2 .. 96 of the ViTs)
  fp32 (16 300, 512, 320), bf16 (16 300, 512, 384)  512 tiles: register-staged 128 x 128, 10 steps rt / 6 steps ct
  The reference is relu(A W^T + b) in float64 of the values the operands hold: A and W are rounded on the CPU the way to_operand
  rounds them (unet_twin.ROUNDING: not at all, to a hi + lo bf16 pair, to bf16) before the float64 product.
ocm_op_maxpool2x2 (B, h, w, C): (1, 258, 258, 1024) has 4 260 096 lanes, past the 16 384-block grid cap (4 194 304 lanes): the
  grid-stride loop's second trip. (1, 2, 2, 4) is one lane; (2, 4, 6, 36) reads the right half of a 2 C-wide buffer (the skip read).
ocm_op_conv1x1_planes (rows, C): 262 181 rows are past the 16 384-block cap (262 144 rows); C = 4, 32 leave sub-lanes idle, C = 128,
  192 take two and three trips of the channel loop; C = 192 runs with a null bias.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.conv_helpers import CONV, FILL, PRECS, TOL, UPCONV, _check_out, _conv_case, _gen, _rows, _run_conv3x3, _s, _slice_in, _slice_out
from tests.memcheck import assert_same_bits
from tests.unet_twin import ROUNDING
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu

KROW = {"fp32": 32, "bf16x3": 32, "bf16": 64}  # gemm_core.h: Elem<E>::KROW
# the rows whose depth is a compile-time one ("ct" above), as (fp32 and split-bf16, bf16); every other row and the up-convolution: "rt"
CT = {"t128_c64": (True, False), "t128_c128": (True, True), "t128_c256": (True, True), "t128_c512": (False, True),
      "t64x128_c64": (True, False), "t64x128_c128": (True, True), "t64x128_c256": (True, True),
      "t64_c128": (True, True), "t64_c256": (True, True), "t64_c512": (False, True), "grid_1x9": (True, False)}

CONV_BF16_ONLY = ("t64_c512",)
CONV_PARAMS = [(c, p) for c in sorted(CONV) for p in PRECS if p == "bf16" or c not in CONV_BF16_ONLY]
T128_TILES = {"t128_c64": 512, "t128_c128": 512, "t128_c256": 512, "t128_c512": 512, "up_t128": 516}


# (precision, (M, N, K))
LINEAR = [
    ("bf16x3", (8, 1024, 9216)), ("bf16x3", (37, 512, 2304)), ("bf16x3", (16300, 512, 288)), ("bf16x3", (4100, 128, 1152)),
    ("fp32", (8, 1024, 9216)), ("fp32", (4100, 128, 1152)), ("fp32", (16300, 512, 320)),
    ("bf16", (8, 1024, 9216)), ("bf16", (4100, 128, 1152)), ("bf16", (16300, 512, 384)),
]

# (B, h, w, C, columns left of the slice, columns right of it)
POOL = {
    "one_lane": (1, 2, 2, 4, 4, 8),
    "skip_read": (2, 4, 6, 36, 36, 0),         # ld_in = 2 C, the right half
    "past_the_cap": (1, 258, 258, 1024, 4, 4),  # ld_in = C + 8
}
# (batch, hw, C, bias given)
PLANES = {
    "past_the_cap": (1, 262144 + 37, 64, True),
    "c4": (2, 35, 4, True),
    "c32": (3, 11, 32, True),
    "c128": (2, 35, 128, True),
    "c192_no_bias": (1, 17, 192, False),
}


def _plan(lib, precision, Mr, N, K, loader3x3):
    """The library's decision for a conv / up-conv GEMM: ((bm, bn), waves, LDS-DMA loop, compile-time K steps)."""
    out = _lib.OcmGemmPlanInfo()
    rc = lib.ocm_gemm_plan(_lib.OCM_GEMM_CONV, _lib.PRECISIONS[precision], 0, Mr, N, K, _lib.OCM_PLAN_CONV3X3 if loader3x3 else 0,
                           ctypes.byref(out))
    assert rc == 0, lib.ocm_last_error()
    return "%dx%d" % (out.bm, out.bn), out.waves, out.lds_dma, out.ksteps


@pytest.mark.parametrize("case", sorted(CONV) + sorted(UPCONV))
def test_dispatch_table(lib, case):
    up = case in UPCONV
    (B, h, w, C, O), tile, steps = (UPCONV if up else CONV)[case]
    Mr, N, K = B * h * w, 4 * O if up else O, C if up else 9 * C
    t128 = -(-Mr // 128) * (N // 128)
    want_ct = (False, False) if up else CT.get(case, (False, False))
    for precision, st, ct in (("fp32", steps[0], want_ct[0]), ("bf16x3", steps[0], want_ct[0]), ("bf16", steps[1], want_ct[1])):
        assert st == -(-K // KROW[precision]), f"{case} {precision}: the table's step count"
        got_tile, waves, lds_dma, ks = _plan(lib, precision, Mr, N, K, not up)
        assert got_tile == tile, f"{case} {precision}: the library runs {got_tile} tiles ({t128} of 128 x 128), the table says {tile}"
        assert (waves, lds_dma) == (4, 0), f"{case} {precision}: four waves on the register-staged loop"
        assert ks == (st if ct else 0), f"{case} {precision}: {st} steps are {'compile-time' if ct else 'run-time'} in the table, the library says {ks}"
        if tile == "128x128":  # ... from 512 tiles of 128 x 128 on: the same width with 511 or fewer runs 64 x 128
            assert t128 == T128_TILES[case] and t128 >= 512
            fewer = 128 * (-(-512 // (N // 128)) - 1)
            assert _plan(lib, precision, fewer, N, K, not up)[0] == "64x128", f"{case} {precision}: {fewer} rows"
    if case.startswith("t"):  # the compile-time-K cases: which precisions run the two-step prefetch
        assert want_ct == {"c64": (True, False), "c128": (True, True), "c256": (True, True), "c512": (False, True)}[case.split("_")[1]]


@pytest.mark.parametrize("case,precision", CONV_PARAMS)
def test_conv3x3(lib, dev, case, precision):
    _run_conv3x3(lib, dev, CONV[case][0], precision)


def test_conv3x3_refuses_more_than_4096_channels(lib, dev):
    buf = torch.zeros(4096, device=dev)
    p = buf.data_ptr()
    assert lib.ocm_op_conv3x3(2, p, 4128, p, p, p, 32, 1, 3, 3, 4128, 32, 0, _s()) == _lib.OCM_EINVAL
    assert "C=4128" in lib.ocm_last_error().decode()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


@pytest.mark.parametrize("precision", PRECS)
def test_conv3x3_image_on_a_one_row_grid(lib, dev, precision):
    """B=2, the 1x5 window at (3, 2) of channels 1..3 of a (2, 5, 7, 9) image: every tap of the top and the bottom row is padding."""
    B, h, w, O = 2, 1, 5, 32
    g = _gen(78)
    big = torch.randn(2, 5, 7, 9, generator=g)
    wt = torch.randn(O, 3, 3, 3, generator=g) / 27 ** 0.5
    bias = torch.randn(O, generator=g)
    ref = _rows(F.conv2d(big[:, 1:4, 3:3 + h, 2:2 + w].double(), wt.double(), bias.double(), padding=1))
    pc = _lib.PRECISIONS[precision]
    kp = 64 if precision == "bf16" else 32
    w_op = to_operand(F.pad(M._rows3x3(wt), (0, kp - 27)).to(dev).contiguous(), pc)
    b_d, big_d = bias.to(dev), big.to(dev)
    vd = big_d[:, 1:4, 3:3 + h, 2:2 + w]
    for relu in (0, 1):
        first = None
        for _ in range(2):
            outbuf, out_ptr, ld_out, pl = _slice_out(B * h * w, O, dev)
            rc = lib.ocm_op_conv3x3_image(pc, vd.data_ptr(), vd.stride(0), vd.stride(1), vd.stride(2), w_op.data_ptr(), b_d.data_ptr(),
                                          out_ptr, ld_out, B, h, w, O, relu, _s())
            assert rc == 0, lib.ocm_last_error()
            torch.cuda.synchronize()
            got = _check_out(outbuf, pl, O, ref.clamp_min(0) if relu else ref, TOL[precision], f"conv3x3_image 1x5 {precision} relu={relu}")
            if first is not None:
                assert_same_bits(first, got, "conv3x3_image run to run", ("row", "channel"))
            first = got


@functools.lru_cache(maxsize=None)
def _upconv_case(shape):
    B, h, w, C, O = shape
    g = _gen(B * 1000 + h * 100 + C + O + 1)
    x = torch.randn(B, C, h, w, generator=g)
    wt = torch.randn(C, O, 2, 2, generator=g) / C ** 0.5
    bias = torch.randn(O, generator=g)
    return x, wt, bias, _rows(F.conv_transpose2d(x.double(), wt.double(), bias.double(), stride=2))


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("case", sorted(UPCONV))
def test_upconv2x2(lib, dev, case, precision):
    """Every output pixel is written exactly once: a pixel the epilogue misses keeps FILL (3.4e38) and fails the comparison."""
    shape = UPCONV[case][0]
    B, h, w, C, O = shape
    x, wt, bias, ref = _upconv_case(shape)
    pc = _lib.PRECISIONS[precision]
    w_op = to_operand(M._rows_up2x2(wt.to(dev)).contiguous(), pc)
    b_d = bias.to(dev)
    inbuf, in_ptr, ld_in = _slice_in(_rows(x), dev)
    first = None
    for _ in range(2):
        outbuf, out_ptr, ld_out, pl = _slice_out(B * 4 * h * w, O, dev, pad_left=0, pad_right=O)
        assert ld_out == 2 * O
        rc = lib.ocm_op_upconv2x2(pc, in_ptr, ld_in, w_op.data_ptr(), b_d.data_ptr(), out_ptr, ld_out, B, h, w, C, O, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        got = _check_out(outbuf, pl, O, ref, TOL[precision], f"upconv2x2 {shape} {precision}")
        if first is not None:
            assert_same_bits(first, got, "upconv2x2 run to run", ("row", "channel"))
        first = got
    assert bool(torch.isnan(inbuf[:, :4]).all()) and bool(torch.isnan(inbuf[:, 4 + C:]).all())


@functools.lru_cache(maxsize=None)
def _linear_case(shape, precision):
    Mr, N, K = shape
    g = _gen(Mr + N + K)
    a = torch.randn(Mr, K, generator=g)
    wt = torch.randn(N, K, generator=g) / K ** 0.5
    bias = torch.randn(N, generator=g)
    rnd = ROUNDING[precision] or (lambda t: t)
    return a, wt, bias, (rnd(a).double() @ rnd(wt).double().T + bias.double()).clamp_min(0)


@pytest.mark.parametrize("precision,shape", LINEAR, ids=lambda v: v if isinstance(v, str) else "m%d_n%d_k%d" % v)
def test_linear_relu_into_the_skip_slice(lib, dev, precision, shape):
    """Columns [N, 2 N) of a 2 N-wide buffer, the way e4.conv2 writes its skip: the left half keeps its bits."""
    Mr, N, K = shape
    a, wt, bias, ref = _linear_case(shape, precision)
    pc = _lib.PRECISIONS[precision]
    a_op, w_op, b_d = to_operand(a.to(dev), pc), to_operand(wt.to(dev), pc), bias.to(dev)
    first = None
    for _ in range(2):
        outbuf, out_ptr, ld_out, pl = _slice_out(Mr, N, dev, pad_left=N, pad_right=0)
        assert ld_out == 2 * N
        rc = lib.ocm_op_linear_relu(pc, a_op.data_ptr(), w_op.data_ptr(), b_d.data_ptr(), out_ptr, ld_out, Mr, N, K, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        got = _check_out(outbuf, pl, N, ref, TOL[precision], f"linear_relu {shape} {precision}")
        if first is not None:
            assert_same_bits(first, got, "linear_relu run to run", ("row", "channel"))
        first = got


@pytest.mark.parametrize("case", sorted(POOL))
def test_maxpool2x2(lib, dev, case):
    """Bit equality with F.max_pool2d on half-integers (ties in most windows), -0 / +0 ties and NaNs."""
    B, h, w, C, pad_left, pad_right = POOL[case]
    g = _gen(h * w + C)
    x = torch.randint(-7, 3, (B, C, h, w), generator=g).float() / 2  # mostly negative
    x[:, ::3, 0::2, 0::2] = 0.0
    x[:, ::3, 0::2, 1::2] = -0.0
    x[:, ::3, 1::2, :] = -0.0
    x[:, 1::3, 1::4, 1::6] = float("nan")
    ref = _rows(F.max_pool2d(x, 2)).view(torch.int32)
    inbuf, in_ptr, ld_in = _slice_in(_rows(x), dev, pad_left, pad_right)
    rows_out = B * (h // 2) * (w // 2)
    outs = []
    for _ in range(2):
        outbuf, out_ptr, ld_out, pl = _slice_out(rows_out, C, dev)
        rc = lib.ocm_op_maxpool2x2(in_ptr, ld_in, out_ptr, ld_out, B, h, w, C, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        others = torch.cat([outbuf[:, :pl], outbuf[:, pl + C:]], dim=1)
        assert bool((others == FILL).all())
        outs.append(outbuf[:, pl:pl + C].clone())
    unwritten = int((outs[0] == FILL).sum())
    print(f"GPUTEST maxpool2x2 {POOL[case][:4]} ld_in={ld_in}: {rows_out * C // 4} lanes, {unwritten} elements left unwritten")
    assert unwritten == 0, f"{unwritten} of {rows_out * C} output elements still hold the fill pattern"
    assert_same_bits(outs[0].cpu(), ref, "maxpool2x2 against F.max_pool2d", ("row", "channel"))
    assert_same_bits(outs[0], outs[1], "maxpool2x2 run to run")


@pytest.mark.parametrize("case", sorted(PLANES))
def test_conv1x1_planes(lib, dev, case):
    B, hw, C, with_bias = PLANES[case]
    g = _gen(hw + C)
    rows = torch.randn(B * hw, C, generator=g)
    wv, bias = torch.randn(C, generator=g), torch.randn(1, generator=g)
    ref = rows.double() @ wv.double() + (bias.double() if with_bias else 0.0)
    inbuf, in_ptr, ld_in = _slice_in(rows, dev)
    w_d, b_d = wv.to(dev), bias.to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((B * hw + 64,), float("nan"), device=dev)  # 64 floats past the planes stay NaN
        rc = lib.ocm_op_conv1x1_planes(in_ptr, ld_in, w_d.data_ptr(), b_d.data_ptr() if with_bias else None, out.data_ptr(), B, hw, C, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[B * hw:]).all()), "conv1x1_planes wrote past its planes"
        outs.append(out[:B * hw])
    assert bool(torch.isfinite(outs[0]).all()), "non-finite output (a row was not written, or a NaN column was read)"
    err = float((outs[0].cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"GPUTEST conv1x1_planes rows={B * hw} C={C} bias={with_bias}: relative error {err:.3e} (bound {TOL['fp32']:.0e})")
    assert err <= TOL["fp32"], f"conv1x1_planes relative error {err:.3e}"
    assert_same_bits(outs[0], outs[1], "conv1x1_planes run to run")
