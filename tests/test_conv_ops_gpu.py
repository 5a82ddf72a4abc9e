"""The U-Net operators of kernels_conv.hip through the C ABI, in the three precisions, against torch on the CPU in float64.

Tolerances are relative to the reference's max |value| and are the project's operator bounds (test_linear_probing_train_gpu.py).
Every activation argument is exercised as a column slice of a wider buffer: inputs at a non-zero column offset among NaN
columns, outputs among columns pre-filled with a bit pattern that must survive.

Tile dispatch of ocm_op_conv3x3 (kernels_conv.hip: conv_gemm), by rows M = B*h*w and output width O:
  O % 128 == 0 and ceil(M / 128) * (O / 128) >= 512  -> 128 x 128 tiles   (O = 128: M >= 65 409)
  O % 128 == 0 and M > 64                            -> 64 x 128 tiles
  otherwise                                          -> 64 x 64 tiles
CONV_CASES sits one shape on each side of both thresholds.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.conv_helpers import FILL, PRECS, TOL, _check_out, _conv_case, _gen, _rows, _run_conv3x3, _s, _slice_in, _slice_out
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu

# (B, h, w, C, O)
CONV_CASES = {
    "odd_grid": (3, 5, 7, 32, 32),        # no multiple of any tile; tiles span image boundaries
    "k_steps": (2, 8, 8, 96, 64),         # several K steps per tap; bf16: 9 C is no multiple of 64
    "m64_n128": (1, 8, 8, 32, 128),       # M = 64: the last shape on 64 x 64 tiles for O % 128 == 0
    "m4608_n128": (2, 48, 48, 64, 128),   # 64 < M, 36 tiles of 128 x 128 < 512: 64 x 128 tiles
    "m4608_n64": (2, 48, 48, 64, 64),     # the issue's example: 64 x 64 tiles, 18 K steps (compile-time K)
    "m65536_n128": (1, 256, 256, 32, 128),  # 512 tiles of 128 x 128: the first shape on them (M = 65 408 has 511)
}
BOTTLENECK = (1, 2, 2, 1024, 1024)  # K = 9216, every output touches padding; split-bf16 only


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("case", sorted(CONV_CASES))
def test_conv3x3(lib, dev, case, precision):
    _run_conv3x3(lib, dev, CONV_CASES[case], precision)


def test_conv3x3_bottleneck(lib, dev):
    _run_conv3x3(lib, dev, BOTTLENECK, "bf16x3")


@pytest.mark.parametrize("precision", PRECS)
def test_conv3x3_image(lib, dev, precision):
    """B=2, 16x24 window at (5, 3) of channels 1..3 of a larger (2, 5, 40, 50) image: non-contiguous, non-zero origin."""
    B, h, w, O = 2, 16, 24, 64
    g = _gen(77)
    big = torch.randn(2, 5, 40, 50, generator=g)
    view = big[:, 1:4, 5:5 + h, 3:3 + w]
    wt = torch.randn(O, 3, 3, 3, generator=g) / 27 ** 0.5
    bias = torch.randn(O, generator=g)
    ref = F.conv2d(view.double(), wt.double(), bias.double(), padding=1).permute(0, 2, 3, 1).reshape(B * h * w, O)
    pc = _lib.PRECISIONS[precision]
    kp = 64 if precision == "bf16" else 32
    w_op = to_operand(F.pad(M._rows3x3(wt), (0, kp - 27)).to(dev).contiguous(), pc)
    b_d, big_d = bias.to(dev), big.to(dev)
    vd = big_d[:, 1:4, 5:5 + h, 3:3 + w]
    first = None
    for relu in (0, 1, 1):
        outbuf, out_ptr, ld_out, pl = _slice_out(B * h * w, O, dev)
        rc = lib.ocm_op_conv3x3_image(pc, vd.data_ptr(), vd.stride(0), vd.stride(1), vd.stride(2), w_op.data_ptr(), b_d.data_ptr(),
                                      out_ptr, ld_out, B, h, w, O, relu, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        got = _check_out(outbuf, pl, O, ref.clamp_min(0) if relu else ref, TOL[precision], f"conv3x3_image {precision} relu={relu}")
        if relu and first is not None:
            assert_same_bits(first, got, "conv3x3_image run to run", ("row", "channel"))
        first = got if relu else None


def test_maxpool2x2(lib, dev):
    """Bit equality with F.max_pool2d: negative values, ties (also between -0 and +0) and an ld_in > C slice."""
    B, h, w, C = 2, 6, 10, 64
    g = _gen(5)
    x = torch.randn(B, C, h, w, generator=g) - 1.0  # mostly negative
    x = (x * 2).round() / 2                          # many ties
    x[:, ::3, 0::2, 0::2] = 0.0
    x[:, ::3, 0::2, 1::2] = -0.0
    x[:, ::3, 1::2, :] = -0.0
    ref = _rows(F.max_pool2d(x, 2))
    inbuf, in_ptr, ld_in = _slice_in(_rows(x), dev)
    outs = []
    for _ in range(2):
        outbuf, out_ptr, ld_out, pl = _slice_out(B * (h // 2) * (w // 2), C, dev)
        rc = lib.ocm_op_maxpool2x2(in_ptr, ld_in, out_ptr, ld_out, B, h, w, C, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        others = torch.cat([outbuf[:, :pl], outbuf[:, pl + C:]], dim=1)
        assert bool((others == FILL).all())
        outs.append(outbuf[:, pl:pl + C].clone())
    assert_same_bits(outs[0].cpu(), ref.view(torch.int32), "maxpool2x2 against F.max_pool2d", ("row", "channel"))
    assert_same_bits(outs[0], outs[1], "maxpool2x2 run to run")


@pytest.mark.parametrize("precision", PRECS)
def test_upconv2x2(lib, dev, precision):
    """B=2, 3x5, C=64, O=32 into the left half of a 2*O-wide buffer whose right half keeps its bits."""
    B, h, w, C, O = 2, 3, 5, 64, 32
    g = _gen(9)
    x = torch.randn(B, C, h, w, generator=g)
    wt = torch.randn(C, O, 2, 2, generator=g) / C ** 0.5
    bias = torch.randn(O, generator=g)
    ref = _rows(F.conv_transpose2d(x.double(), wt.double(), bias.double(), stride=2))
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
        got = _check_out(outbuf, pl, O, ref, TOL[precision], f"upconv2x2 {precision}")
        if first is not None:
            assert_same_bits(first, got, "upconv2x2 run to run", ("row", "channel"))
        first = got


@pytest.mark.parametrize("precision", PRECS)
def test_linear_relu_into_a_slice(lib, dev, precision):
    """im2col3x3 + linear_relu (the composition build_unet runs at its deepest layers) equals the convolution + ReLU: B=2, 4x4,
    C=64 -> O=64, the output a column slice of a wider buffer."""
    shape = (2, 4, 4, 64, 64)
    B, h, w, C, O = shape
    x, wt, bias, ref = _conv_case(shape)
    pc = _lib.PRECISIONS[precision]
    w_op = to_operand(M._rows3x3(wt.to(dev)).contiguous(), pc)
    b_d, rows = bias.to(dev), _rows(x).to(dev)
    cols = torch.empty((B * h * w, 9 * C), dtype=M._OPERAND_DTYPE[pc], device=dev)
    assert lib.ocm_op_im2col3x3(pc, rows.data_ptr(), cols.data_ptr(), B, h, w, C, 0, _s()) == 0
    first = None
    for _ in range(2):
        outbuf, out_ptr, ld_out, pl = _slice_out(B * h * w, O, dev)
        rc = lib.ocm_op_linear_relu(pc, cols.data_ptr(), w_op.data_ptr(), b_d.data_ptr(), out_ptr, ld_out, B * h * w, O, 9 * C, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        got = _check_out(outbuf, pl, O, ref.clamp_min(0), TOL[precision], f"im2col + linear_relu {precision}")
        if first is not None:
            assert_same_bits(first, got, "linear_relu run to run", ("row", "channel"))
        first = got
    assert lib.ocm_op_linear_relu(pc, cols.data_ptr(), w_op.data_ptr(), b_d.data_ptr(), out_ptr, 32, B * h * w, O, 9 * C, _s()) == _lib.OCM_EINVAL


def test_conv1x1_planes(lib, dev):
    B, hw, C = 2, 35, 64
    g = _gen(13)
    rows = torch.randn(B * hw, C, generator=g)
    wv, bias = torch.randn(C, generator=g), torch.randn(1, generator=g)
    ref = (rows.double() @ wv.double() + bias.double()).reshape(B, 1, hw)
    inbuf, in_ptr, ld_in = _slice_in(rows, dev)
    w_d, b_d = wv.to(dev), bias.to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((B, 1, hw), float("nan"), device=dev)
        rc = lib.ocm_op_conv1x1_planes(in_ptr, ld_in, w_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), B, hw, C, _s())
        assert rc == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        outs.append(out)
    err = float((outs[0].cpu().double() - ref).abs().max() / ref.abs().max())
    assert err <= TOL["fp32"], f"conv1x1_planes relative error {err:.3e}"
    assert_same_bits(outs[0], outs[1], "conv1x1_planes run to run")


def test_bad_arguments_return_einval(lib, dev):
    """Every argument a kernel cannot handle is refused with a message before anything is launched."""
    buf = torch.zeros(4096, device=dev)
    p = buf.data_ptr()
    E = _lib.OCM_EINVAL
    assert lib.ocm_op_conv3x3(2, p, 32, p, p, p, 32, 1, 4, 4, 32, 48, 0, _s()) == E      # O % 32
    assert lib.ocm_op_conv3x3(2, p, 32, p, p, p, 32, 1, 4, 4, 48, 32, 0, _s()) == E      # C % 32
    assert lib.ocm_op_conv3x3(2, p, 34, p, p, p, 32, 1, 4, 4, 32, 32, 0, _s()) == E      # ld_in % 4
    assert lib.ocm_op_conv3x3(2, p, 32, p, p, p, 16, 1, 4, 4, 32, 32, 0, _s()) == E      # ld_out < O
    assert lib.ocm_op_conv3x3(2, p + 4, 32, p, p, p, 32, 1, 4, 4, 32, 32, 0, _s()) == E  # alignment
    assert lib.ocm_op_conv3x3(5, p, 32, p, p, p, 32, 1, 4, 4, 32, 32, 0, _s()) == E      # precision
    assert lib.ocm_op_conv3x3(2, p, 32, p, p, p, 32, 70000, 256, 256, 32, 32, 0, _s()) == E  # rows past 2^31
    assert lib.ocm_op_conv3x3(2, None, 32, p, p, p, 32, 1, 4, 4, 32, 32, 0, _s()) == E
    assert lib.ocm_op_conv3x3_image(2, p, 48, 16, 2, p, p, p, 32, 1, 4, 4, 32, 0, _s()) == E  # stride_y < w
    assert lib.ocm_op_maxpool2x2(p, 32, p, 32, 1, 3, 4, 32, _s()) == E                   # odd h
    assert lib.ocm_op_maxpool2x2(p, 32, p, 32, 1, 4, 4, 30, _s()) == E                   # C % 4
    assert lib.ocm_op_upconv2x2(2, p, 32, p, p, p, 16, 1, 4, 4, 32, 32, _s()) == E       # ld_out < O
    assert lib.ocm_op_conv1x1_planes(p, 64, p, p, p, 1, 0, 64, _s()) == E                # no pixels
    assert lib.ocm_last_error()
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0
