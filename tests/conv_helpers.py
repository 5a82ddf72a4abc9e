"""Shared by test_conv_ops_gpu.py and test_conv_shapes_gpu.py: the float64 reference of a 3x3 convolution case, activation
arguments as column slices of wider buffers (inputs among NaN columns, outputs among columns pre-filled with a bit pattern that
must survive), and the check of every output element against the reference.

Tolerances are relative to the reference's max |value| and are the project's operator bounds (test_linear_probing_train_gpu.py).
"""
import functools

import torch
import torch.nn.functional as F

from tests.memcheck import PATTERNS, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.engine import to_operand

TOL = {"fp32": 2e-5, "bf16x3": 2e-4, "bf16": 3e-2}
PRECS = ("fp32", "bf16x3", "bf16")
FILL = PATTERNS["big"]  # 0x7F7F7F7F: finite, unmistakable

# The shapes of tests/test_conv_shapes_gpu.py (its docstring explains each) with the tile and K steps they dispatch; the same rows
# are asserted without a GPU by tests/test_gemm_plan_host.py.
# name: ((B, h, w, C, O), tile, (steps fp32 / split-bf16, steps bf16))
CONV = {
    "t128_c64": ((3, 105, 104, 64, 256), "128x128", (18, 9)),
    "t128_c128": ((1, 181, 181, 128, 256), "128x128", (36, 18)),
    "t128_c256": ((1, 181, 181, 256, 256), "128x128", (72, 36)),
    "t128_c512": ((1, 181, 181, 512, 256), "128x128", (144, 72)),
    "t64x128_c64": ((1, 9, 9, 64, 128), "64x128", (18, 9)),
    "t64x128_c128": ((2, 9, 7, 128, 128), "64x128", (36, 18)),
    "t64x128_c256": ((1, 9, 9, 256, 256), "64x128", (72, 36)),
    "t64_c128": ((2, 5, 7, 128, 64), "64x64", (36, 18)),
    "t64_c256": ((1, 5, 7, 256, 32), "64x64", (72, 36)),
    "t64_c512": ((1, 5, 7, 512, 64), "64x64", (144, 72)),
    "grid_1x1": ((3, 1, 1, 32, 32), "64x64", (9, 5)),
    "grid_1x9": ((1, 1, 9, 64, 64), "64x64", (18, 9)),
    "grid_6x1": ((2, 6, 1, 32, 64), "64x64", (9, 5)),
    "c4096": ((1, 3, 3, 4096, 32), "64x64", (1152, 576)),
    "c4064": ((1, 3, 3, 4064, 32), "64x64", (1143, 572)),
}
UPCONV = {
    "up_c96": ((2, 3, 5, 96, 32), "64x64", (3, 2)),
    "up_1x1": ((1, 1, 1, 32, 32), "64x64", (1, 1)),
    "up_d1": ((1, 2, 2, 1024, 512), "64x64", (32, 16)),
    "up_m70": ((2, 7, 5, 64, 32), "64x128", (2, 1)),
    "up_n256": ((1, 9, 9, 128, 64), "64x128", (4, 2)),
    "up_t128": ((3, 74, 74, 32, 128), "128x128", (1, 1)),
}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _conv_case(shape):
    B, h, w, C, O = shape
    g = _gen(B * 1000 + h * 100 + C + O)
    x = torch.randn(B, C, h, w, generator=g)
    wt = torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** 0.5
    bias = torch.randn(O, generator=g)
    ref = F.conv2d(x.double(), wt.double(), bias.double(), padding=1)
    return x, wt, bias, ref.permute(0, 2, 3, 1).reshape(B * h * w, O)


def _rows(x):
    """(B, C, h, w) -> token-major (B*h*w, C)"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _slice_in(rows, dev, pad_left=4, pad_right=8):
    """rows (M, C) as columns [pad_left, pad_left + C) of a NaN-filled buffer: (buffer, pointer of the slice, ld)"""
    Mr, C = rows.shape
    buf = torch.full((Mr, pad_left + C + pad_right), float("nan"), dtype=torch.float32, device=dev)
    buf[:, pad_left:pad_left + C] = rows.to(dev)
    return buf, buf.data_ptr() + 4 * pad_left, buf.shape[1]


def _slice_out(Mr, O, dev, pad_left=8, pad_right=4):
    buf = torch.full((Mr, pad_left + O + pad_right), FILL - (1 << 32) if FILL >= 1 << 31 else FILL, dtype=torch.int32, device=dev)
    return buf, buf.data_ptr() + 4 * pad_left, buf.shape[1], pad_left


def _check_out(buf, pad_left, O, ref, tol, what):
    got = buf[:, pad_left:pad_left + O].view(torch.float32).cpu().double()
    others = torch.cat([buf[:, :pad_left], buf[:, pad_left + O:]], dim=1)
    assert bool((others == FILL).all()), f"{what}: columns outside the output slice were written"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output (a NaN column of the input buffer was read?)"
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"GPUTEST {what}: relative error {err:.3e} (bound {tol:.0e})")
    assert err <= tol, f"{what}: relative error {err:.3e} > {tol:.0e}"
    return buf[:, pad_left:pad_left + O].clone()


def _run_conv3x3(lib, dev, shape, precision):
    B, h, w, C, O = shape
    x, wt, bias, ref = _conv_case(shape)
    pc = _lib.PRECISIONS[precision]
    w_op = to_operand(M._rows3x3(wt.to(dev)).contiguous(), pc)
    b_d = bias.to(dev)
    inbuf, in_ptr, ld_in = _slice_in(_rows(x), dev)
    for relu in (0, 1):
        want = ref.clamp_min(0) if relu else ref
        first = None
        for _ in range(2):
            outbuf, out_ptr, ld_out, pl = _slice_out(B * h * w, O, dev)
            rc = lib.ocm_op_conv3x3(pc, in_ptr, ld_in, w_op.data_ptr(), b_d.data_ptr(), out_ptr, ld_out, B, h, w, C, O, relu, _s())
            assert rc == 0, lib.ocm_last_error()
            torch.cuda.synchronize()
            got = _check_out(outbuf, pl, O, want, TOL[precision], f"conv3x3 {shape} {precision} relu={relu}")
            if first is not None:
                assert_same_bits(first, got, "conv3x3 run to run", ("row", "channel"))
            first = got
    assert bool(torch.isnan(inbuf[:, :4]).all()) and bool(torch.isnan(inbuf[:, 4 + C:]).all())
