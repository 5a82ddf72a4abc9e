"""Operators of the decoder backward (kernels_train.hip) against float64 on the CPU, and under the guard / poisoned-workspace
protocol of test_memcheck_gpu.py ((a) OCM_OK, (b) guards intact, (c) outputs fully written, (d) no dependence on the
workspace's previous contents). Needs an MI355X."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.memcheck import assert_same_bits
from tests.test_memcheck_gpu import POISON, _ACT, _spec, check_call
from vit_ocm_wmsegmentation_amd import _lib as L
from vit_ocm_wmsegmentation_amd.engine import to_operand
from vit_ocm_wmsegmentation_amd.model import flip_conv3x3

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-5, "bf16x3": 2e-4, "bf16": 3e-2}  # relative to the reference tensor's max |value|
# (M, N, K): conv1 at stride 8 (D 128 / 384) and 16, conv2 at strides 8 / 16, the 1x1 head; M from 64^2 rows to ~20 k, with
# M one row past a multiple of the 32-row stage and of the slices
WGRAD_SHAPES = [(4096, 256, 1152), (20000, 256, 3456), (196, 1024, 1152), (2305, 64, 2304), (785, 256, 9216),
                (4097, 64, 384), (33, 64, 128)]


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _wgrad(lib, pc, dy, x, want_db=True):
    M, N = dy.shape
    K = x.shape[1]
    nb = lib.ocm_weight_grad_workspace_bytes(M, N, K)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    dw = torch.empty(N, K, device="cuda")
    db = torch.empty(N, device="cuda") if want_db else None
    rc = lib.ocm_op_weight_grad(pc, dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr() if want_db else None, M, N, K,
                                ws.data_ptr(), nb, _s())
    assert rc == 0, lib.ocm_last_error()
    return dw, db


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES)
def test_weight_grad_matches_float64(lib, dev, M, N, K, precision):
    g = torch.Generator().manual_seed(M + N + K)
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    x = (torch.randn(M, K, generator=g, dtype=torch.float64) + 0.5).relu()  # ReLU outputs / im2col zeros, like a2
    want = dy.T @ x
    dw, db = _wgrad(lib, L.PRECISIONS[precision], dy.float().cuda(), x.float().cuda())
    torch.cuda.synchronize()
    assert _rel(dw, want) <= TOL[precision], f"dW rel {_rel(dw, want):.3e}"
    assert _rel(db, dy.sum(0)) <= 2e-5  # the bias gradient is an fp32 column sum in every precision
    dw2, db2 = _wgrad(lib, L.PRECISIONS[precision], dy.float().cuda(), x.float().cuda())
    assert_same_bits(dw, dw2, "dW run to run")
    assert_same_bits(db, db2, "db run to run")


@pytest.mark.parametrize("rows,C,offset", [(4096, 256, 0.0), (18433, 1024, 30.0), (97, 64, 30.0)])
def test_batch_stats_two_pass(lib, dev, rows, C, offset):
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * (0.5 + torch.rand(C, generator=g, dtype=torch.float64))
    x = x + offset * x.std(0)  # a channel mean of 30 sigma: a one-pass E[x^2] - E[x]^2 in fp32 loses the variance
    xf = x.float()
    x64 = xf.double()
    nb = lib.ocm_channel_reduce_workspace_bytes(rows, C)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    mean, var = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    assert lib.ocm_op_batch_stats(xf.cuda().data_ptr(), mean.data_ptr(), var.data_ptr(), rows, C, ws.data_ptr(), nb, _s()) == 0
    torch.cuda.synchronize()
    assert _rel(mean, x64.mean(0)) <= 2e-5
    assert _rel(var, x64.var(0, unbiased=False)) <= 2e-5


def test_pixel_shuffle_backward_is_the_exact_inverse(lib, dev):
    for B, hp, wp, c_out, s in [(2, 8, 8, 1, 8), (1, 14, 14, 1, 16), (3, 5, 7, 3, 4)]:
        lin = torch.randn(B * hp * wp, c_out * s * s, device="cuda")
        out = torch.empty(B, c_out, hp * s, wp * s, device="cuda")
        back = torch.empty_like(lin)
        assert lib.ocm_op_pixel_shuffle(lin.data_ptr(), out.data_ptr(), B, hp, wp, c_out, s, _s()) == 0
        assert lib.ocm_op_pixel_shuffle_backward(out.data_ptr(), back.data_ptr(), B, hp, wp, c_out, s, _s()) == 0
        torch.cuda.synchronize()
        assert_same_bits(back, lin, f"pixel_shuffle_backward(pixel_shuffle(x)) B={B} s={s}")
        want = F.pixel_unshuffle(out.cpu(), s).permute(0, 2, 3, 1).reshape(B * hp * wp, -1)
        assert_same_bits(back.cpu(), want, "pixel_unshuffle")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("B,hp,s", [(2, 8, 8), (1, 14, 16)])
def test_conv2_data_gradient_matches_conv2d_input(lib, dev, B, hp, s, precision):
    """im2col3x3(dY2) . flip(W2)^T on ocm_op_im2col3x3 + ocm_op_linear equals torch.nn.grad.conv2d_input."""
    pc = L.PRECISIONS[precision]
    mid, oc, M = 4 * s * s, s * s, B * hp * hp
    g = torch.Generator().manual_seed(B + s)
    w2 = torch.randn(oc, mid, 3, 3, generator=g, dtype=torch.float64) / (9 * mid) ** 0.5
    dy = torch.randn(B, oc, hp, hp, generator=g, dtype=torch.float64)
    want = torch.nn.grad.conv2d_input((B, mid, hp, hp), w2, dy, padding=1)
    tok = dy.float().permute(0, 2, 3, 1).reshape(M, oc).contiguous().cuda()
    d2 = torch.empty((M, 9 * oc), dtype=_ACT[pc], device="cuda")
    assert lib.ocm_op_im2col3x3(pc, tok.data_ptr(), d2.data_ptr(), B, hp, hp, oc, 0, _s()) == 0
    wf = to_operand(flip_conv3x3(w2.float()).contiguous().cuda(), pc)
    dz = torch.empty((M, mid), device="cuda")
    zero = torch.zeros(mid, device="cuda")
    assert lib.ocm_op_linear(pc, d2.data_ptr(), wf.data_ptr(), zero.data_ptr(), None, dz.data_ptr(), M, mid, 9 * oc,
                             L.OCM_EPI_BIAS_F32, _s()) == 0
    torch.cuda.synchronize()
    got = dz.cpu().double().reshape(B, hp, hp, mid).permute(0, 3, 1, 2)
    assert _rel(got, want) <= TOL[precision]


def _bn_inputs(rows, C, seed):
    """y, mean, invstd, scale, shift with every pre-activation y * scale + shift at least 1e-3 from zero (the ReLU mask is
    then the same in fp32 and float64: fp32 puts it within ~1e-6)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(rows, C, generator=g) * 0.7 + 0.2
    mean, var = y.double().mean(0), y.double().var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    gamma = 1.0 + 0.3 * torch.rand(C, generator=g, dtype=torch.float64)
    beta = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    scale = (gamma * invstd).float()
    shift = (beta - mean * gamma * invstd).float()
    pre = y.double() * scale.double() + shift.double()
    y = torch.where(pre.abs() < 1e-3, y + 3e-3 / scale * torch.sign(pre + 1e-30).float(), y)
    return y, mean.float(), invstd.float(), scale, shift


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_bn_relu_im2col_matches_float64(lib, dev, precision):
    pc = L.PRECISIONS[precision]
    B, h, w, C = 2, 9, 7, 64
    y, _, _, scale, shift = _bn_inputs(B * h * w, C, 3)
    z = (y.double() * scale.double() + shift.double()).relu()
    want = F.unfold(z.reshape(B, h, w, C).permute(0, 3, 1, 2), 3, padding=1)
    want = want.reshape(B, C, 9, h * w).permute(0, 3, 2, 1).reshape(B * h * w, 9 * C)
    out = torch.empty((B * h * w, 9 * C), dtype=_ACT[pc], device="cuda")
    assert lib.ocm_op_bn_relu_im2col3x3(pc, y.cuda().data_ptr(), scale.cuda().data_ptr(), shift.cuda().data_ptr(),
                                        out.data_ptr(), B, h, w, C, _s()) == 0
    ref32 = torch.empty((B * h * w, 9 * C), device="cuda")
    assert lib.ocm_op_bn_relu_im2col3x3(L.OCM_PREC_FP32, y.cuda().data_ptr(), scale.cuda().data_ptr(), shift.cuda().data_ptr(),
                                        ref32.data_ptr(), B, h, w, C, _s()) == 0
    torch.cuda.synchronize()
    assert _rel(ref32, want) <= 2e-6  # one fp32 fma per element
    assert_same_bits(out, to_operand(ref32, pc), f"{precision} operand = the fp32 rows converted")


@pytest.mark.parametrize("rows,C", [(4096, 256), (2305, 1024)])
def test_bn_relu_backward_matches_float64(lib, dev, rows, C):
    y, mean, invstd, scale, shift = _bn_inputs(rows, C, rows)
    dz = torch.randn(rows, C, generator=torch.Generator().manual_seed(5))
    d64, y64 = dz.double(), y.double()
    u = d64 * ((y64 * scale.double() + shift.double()) > 0)
    xh = (y64 - mean.double()) * invstd.double()
    dbeta, dgamma = u.sum(0), (u * xh).sum(0)
    want = scale.double() * (u - dbeta / rows - xh * dgamma / rows)
    cu = [t.cuda() for t in (dz, y, mean, invstd, scale, shift)]
    dy, dg, db = torch.empty(rows, C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    nb = lib.ocm_channel_reduce_workspace_bytes(rows, C)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    assert lib.ocm_op_bn_relu_backward(*[t.data_ptr() for t in cu], dy.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, C,
                                       ws.data_ptr(), nb, _s()) == 0
    torch.cuda.synchronize()
    assert _rel(db, dbeta) <= 2e-5 and _rel(dg, dgamma) <= 2e-5
    assert _rel(dy, want) <= 2e-5


# ---- (a)-(d) of test_memcheck_gpu.py for every new operator ----
@pytest.mark.parametrize("pattern", POISON)
@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", [(2305, 64, 2304), (4097, 256, 1152), (33, 64, 128)])
def test_weight_grad_guarded(lib, dev, M, N, K, precision, pattern):
    pc = L.PRECISIONS[precision]
    g = torch.Generator().manual_seed(M)
    dy, x = torch.randn(M, N, generator=g).cuda(), torch.randn(M, K, generator=g).cuda()
    nb = lib.ocm_weight_grad_workspace_bytes(M, N, K)
    check_call(lib, f"weight_grad {precision} {M}x{N}x{K}",
               lambda p, sc: lib.ocm_op_weight_grad(pc, dy.data_ptr(), x.data_ptr(), p["dw"], p["db"], M, N, K, sc, nb, _s()),
               {"dw": _spec((N, K)), "db": _spec((N,))}, scratch_bytes=nb, pattern=pattern)


@pytest.mark.parametrize("pattern", POISON)
def test_channel_ops_guarded(lib, dev, pattern):
    rows, C = 2305, 256
    y, mean, invstd, scale, shift = [t.cuda() for t in _bn_inputs(rows, C, 9)]
    dz = torch.randn(rows, C, generator=torch.Generator().manual_seed(2)).cuda()
    nb = lib.ocm_channel_reduce_workspace_bytes(rows, C)
    check_call(lib, "batch_stats",
               lambda p, sc: lib.ocm_op_batch_stats(y.data_ptr(), p["mean"], p["var"], rows, C, sc, nb, _s()),
               {"mean": _spec((C,)), "var": _spec((C,))}, scratch_bytes=nb, pattern=pattern)
    check_call(lib, "bn_relu_backward",
               lambda p, sc: lib.ocm_op_bn_relu_backward(dz.data_ptr(), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                                         scale.data_ptr(), shift.data_ptr(), p["dy"], p["dg"], p["db"], rows,
                                                         C, sc, nb, _s()),
               {"dy": _spec((rows, C)), "dg": _spec((C,)), "db": _spec((C,))}, scratch_bytes=nb, pattern=pattern)


@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
def test_bn_relu_im2col_and_pixel_shuffle_backward_guarded(lib, dev, precision):
    pc = L.PRECISIONS[precision]
    B, h, w, Cc = 2, 14, 14, 64
    y, _, _, scale, shift = [t.cuda() for t in _bn_inputs(B * h * w, Cc, 4)]
    check_call(lib, f"bn_relu_im2col3x3 {precision}",
               lambda p, sc: lib.ocm_op_bn_relu_im2col3x3(pc, y.data_ptr(), scale.data_ptr(), shift.data_ptr(), p["y"], B, h,
                                                          w, Cc, _s()),
               {"y": _spec((B * h * w, 9 * Cc), _ACT[pc])})
    s, c_out = 4, 3
    gout = torch.randn(B, c_out, h * s, w * s).cuda()
    check_call(lib, "pixel_shuffle_backward",
               lambda p, sc: lib.ocm_op_pixel_shuffle_backward(gout.data_ptr(), p["y"], B, h, w, c_out, s, _s()),
               {"y": _spec((B * h * w, s * s * c_out))})
