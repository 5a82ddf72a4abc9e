"""Decoder training entry points (include/ocm_vit.h, kernels_train.hip) on the host: argument validation returns OCM_EINVAL
before anything reaches a device, and the host-side kernel flip of conv2's data gradient (model.flip_conv3x3) agrees with
torch.nn.grad.conv2d_input in float64. No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

from vit_ocm_wmsegmentation_amd import _lib as L
from vit_ocm_wmsegmentation_amd.model import flip_conv3x3

P = 256  # a non-null pointer value: validation fails before any pointer is used


def _ws(lib, M, N, K):
    return lib.ocm_weight_grad_workspace_bytes(M, N, K)


@pytest.mark.parametrize("prec,M,N,K", [(7, 64, 64, 64), (L.OCM_PREC_BF16, 0, 64, 64), (L.OCM_PREC_BF16, 64, 48, 64),
                                        (L.OCM_PREC_FP32, 64, 64, 40), (L.OCM_PREC_BF16X3, 64, 0, 64),
                                        (L.OCM_PREC_BF16X3, -5, 64, 64)])
def test_weight_grad_rejects_bad_shapes(lib, prec, M, N, K):
    rc = lib.ocm_op_weight_grad(prec, P, P, P, None, M, N, K, P, 1 << 30, None)
    assert rc == L.OCM_EINVAL, lib.ocm_last_error()


def test_weight_grad_rejects_null_and_small_workspace(lib):
    assert lib.ocm_op_weight_grad(L.OCM_PREC_FP32, None, P, P, None, 64, 64, 64, P, 1 << 30, None) == L.OCM_EINVAL
    assert lib.ocm_op_weight_grad(L.OCM_PREC_FP32, P, P, None, None, 64, 64, 64, P, 1 << 30, None) == L.OCM_EINVAL
    need = _ws(lib, 20000, 256, 3456)
    assert need >= 2 * 256 * 3456 * 4  # M is split: at least two fp32 slabs of dW
    assert lib.ocm_op_weight_grad(L.OCM_PREC_BF16, P, P, P, P, 20000, 256, 3456, P, need - 4, None) == L.OCM_ENOMEM
    assert lib.ocm_op_weight_grad(L.OCM_PREC_BF16, P, P, P, P, 20000, 256, 3456, None, need, None) == L.OCM_ENOMEM


def test_workspace_queries():
    lib = L.load()
    assert lib.ocm_weight_grad_workspace_bytes(0, 64, 64) == 0
    assert lib.ocm_channel_reduce_workspace_bytes(0, 64) == 0
    assert lib.ocm_channel_reduce_workspace_bytes(4096, 256) > 0
    # a function of the shape alone
    assert lib.ocm_weight_grad_workspace_bytes(4097, 64, 384) == lib.ocm_weight_grad_workspace_bytes(4097, 64, 384)


def test_channel_ops_reject_bad_shapes(lib):
    big = 1 << 30
    assert lib.ocm_op_batch_stats(P, P, P, 0, 64, P, big, None) == L.OCM_EINVAL
    assert lib.ocm_op_batch_stats(P, P, P, 64, 0, P, big, None) == L.OCM_EINVAL
    assert lib.ocm_op_batch_stats(None, P, P, 64, 64, P, big, None) == L.OCM_EINVAL
    assert lib.ocm_op_batch_stats(P, P, P, 64, 64, P, 0, None) == L.OCM_ENOMEM
    args = [P] * 9
    assert lib.ocm_op_bn_relu_backward(*args, 64, 66, P, big, None) == L.OCM_EINVAL  # channels % 4
    assert lib.ocm_op_bn_relu_backward(*args, 0, 64, P, big, None) == L.OCM_EINVAL
    assert lib.ocm_op_bn_relu_backward(None, *args[1:], 64, 64, P, big, None) == L.OCM_EINVAL
    assert lib.ocm_op_bn_relu_im2col3x3(L.OCM_PREC_BF16, P, P, P, P, 1, 4, 4, 48, None) == L.OCM_EINVAL  # channels % 32
    assert lib.ocm_op_bn_relu_im2col3x3(L.OCM_PREC_BF16, P, P, P, P, 0, 4, 4, 64, None) == L.OCM_EINVAL
    assert lib.ocm_op_bn_relu_im2col3x3(9, P, P, P, P, 1, 4, 4, 64, None) == L.OCM_EINVAL
    assert lib.ocm_op_bn_relu_im2col3x3(L.OCM_PREC_FP32, P, None, P, P, 1, 4, 4, 64, None) == L.OCM_EINVAL
    assert lib.ocm_op_pixel_shuffle_backward(P, P, 1, 4, 4, 1, 0, None) == L.OCM_EINVAL
    assert lib.ocm_op_pixel_shuffle_backward(P, P, 0, 4, 4, 1, 8, None) == L.OCM_EINVAL
    assert lib.ocm_op_pixel_shuffle_backward(None, P, 1, 4, 4, 1, 8, None) == L.OCM_EINVAL


def _im2col3x3(x):
    """Token-major 3x3 / padding-1 operand rows of a (B, C, h, w) map in ocm_op_im2col3x3's K order (ky*3 + kx)*C + c."""
    B, C, h, w = x.shape
    cols = F.unfold(x, 3, padding=1)  # (B, C*9, h*w), index c*9 + ky*3 + kx
    return cols.reshape(B, C, 9, h * w).permute(0, 3, 2, 1).reshape(B * h * w, 9 * C)


@pytest.mark.parametrize("B,O,C,h,w", [(2, 64, 256, 8, 8), (1, 16, 32, 5, 7)])
def test_flip_conv3x3_is_the_data_gradient(B, O, C, h, w):
    g = torch.Generator().manual_seed(B * O + C)
    weight = torch.randn(O, C, 3, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(B, O, h, w, generator=g, dtype=torch.float64)
    want = torch.nn.grad.conv2d_input((B, C, h, w), weight, dy, padding=1)
    got = _im2col3x3(dy) @ flip_conv3x3(weight).T  # (B*h*w, C) token-major
    got = got.reshape(B, h, w, C).permute(0, 3, 1, 2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
