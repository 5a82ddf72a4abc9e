"""Training build_unet, what needs no GPU: the C ABI of the new operators (declared, bound, exported, since version 18), their
argument checks (each returns OCM_EINVAL before anything is launched), the opt-in flag and the chunk rule of the im2col cap."""
import os
import re

import pytest
import torch

from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ocm_op_bn_relu", "ocm_op_maxpool2x2_backward", "ocm_op_upconv2x2_gather", "ocm_op_im2col3x3_image",
       "ocm_conv1x1_planes_backward_workspace_bytes", "ocm_op_conv1x1_planes_backward")
P = 0x10000  # a non-null, 16-byte aligned address: the argument checks never follow it


def test_symbols_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "ocm_vit.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), f"{name} is not declared in include/ocm_vit.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the operators arrived with version 18; library, binding and header name one version, whatever was added since
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION >= 18
    assert "#define OCM_ABI_VERSION %d\n" % _lib.OCM_ABI_VERSION in header


def test_bn_relu_argument_checks(lib):
    E = _lib.OCM_EINVAL
    assert lib.ocm_op_bn_relu(None, P, P, P, 8, 4, 8, None) == E
    assert lib.ocm_op_bn_relu(P, None, P, P, 8, 4, 8, None) == E
    assert lib.ocm_op_bn_relu(P, P, None, P, 8, 4, 8, None) == E
    assert lib.ocm_op_bn_relu(P, P, P, None, 8, 4, 8, None) == E
    assert lib.ocm_op_bn_relu(P, P, P, P, 4, 4, 8, None) == E   # ld_z below the channel count
    assert lib.ocm_op_bn_relu(P, P, P, P, 10, 4, 8, None) == E  # ld_z not a multiple of 4
    assert lib.ocm_op_bn_relu(P, P, P, P, 8, 4, 6, None) == E   # channels % 4
    assert lib.ocm_op_bn_relu(P, P, P, P, 8, 0, 8, None) == E
    assert lib.ocm_op_bn_relu(P, P, P, P + 4, 8, 4, 8, None) == E  # alignment


def test_maxpool2x2_backward_argument_checks(lib):
    E = _lib.OCM_EINVAL
    f = lib.ocm_op_maxpool2x2_backward
    assert f(None, 8, P, 8, P, 8, P, 8, 1, 2, 2, 8, None) == E
    assert f(P, 8, None, 8, P, 8, P, 8, 1, 2, 2, 8, None) == E
    assert f(P, 8, P, 8, P, 8, None, 8, 1, 2, 2, 8, None) == E
    for lds in ((4, 8, 8, 8), (8, 4, 8, 8), (8, 8, 4, 8), (8, 8, 8, 4)):
        assert f(P, lds[0], P, lds[1], P, lds[2], P, lds[3], 1, 2, 2, 8, None) == E
    assert f(P, 8, P, 8, P, 8, P, 8, 1, 2, 2, 6, None) == E  # channels % 4
    assert f(P, 8, P, 8, P, 8, P, 8, 1, 3, 2, 8, None) == E  # odd grid
    assert f(P, 8, P, 8, P, 8, P, 8, 1, 2, 5, 8, None) == E
    assert f(P, 8, P, 8, P, 8, P, 8, 0, 2, 2, 8, None) == E


def test_upconv2x2_gather_argument_checks(lib):
    E = _lib.OCM_EINVAL
    f = lib.ocm_op_upconv2x2_gather
    assert f(None, 8, P, 1, 2, 2, 8, None) == E
    assert f(P, 8, None, 1, 2, 2, 8, None) == E
    assert f(P, 4, P, 1, 2, 2, 8, None) == E  # ld below the channel count
    assert f(P, 8, P, 1, 2, 2, 6, None) == E  # channels % 4
    assert f(P, 8, P, 1, 0, 2, 8, None) == E


def test_im2col3x3_image_argument_checks(lib):
    E = _lib.OCM_EINVAL
    f = lib.ocm_op_im2col3x3_image
    assert f(None, 48, 16, 4, P, 1, 4, 4, None) == E
    assert f(P, 48, 16, 4, None, 1, 4, 4, None) == E
    assert f(P, 48, 16, 3, P, 1, 4, 4, None) == E  # a row stride below the width
    assert f(P, 48, 16, 4, P, 1, 0, 4, None) == E
    assert f(P, 48, 16, 4, P + 8, 1, 4, 4, None) == E


def test_conv1x1_planes_backward_argument_checks(lib):
    E = _lib.OCM_EINVAL
    f = lib.ocm_op_conv1x1_planes_backward
    n = lib.ocm_conv1x1_planes_backward_workspace_bytes(10, 8)
    assert n == 1 * 9 * 4
    assert lib.ocm_conv1x1_planes_backward_workspace_bytes(600, 64) == 3 * 65 * 4  # a function of the shapes: 256 rows per chunk
    assert lib.ocm_conv1x1_planes_backward_workspace_bytes(0, 64) == 0
    assert f(None, P, 8, P, P, 8, P, P, 1, 10, 8, P, n, None) == E
    assert f(P, None, 8, P, P, 8, P, P, 1, 10, 8, P, n, None) == E  # dw wanted, no input rows
    assert f(P, P, 8, None, P, 8, P, P, 1, 10, 8, P, n, None) == E
    assert f(P, P, 8, P, None, 8, P, P, 1, 10, 8, P, n, None) == E
    assert f(P, P, 4, P, P, 8, P, P, 1, 10, 8, P, n, None) == E  # ld_in below the channel count
    assert f(P, P, 8, P, P, 4, P, P, 1, 10, 8, P, n, None) == E  # ld_din below the channel count
    assert f(P, P, 8, P, P, 8, P, P, 1, 10, 6, P, n, None) == E  # channels % 4
    assert f(P, P, 8, P, P, 8, P, P, 0, 10, 8, P, n, None) == E
    assert f(P, P, 8, P, P, 8, P, P, 1, 10, 8, P, n - 1, None) == _lib.OCM_ENOMEM


def test_flag():
    net = M.build_unet()
    assert net.train_backward is False
    assert not any("train_backward" in k for k in net.state_dict())
    assert "train_backward" not in dict(net.named_parameters()) and "train_backward" not in dict(net.named_buffers())
    assert net.enable_training() is net and net.train_backward is True
    assert net.enable_training(False) is net and net.train_backward is False
    sd = M.build_unet().enable_training().state_dict()
    assert set(sd) == set(M.build_unet().state_dict())


def test_refusal_without_the_flag_is_unchanged():
    net = M.build_unet()
    with pytest.raises(NotImplementedError, match=r"\.eval\(\)") as e:
        net(torch.zeros(1, 3, 32, 32))
    assert "build_unet runs inference on the HIP path" in str(e.value) and "enable_training()" in str(e.value)
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"\.eval\(\)"):  # BatchNorm2d in training mode
        net(torch.zeros(1, 3, 32, 32))
    net.enable_training().enable_training(False)
    with pytest.raises(NotImplementedError, match=r"\.eval\(\)"):
        net(torch.zeros(1, 3, 32, 32))


def test_refusals_with_the_flag_need_no_device():
    net = M.build_unet().enable_training()
    with pytest.raises(RuntimeError, match="H=40, W=32"):
        net(torch.zeros(2, 3, 40, 32))
    with pytest.raises(RuntimeError, match=r"\(B, 3, H, W\)"):
        net(torch.zeros(2, 1, 32, 32))
    with pytest.raises(NotImplementedError, match="gradient of the input image"):
        net(torch.zeros(2, 3, 32, 32, requires_grad=True))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        net(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="HIP device"):  # a valid call on a CPU tensor: no CPU fallback
        net(torch.zeros(2, 3, 16, 16))
    net.d2.conv.bn1.eval()
    with pytest.raises(NotImplementedError, match="BatchNorm2d in eval mode"):
        net(torch.zeros(2, 3, 32, 32))
    net.eval()  # eval mode of an opted-in net is the inference path, with its own refusals
    with pytest.raises(RuntimeError, match="HIP device"):
        net(torch.zeros(1, 3, 16, 16))


@pytest.mark.parametrize("batch,rows,k", [(8, 384 * 384, 576), (8, 384 * 384, 32), (8, 24 * 24, 9216), (1, 1 << 22, 1152),
                                          (5, 192 * 192, 1152), (3, 1, 576)])
def test_im2col_chunk_rule(batch, rows, k):
    chunks = M._im2col_chunks(batch, rows, k)
    assert chunks == M._im2col_chunks(batch, rows, k)  # a pure function of the shapes
    assert all(n >= 1 for _, n in chunks)
    covered = [b for b0, n in chunks for b in range(b0, b0 + n)]
    assert covered == list(range(batch))  # every image exactly once, in order
    for _, n in chunks:
        assert n == 1 or n * rows * k * 4 <= M._IM2COL_CAP
    per = max(n for _, n in chunks)
    assert per == batch or (per + 1) * rows * k * 4 > M._IM2COL_CAP  # as many images as fit
    assert M._im2col_chunks(8, 384 * 384, 576) == [(0, 3), (3, 3), (6, 2)]  # e1.conv2 at the bench shape under 1 GiB
