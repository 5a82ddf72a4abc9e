"""The byte-moving operators of Swin training on the padded geometries (kernels_swin_train.hip: ocm_op_swin_pad_rows /
_crop_rows, ocm_op_swin_merge_gather_pad / _scatter_pad), bit for bit against F.pad, slicing and the oracle's gather
(oracle.swin_oracle.patch_merging's padding and x0 | x1 | x2 | x3 order). Needs an MI355X."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poison(shape):
    """An output buffer whose every byte must be overwritten: 0xFF bytes (NaN as fp32, never a source value below)."""
    return torch.full(shape, -1, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("row_bytes", [16, 128, 384, 1552])
@pytest.mark.parametrize("B,H,W,Hp,Wp", [(2, 5, 3, 6, 4), (1, 15, 15, 21, 21), (3, 10, 10, 12, 12), (65, 7, 7, 7, 7)])
def test_pad_and_crop_rows_exact(lib, B, H, W, Hp, Wp, row_bytes):
    """Rows as int32 words with no zero word among them (any element format is bytes to these kernels): the pad is F.pad, the
    crop is slicing, crop(pad(x)) is x."""
    n = row_bytes // 4
    g = torch.Generator().manual_seed(B * 100 + H + row_bytes)
    x = torch.randint(1, 2 ** 31 - 1, (B, H, W, n), generator=g, dtype=torch.int32).cuda()
    padded = _poison((B, Hp, Wp, n))
    _lib.check(lib.ocm_op_swin_pad_rows(_p(x), _p(padded), B, H, W, Hp, Wp, row_bytes, _st()))
    assert torch.equal(padded, F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H)))
    xp = torch.randint(1, 2 ** 31 - 1, (B, Hp, Wp, n), generator=g, dtype=torch.int32).cuda()
    cropped = _poison((B, H, W, n))
    _lib.check(lib.ocm_op_swin_crop_rows(_p(xp), _p(cropped), B, H, W, Hp, Wp, row_bytes, _st()))
    assert torch.equal(cropped, xp[:, :H, :W].contiguous())
    back = _poison((B, H, W, n))
    _lib.check(lib.ocm_op_swin_crop_rows(_p(padded), _p(back), B, H, W, Hp, Wp, row_bytes, _st()))
    assert torch.equal(back, x)


def _oracle_gather(x):
    """SwinPatchMerging's input rows as oracle.swin_oracle.patch_merging builds them (one zero row / column on an odd side)."""
    B, H, W, Cn = x.shape
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[:, row::2, col::2, :] for col in range(2) for row in range(2)], dim=-1).reshape(-1, 4 * Cn)


@pytest.mark.parametrize("B,H,W,Cn", [(3, 5, 5, 32), (2, 8, 6, 96), (1, 7, 9, 384), (1, 3, 2, 512), (1, 1, 1, 32)])
def test_merge_gather_scatter_pad_exact(lib, B, H, W, Cn):
    g = torch.Generator().manual_seed(H * 10 + W)
    x = (torch.rand(B, H, W, Cn, generator=g) + 0.5).cuda()  # no zeros: a zero in y is an out-of-grid slot
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    want = _oracle_gather(x)
    y = _poison(want.shape).view(torch.float32)
    _lib.check(lib.ocm_op_swin_merge_gather_pad(_p(x), _p(y), B, H, W, Cn, _st()))
    assert torch.equal(y, want)
    back = _poison(x.shape).view(torch.float32)
    _lib.check(lib.ocm_op_swin_merge_scatter_pad(_p(y), _p(back), B, H, W, Cn, _st()))
    assert torch.equal(back, x)  # scatter(gather(x)) == x
    # the scatter drops what dy holds at the appended row / column: gather(scatter(dy)) is dy with those slots zeroed
    dy = (torch.rand(B * H2 * W2, 4 * Cn, generator=g) + 0.5).cuda()
    dx = _poison(x.shape).view(torch.float32)
    _lib.check(lib.ocm_op_swin_merge_scatter_pad(_p(dy), _p(dx), B, H, W, Cn, _st()))
    again = _poison(dy.shape).view(torch.float32)
    _lib.check(lib.ocm_op_swin_merge_gather_pad(_p(dx), _p(again), B, H, W, Cn, _st()))
    inside = _oracle_gather(torch.ones(B, H, W, Cn, device="cuda"))
    assert torch.equal(again, dy * inside)
    assert int((inside == 0).sum()) == B * Cn * (4 * H2 * W2 - H * W)
    # the transpose of the gather: autograd's gradient of the oracle's gather (one source per element: no sum, no rounding)
    xr = x.clone().requires_grad_(True)
    _oracle_gather(xr).backward(dy)
    assert torch.equal(dx, xr.grad)
    if H % 2 == 0 and W % 2 == 0:  # the bits of the existing even-sided pair
        y0, dx0 = _poison(want.shape).view(torch.float32), _poison(x.shape).view(torch.float32)
        _lib.check(lib.ocm_op_swin_merge_gather(_p(x), _p(y0), B, H, W, Cn, _st()))
        _lib.check(lib.ocm_op_swin_merge_scatter(_p(dy), _p(dx0), B, H, W, Cn, _st()))
        assert torch.equal(y, y0) and torch.equal(dx, dx0)
    else:
        assert lib.ocm_op_swin_merge_gather(_p(x), _p(y), B, H, W, Cn, _st()) == _lib.OCM_EINVAL  # their domain is unchanged
