"""ocm_op_swin_window_attention_backward_wide (windows of 8 to 12, kernels_swin_train.hip) against torch autograd on the float64
window attention (tests.test_swin._window_attention_oracle, transformers' -100 shift mask), inputs built as in
test_swin_train_ops_gpu.test_window_attention_backward_vs_float64, each with a bitwise rerun. Needs an MI355X.

Bound 2e-5 on dqkv and the table gradient, the project's bound for the windows of 2 to 7: a float32 autograd restatement of these
cases on the CPU sits at 3e-7 to 9e-7, and a transposed bias bin moves dqkv by 0.6 to 1.1 and the table gradient by 1.2 to 2.3
relative. The peaked case (q x 3) takes max(2e-5, 3 x the error of its own float32 CPU restatement)."""
import ctypes as C

import pytest
import torch

from tests.test_swin import _window_attention_oracle
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu

BOUND = 2e-5
CASES = [(1, 12, 12, 12, 0, 1),    # one window, five wavefronts
         (2, 24, 24, 12, 6, 2),    # masked and interior windows
         (2, 16, 24, 8, 4, 3),     # 64 positions: no padding keys
         (1, 18, 27, 9, 4, 1),     # 81 positions, odd window
         (2, 20, 10, 10, 5, 2),    # 100 positions
         (1, 22, 22, 11, 5, 4),    # 121 positions, odd window
         (1, 36, 36, 12, 6, 32),   # Swin-B's last-stage head count
         (33, 12, 24, 12, 6, 1)]   # 66 windows: the table sum crosses a first-level chunk


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _wattn_bwd_wide(lib, qkv, dctx, table, B, H, W, ws, shift, heads):
    dqkv = torch.full_like(qkv, float("nan"))
    dtab = torch.full_like(table, float("nan"))
    nbytes = lib.ocm_swin_window_attention_backward_wide_workspace_bytes(B, H, W, ws, heads)
    assert nbytes > 0
    wsb = torch.full((nbytes // 4,), float("nan"), device=qkv.device)
    _lib.check(lib.ocm_op_swin_window_attention_backward_wide(_p(qkv), _p(dctx), _p(table), _p(dqkv), _p(dtab), B, H, W, ws,
                                                              shift, heads, _p(wsb), nbytes, _st()))
    return dqkv, dtab


def _inputs(B, H, W, ws, shift, heads, qgain=1.5):
    C_ = heads * 32
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + shift + heads)
    qkv = torch.randn(B * H * W, 3 * C_, generator=g)
    qkv[:, :2 * C_] *= 1.5
    if qgain != 1.5:
        qkv[:, :C_] *= qgain / 1.5
    dctx = torch.randn(B * H * W, C_, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    return qkv, dctx, table


def _autograd(qkv, dctx, table, B, H, W, ws, shift, heads, dtype):
    q, t = qkv.to(dtype).requires_grad_(True), table.to(dtype).requires_grad_(True)
    _window_attention_oracle(q, B, H, W, heads, ws, shift, t).backward(dctx.to(dtype))
    return q.grad, t.grad


def _rel(got, want):
    return float((got.cpu().double() - want.double()).abs().max() / want.double().abs().max())


@pytest.mark.parametrize("B,H,W,ws,shift,heads", CASES)
def test_window_attention_backward_wide_vs_float64(lib, B, H, W, ws, shift, heads):
    dev = torch.device("cuda:0")
    qkv, dctx, table = _inputs(B, H, W, ws, shift, heads)
    dq64, dt64 = _autograd(qkv, dctx, table, B, H, W, ws, shift, heads, torch.float64)
    got, gtab = _wattn_bwd_wide(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    e, et = _rel(got, dq64), _rel(gtab, dt64)
    print(f"GPUTEST swin wide window attention backward B={B} {H}x{W} ws{ws} shift{shift} heads{heads}: dqkv {e:.2e}, "
          f"table {et:.2e}")
    assert e <= BOUND and et <= BOUND
    again, gtab2 = _wattn_bwd_wide(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    assert torch.equal(again, got) and torch.equal(gtab2, gtab)


def test_window_attention_backward_wide_peaked(lib):
    """q x 3 (scores three times as peaked). The bound comes from the float32 CPU restatement of this same case, never from
    the device's figure."""
    dev = torch.device("cuda:0")
    B, H, W, ws, shift, heads = 2, 24, 24, 12, 6, 2
    qkv, dctx, table = _inputs(B, H, W, ws, shift, heads, qgain=4.5)  # randn x 1.5 x 3
    dq64, dt64 = _autograd(qkv, dctx, table, B, H, W, ws, shift, heads, torch.float64)
    dq32, dt32 = _autograd(qkv, dctx, table, B, H, W, ws, shift, heads, torch.float32)
    r, rt = _rel(dq32, dq64), _rel(dt32, dt64)
    bound, bound_t = max(BOUND, 3 * r), max(BOUND, 3 * rt)
    got, gtab = _wattn_bwd_wide(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    e, et = _rel(got, dq64), _rel(gtab, dt64)
    print(f"GPUTEST swin wide window attention backward peaked: dqkv {e:.2e} (float32 CPU {r:.2e}, bound {bound:.2e}), "
          f"table {et:.2e} (float32 CPU {rt:.2e}, bound {bound_t:.2e})")
    assert e <= bound and et <= bound_t
    again, gtab2 = _wattn_bwd_wide(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    assert torch.equal(again, got) and torch.equal(gtab2, gtab)


def test_window_attention_backward_wide_rejects(lib):
    dev = torch.device("cuda:0")
    x = torch.zeros(2 * 24 * 24, 3 * 96, device=dev)
    d = torch.zeros(2 * 24 * 24, 96, device=dev)
    t = torch.zeros(529, 3, device=dev)
    nbytes = lib.ocm_swin_window_attention_backward_wide_workspace_bytes(2, 24, 24, 12, 3)
    w = torch.zeros(nbytes // 4, device=dev)
    call = lambda *a: lib.ocm_op_swin_window_attention_backward_wide(*a, _p(w), nbytes, _st())  # noqa: E731
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 24, 24, 12, 6, 3) == _lib.OCM_OK  # the accepted call the rejects vary
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 21, 21, 7, 3, 3) == _lib.OCM_EINVAL   # window 7
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 26, 26, 13, 6, 3) == _lib.OCM_EINVAL  # window 13
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 25, 24, 12, 0, 3) == _lib.OCM_EINVAL  # grid not a multiple
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 24, 24, 12, 12, 3) == _lib.OCM_EINVAL  # shift >= window
    assert call(_p(x), None, _p(t), _p(x), _p(t), 2, 24, 24, 12, 6, 3) == _lib.OCM_EINVAL
    assert call(_p(x), _p(d), _p(t), None, _p(t), 2, 24, 24, 12, 6, 3) == _lib.OCM_EINVAL
    assert lib.ocm_op_swin_window_attention_backward_wide(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 24, 24, 12, 6, 3, _p(w),
                                                          nbytes - 4, _st()) == _lib.OCM_EINVAL
    assert lib.ocm_op_swin_window_attention_backward_wide(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 24, 24, 12, 6, 3, None, nbytes,
                                                          _st()) == _lib.OCM_EINVAL
    # the entry points of the windows of 2 to 7 still refuse these windows
    assert lib.ocm_swin_window_attention_backward_workspace_bytes(2, 24, 24, 12, 3) == 0
    assert lib.ocm_swin_window_attention_backward_wide_workspace_bytes(2, 21, 21, 7, 3) == 0
    assert lib.ocm_swin_window_attention_backward_wide_workspace_bytes(2, 26, 26, 13, 3) == 0
