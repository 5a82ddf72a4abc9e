"""The Swin training operators of include/ocm_swin.h (kernels_swin_train.hip) against float64 torch, each with a bitwise rerun:
the window-attention backward (windows 2 to 7, shift on and off, 1 to 32 heads, the relative-position-table bins), the patch-merging
gather / scatter, the pooled head and the drop-path scale. Needs an MI355X."""
import ctypes as C

import pytest
import torch

from oracle import swin_oracle as SO
from tests.test_swin import _window_attention_oracle
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


def _wattn_bwd(lib, qkv, dctx, table, B, H, W, ws, shift, heads):
    dqkv = torch.full_like(qkv, float("nan"))
    dtab = torch.full_like(table, float("nan"))
    nbytes = lib.ocm_swin_window_attention_backward_workspace_bytes(B, H, W, ws, heads)
    wsb = torch.full((nbytes // 4,), float("nan"), device=qkv.device)
    _lib.check(lib.ocm_op_swin_window_attention_backward(_p(qkv), _p(dctx), _p(table), _p(dqkv), _p(dtab), B, H, W, ws, shift,
                                                         heads, _p(wsb), nbytes, _st()))
    return dqkv, dtab


@pytest.mark.parametrize("B,H,W,ws,shift,heads", [(2, 4, 4, 2, 0, 1), (3, 4, 6, 2, 1, 2), (2, 9, 6, 3, 1, 3), (1, 8, 8, 4, 2, 4),
                                                  (2, 10, 5, 5, 2, 2), (3, 12, 12, 6, 3, 3), (2, 14, 14, 7, 3, 3),
                                                  (2, 14, 14, 7, 0, 6), (1, 7, 7, 7, 0, 24), (1, 7, 7, 7, 0, 32),
                                                  (65, 7, 14, 7, 3, 2)])
def test_window_attention_backward_vs_float64(lib, B, H, W, ws, shift, heads):
    """dq | dk | dv and d(relative_position_bias_table) against torch autograd on the float64 window attention (with
    transformers' -100 shift mask); 65 images x 2 windows puts the table sum across two first-level chunks."""
    dev = torch.device("cuda:0")
    C_ = heads * 32
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + shift + heads)
    qkv = torch.randn(B * H * W, 3 * C_, generator=g)
    qkv[:, :2 * C_] *= 1.5
    dctx = torch.randn(B * H * W, C_, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    q64, t64 = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    _window_attention_oracle(q64, B, H, W, heads, ws, shift, t64).backward(dctx.double())
    got, gtab = _wattn_bwd(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    e = float((got.cpu().double() - q64.grad).abs().max() / q64.grad.abs().max())
    et = float((gtab.cpu().double() - t64.grad).abs().max() / t64.grad.abs().max())
    print(f"GPUTEST swin window attention backward B={B} {H}x{W} ws{ws} shift{shift} heads{heads}: dqkv {e:.2e}, table {et:.2e}")
    assert e <= 2e-5 and et <= 2e-5
    again, gtab2 = _wattn_bwd(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    assert torch.equal(again, got) and torch.equal(gtab2, gtab)


def test_window_attention_backward_rejects(lib):
    dev = torch.device("cuda:0")
    x = torch.zeros(2 * 14 * 14, 3 * 96, device=dev)
    d = torch.zeros(2 * 14 * 14, 96, device=dev)
    t = torch.zeros(169, 3, device=dev)
    nbytes = lib.ocm_swin_window_attention_backward_workspace_bytes(2, 14, 14, 7, 3)
    w = torch.zeros(nbytes // 4, device=dev)
    call = lambda *a: lib.ocm_op_swin_window_attention_backward(*a, _p(w), nbytes, _st())  # noqa: E731
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 14, 14, 8, 0, 3) == _lib.OCM_EINVAL  # window 8
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 15, 14, 7, 0, 3) == _lib.OCM_EINVAL  # grid not a multiple
    assert call(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 14, 14, 7, 7, 3) == _lib.OCM_EINVAL  # shift >= window
    assert call(_p(x), None, _p(t), _p(x), _p(t), 2, 14, 14, 7, 3, 3) == _lib.OCM_EINVAL
    assert lib.ocm_op_swin_window_attention_backward(_p(x), _p(d), _p(t), _p(x), _p(t), 2, 14, 14, 7, 3, 3, _p(w), nbytes - 4,
                                                     _st()) == _lib.OCM_EINVAL


@pytest.mark.parametrize("B,H,W,Cn", [(1, 4, 4, 32), (3, 8, 6, 96), (2, 14, 14, 192), (5, 2, 4, 512)])
def test_merge_gather_scatter_exact(lib, B, H, W, Cn):
    """The merging LayerNorm's input (x0 | x1 | x2 | x3, modeling_swin.py:309-326) and its inverse: permutations, bit exact."""
    dev = torch.device("cuda:0")
    x = torch.randn(B, H, W, Cn, device=dev)
    want = torch.cat([x[:, r::2, c::2, :] for c in range(2) for r in range(2)], -1).reshape(-1, 4 * Cn)
    y = torch.full_like(want, float("nan"))
    _lib.check(lib.ocm_op_swin_merge_gather(_p(x), _p(y), B, H, W, Cn, _st()))
    assert torch.equal(y, want)
    back = torch.full_like(x, float("nan"))
    _lib.check(lib.ocm_op_swin_merge_scatter(_p(y), _p(back), B, H, W, Cn, _st()))
    assert torch.equal(back, x)
    assert lib.ocm_op_swin_merge_gather(_p(x), _p(y), B, H + 1, W, Cn, _st()) == _lib.OCM_EINVAL


@pytest.mark.parametrize("B,L,Cn", [(1, 1, 32), (8, 49, 768), (3, 144, 96), (2, 4, 1024)])
def test_pool_and_backward(lib, B, L, Cn):
    dev = torch.device("cuda:0")
    x = torch.randn(B, L, Cn, device=dev) * 2 + 0.5
    pooled = torch.full((B, Cn), float("nan"), device=dev)
    _lib.check(lib.ocm_op_swin_pool(_p(x), _p(pooled), B, L, Cn, _st()))
    assert float((pooled.cpu().double() - x.cpu().double().mean(1)).abs().max()) <= 1e-5
    again = torch.empty_like(pooled)
    _lib.check(lib.ocm_op_swin_pool(_p(x), _p(again), B, L, Cn, _st()))
    assert torch.equal(again, pooled)
    dp = torch.randn(B, Cn, device=dev)
    dx = torch.full_like(x, float("nan"))
    _lib.check(lib.ocm_op_swin_pool_backward(_p(dp), _p(dx), B, L, Cn, _st()))
    want = (dp.double() / L).unsqueeze(1).expand(B, L, Cn)
    assert float((dx.double() - want).abs().max() / want.abs().max()) <= 1e-7  # dp / L rounded once
    assert torch.equal(dx, dx[:, :1].expand(B, L, Cn))  # the same value on every token


@pytest.mark.parametrize("B,L,Cn", [(1, 49, 96), (8, 3136, 96), (3, 16, 512)])
def test_drop_path_and_backward(lib, B, L, Cn):
    dev = torch.device("cuda:0")
    x, br, dout = (torch.randn(B, L, Cn, device=dev) for _ in range(3))
    keep = 0.9
    mask = torch.floor(torch.rand(B, device=dev) + keep)
    mask[0] = 0.0
    scale = mask / keep
    out = torch.full_like(x, float("nan"))
    _lib.check(lib.ocm_op_swin_drop_path(_p(x), _p(br), _p(scale), _p(out), B, L, Cn, _st()))
    want = x.double() + br.double() * scale.double().view(B, 1, 1)
    assert float((out.double() - want).abs().max()) <= 1e-6
    assert torch.equal(out[0], x[0])
    inplace = x.clone()
    _lib.check(lib.ocm_op_swin_drop_path(_p(inplace), _p(br), _p(scale), _p(inplace), B, L, Cn, _st()))
    assert torch.equal(inplace, out)
    dbr = torch.full_like(x, float("nan"))
    _lib.check(lib.ocm_op_swin_drop_path_backward(_p(dout), _p(scale), _p(dbr), B, L, Cn, _st()))
    assert torch.equal(dbr, dout * scale.view(B, 1, 1))
