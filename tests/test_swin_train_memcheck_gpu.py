"""The Swin training kernels (kernels_swin_train.hip) on poisoned workspaces and guard-banded outputs (tests/memcheck.py): no store
outside an output, no read of a workspace byte the call did not write, every output byte written. Needs an MI355X."""
import pytest
import torch

from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _run(lib, what, outs, ws_bytes, call):
    """outs: name -> nbytes (fp32). Runs `call(ptrs, ws_ptr)` with outputs / workspace under two fills; returns the outputs."""
    results = []
    for out_fill, ws_fill in (("nan", "big"), ("zero", "unit")):
        g = {k: Guarded(nb, "cuda", out_fill) for k, nb in outs.items()}
        ws = Guarded(ws_bytes, "cuda", ws_fill) if ws_bytes is not None else None
        torch.cuda.synchronize()
        rc = call({k: v.ptr for k, v in g.items()}, ws.ptr if ws is not None else None)
        assert rc == 0, f"{what}: {lib.ocm_last_error().decode()}"
        torch.cuda.synchronize()
        for k, v in g.items():
            assert v.check() is None, f"{what}: {k}: {v.check()}"
        if ws is not None:
            assert ws.check() is None, f"{what}: workspace: {ws.check()}"
        results.append({k: v.payload(torch.float32).clone() for k, v in g.items()})
    for k in outs:
        assert_same_bits(results[0][k], results[1][k], f"{what}: {k} under two output / workspace fills")
    return results[0]


@pytest.mark.parametrize("B,H,ws,shift,heads", [(2, 14, 7, 3, 3), (65, 7, 7, 0, 2), (3, 6, 2, 1, 4)])
def test_window_attention_backward_guarded(lib, B, H, ws, shift, heads):
    T, C = B * H * H, heads * 32
    g = torch.Generator().manual_seed(B + H)
    qkv, dctx = torch.randn(T, 3 * C, generator=g).cuda(), torch.randn(T, C, generator=g).cuda()
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).cuda()
    nbytes = lib.ocm_swin_window_attention_backward_workspace_bytes(B, H, H, ws, heads)
    out = _run(lib, "window_attention_backward", {"dqkv": T * 3 * C * 4, "dtab": table.numel() * 4}, nbytes,
               lambda o, w: lib.ocm_op_swin_window_attention_backward(qkv.data_ptr(), dctx.data_ptr(), table.data_ptr(),
                                                                      o["dqkv"], o["dtab"], B, H, H, ws, shift, heads, w,
                                                                      nbytes, None))
    assert torch.isfinite(out["dqkv"]).all() and torch.isfinite(out["dtab"]).all()


def test_merge_pool_drop_path_guarded(lib):
    B, H, W, Cn = 3, 6, 4, 64
    x = torch.randn(B, H, W, Cn).cuda()
    n = x.numel()
    _run(lib, "merge_gather", {"y": n * 4}, None,
         lambda o, _: lib.ocm_op_swin_merge_gather(x.data_ptr(), o["y"], B, H, W, Cn, None))
    _run(lib, "merge_scatter", {"dx": n * 4}, None,
         lambda o, _: lib.ocm_op_swin_merge_scatter(x.data_ptr(), o["dx"], B, H, W, Cn, None))
    L = H * W
    _run(lib, "pool", {"pooled": B * Cn * 4}, None, lambda o, _: lib.ocm_op_swin_pool(x.data_ptr(), o["pooled"], B, L, Cn, None))
    dp = torch.randn(B, Cn).cuda()
    _run(lib, "pool_backward", {"dx": n * 4}, None,
         lambda o, _: lib.ocm_op_swin_pool_backward(dp.data_ptr(), o["dx"], B, L, Cn, None))
    br, scale = torch.randn(B, H, W, Cn).cuda(), torch.tensor([0.0, 1.25, 1.25]).cuda()
    _run(lib, "drop_path", {"out": n * 4}, None,
         lambda o, _: lib.ocm_op_swin_drop_path(x.data_ptr(), br.data_ptr(), scale.data_ptr(), o["out"], B, L, Cn, None))
    _run(lib, "drop_path_backward", {"dbr": n * 4}, None,
         lambda o, _: lib.ocm_op_swin_drop_path_backward(br.data_ptr(), scale.data_ptr(), o["dbr"], B, L, Cn, None))
