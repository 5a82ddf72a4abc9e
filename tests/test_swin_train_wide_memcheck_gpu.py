"""ocm_op_swin_window_attention_backward_wide on poisoned workspaces and guard-banded outputs (tests/memcheck.py), as
test_swin_train_memcheck_gpu.test_window_attention_backward_guarded does for the windows of 2 to 7: every output byte written,
nothing written outside the outputs, no workspace byte read before it is written, the same bits under both fills. Needs an MI355X."""
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


@pytest.mark.parametrize("B,H,ws,shift,heads", [(2, 24, 12, 6, 2), (1, 18, 9, 4, 1), (33, 12, 12, 0, 1)])
def test_window_attention_backward_wide_guarded(lib, B, H, ws, shift, heads):
    T, C = B * H * H, heads * 32
    g = torch.Generator().manual_seed(B + H)
    qkv, dctx = torch.randn(T, 3 * C, generator=g).cuda(), torch.randn(T, C, generator=g).cuda()
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).cuda()
    nbytes = lib.ocm_swin_window_attention_backward_wide_workspace_bytes(B, H, H, ws, heads)
    assert nbytes > 0
    outs = {"dqkv": T * 3 * C * 4, "dtab": table.numel() * 4}
    results = []
    for out_fill, ws_fill in (("nan", "big"), ("zero", "unit")):
        guarded = {k: Guarded(nb, "cuda", out_fill) for k, nb in outs.items()}
        wsg = Guarded(nbytes, "cuda", ws_fill)
        torch.cuda.synchronize()
        rc = lib.ocm_op_swin_window_attention_backward_wide(qkv.data_ptr(), dctx.data_ptr(), table.data_ptr(),
                                                            guarded["dqkv"].ptr, guarded["dtab"].ptr, B, H, H, ws, shift, heads,
                                                            wsg.ptr, nbytes, None)
        assert rc == 0, lib.ocm_last_error().decode()
        torch.cuda.synchronize()
        for k, v in guarded.items():
            assert v.check() is None, f"{k}: {v.check()}"
        assert wsg.check() is None, f"workspace: {wsg.check()}"
        results.append({k: v.payload(torch.float32).clone() for k, v in guarded.items()})
    for k in outs:
        assert_same_bits(results[0][k], results[1][k], f"{k} under two output / workspace fills")
        assert torch.isfinite(results[0][k]).all()
