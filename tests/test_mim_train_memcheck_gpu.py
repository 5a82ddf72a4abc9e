"""The encoder-backward kernels on poisoned workspaces and guard-banded outputs (tests/memcheck.py): no store outside an output,
no read of a workspace byte the call did not write (the outputs are the same bits whatever the workspace held), every output
byte written (outputs pre-filled with two patterns end up equal). Needs an MI355X."""
import pytest
import torch

from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _run(lib, what, outs, ws_bytes, call):
    """outs: name -> (nbytes, dtype). Runs `call(ptrs, ws_ptr)` with outputs / workspace under two fills; returns the outputs."""
    results = []
    for out_fill, ws_fill in (("nan", "big"), ("zero", "unit")):
        g = {k: Guarded(nb, "cuda", out_fill) for k, (nb, _) in outs.items()}
        ws = Guarded(ws_bytes, "cuda", ws_fill) if ws_bytes is not None else None
        torch.cuda.synchronize()
        rc = call({k: v.ptr for k, v in g.items()}, ws.ptr if ws is not None else None)
        assert rc == 0, f"{what}: {lib.ocm_last_error().decode()}"
        torch.cuda.synchronize()
        for k, v in g.items():
            assert v.check() is None, f"{what}: {k}: {v.check()}"
        if ws is not None:
            assert ws.check() is None, f"{what}: workspace: {ws.check()}"
        results.append({k: v.payload(outs[k][1]).clone() for k, v in g.items()})
    for k in outs:
        assert_same_bits(results[0][k], results[1][k], f"{what}: {k} under two output / workspace fills")
    return results[0]


@pytest.mark.parametrize("hd,N", [(64, 65), (128, 197), (128, 33)])
def test_attention_backward_guarded(lib, hd, N):
    B, H = 2, 3
    D = H * hd
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(3, B, H, N, hd, generator=g).cuda()
    do = torch.randn(B * N, D, generator=g).cuda()
    lse = (torch.randn(B * H, N, generator=g) + 8).cuda()
    delta = torch.randn(B * H, N, generator=g).cuda()
    out = _run(lib, "attention_backward", {"dqkv": (B * N * 3 * D * 4, torch.float32)}, None,
               lambda o, _: lib.ocm_op_attention_backward(qkv.data_ptr(), lse.data_ptr(), do.data_ptr(), delta.data_ptr(),
                                                         o["dqkv"], B, N, H, hd, hd ** -0.5, None))
    assert torch.isfinite(out["dqkv"]).all()
    for name, prec in _lib.PRECISIONS.items():
        ctx = to_operand(torch.randn(B * N, D, generator=g).cuda(), prec)
        _run(lib, f"attention_backward_delta[{name}]", {"delta": (B * H * N * 4, torch.float32),
                                                        "ctx32": (B * N * D * 4, torch.float32)}, None,
             lambda o, _: lib.ocm_op_attention_backward_delta(prec, ctx.data_ptr(), do.data_ptr(), o["delta"], o["ctx32"], B, N,
                                                              H, hd, None))


def test_layernorm_backward_guarded(lib):
    rows, dim = 777, 384
    g = torch.Generator().manual_seed(1)
    x, dy, res = (torch.randn(rows, dim, generator=g).cuda() for _ in range(3))
    w = torch.randn(dim, generator=g).cuda()
    nbytes = lib.ocm_layernorm_backward_workspace_bytes(rows, dim)
    _run(lib, "layernorm_backward", {"dx": (rows * dim * 4, torch.float32), "dg": (dim * 4, torch.float32),
                                     "db": (dim * 4, torch.float32)}, nbytes,
         lambda o, ws: lib.ocm_op_layernorm_backward(dy.data_ptr(), x.data_ptr(), w.data_ptr(), res.data_ptr(), o["dx"], o["dg"],
                                                     o["db"], rows, dim, 1e-6, ws, nbytes, None))


def test_gelu_kernels_guarded(lib):
    n = 96 * 1536
    g = torch.Generator().manual_seed(2)
    h, dg = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    for prec, esz in ((_lib.OCM_PREC_BF16, 2), (_lib.OCM_PREC_FP32, 4), (_lib.OCM_PREC_BF16X3, 4)):
        _run(lib, f"gelu[{prec}]", {"out": (n * esz, torch.uint8), "out32": (n * 4, torch.float32)}, None,
             lambda o, _: lib.ocm_op_gelu(prec, h.data_ptr(), o["out"], o["out32"], n, None))
    _run(lib, "gelu_backward", {"dh": (n * 4, torch.float32), "g32": (n * 4, torch.float32)}, None,
         lambda o, _: lib.ocm_op_gelu_backward(dg.data_ptr(), h.data_ptr(), o["dh"], o["g32"], n, None))


def test_patch_kernels_guarded(lib):
    B, hp, D, p, Cc = 3, 5, 128, 8, 3
    N = hp * hp + 1
    g = torch.Generator().manual_seed(3)
    dt = torch.randn(B, N, D, generator=g).cuda()
    w = (torch.rand(B, N - 1, generator=g) < 0.5).float().cuda()
    img = torch.rand(B, Cc, hp * p, hp * p, generator=g).cuda()
    nbytes = lib.ocm_patch_embed_backward_workspace_bytes(B, N, D)
    _run(lib, "patch_embed_backward", {"dpatch": (B * (N - 1) * D * 4, torch.float32), "dmask": (D * 4, torch.float32),
                                       "dpos": (N * D * 4, torch.float32)}, nbytes,
         lambda o, ws: lib.ocm_op_patch_embed_backward(dt.data_ptr(), w.data_ptr(), o["dpatch"], o["dmask"], o["dpos"], B, N, D,
                                                       ws, nbytes, None))
    _run(lib, "patch_unfold", {"cols": (B * hp * hp * Cc * p * p * 4, torch.float32)}, None,
         lambda o, _: lib.ocm_op_patch_unfold(img.data_ptr(), o["cols"], B, Cc, hp * p, hp * p, p, None))
