"""The drop-path operators (kernels_drop_path.hip) on poisoned, guard-banded outputs (tests/memcheck.py): no store outside an
output, every output byte written, the same bits under two fills. Shapes: 15 rows of 128 (no multiple of the 8-row workgroup of
the 16-byte kernel, two images inside one workgroup) and 18 rows of 96 (the generic-width kernel, a partial 4-row workgroup).
Needs an MI355X."""
import pytest
import torch

from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 128), (2, 9, 96)]
KINDS = [("f32", _lib.OCM_LN_F32, 4), ("bf16", _lib.OCM_LN_BF16, 2), ("split", _lib.OCM_LN_SPLIT, 4)]
PRECS = [("fp32", 0), ("bf16", 2), ("bf16x3", 4)]  # bytes per element of the operand output


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _run(lib, what, outs, call):
    """outs: name -> nbytes. Runs `call(ptrs)` with the outputs under two fills; returns the payload bytes of the first."""
    results = []
    for fill in ("nan", "zero"):
        g = {k: Guarded(nb, "cuda", fill) for k, nb in outs.items()}
        torch.cuda.synchronize()
        rc = call({k: v.ptr for k, v in g.items()})
        assert rc == 0, f"{what}: {lib.ocm_last_error().decode()}"
        torch.cuda.synchronize()
        for k, v in g.items():
            assert v.check() is None, f"{what}: {k}: {v.check()}"
        results.append({k: v.payload(torch.uint8).clone() for k, v in g.items()})
    for k in outs:
        assert_same_bits(results[0][k], results[1][k], f"{what}: {k} under two output fills")
    return results[0]


def _inputs(shape):
    B, N, D = shape
    g = torch.Generator().manual_seed(D)
    x, br = (torch.randn(B, N, D, generator=g) + 50.0).cuda(), torch.randn(B, N, D, generator=g).cuda()
    scale = torch.tensor([0.0, 1.25, 1.25][:B]).cuda()
    return x, br, scale, torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_drop_path_layernorm_guarded(lib, shape):
    B, N, D = shape
    x, br, scale, gamma, beta = _inputs(shape)
    n = x.numel()
    for name, kind, width in KINDS:
        out = _run(lib, f"drop_path_layernorm {name}", {"x_out": n * 4, "y": n * width},
                   lambda o: lib.ocm_op_drop_path_layernorm(x.data_ptr(), br.data_ptr(), scale.data_ptr(), gamma.data_ptr(),
                                                            beta.data_ptr(), o["x_out"], o["y"], kind, B, N, D, 1e-6, None))
        xo = out["x_out"].view(torch.float32).reshape(B, N, D)
        assert torch.isfinite(xo).all()
        assert torch.equal(xo[0], x[0])  # the dropped image keeps its rows


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_drop_path_backward_guarded(lib, shape):
    B, N, D = shape
    _, dout, scale, _, _ = _inputs(shape)
    n = dout.numel()
    for name, width in PRECS:
        outs = {"d32": n * 4}
        if width:
            outs["d_op"] = n * width
        out = _run(lib, f"drop_path_backward {name}", outs,
                   lambda o: lib.ocm_op_drop_path_backward(_lib.PRECISIONS[name], dout.data_ptr(), scale.data_ptr(), o["d32"],
                                                           o.get("d_op"), B, N, D, None))
        d32 = out["d32"].view(torch.float32).reshape(B, N, D)
        assert torch.isfinite(d32).all() and not d32[0].any() and torch.equal(d32[1], dout[1] * 1.25)
