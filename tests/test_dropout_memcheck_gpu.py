"""The dropout operators (kernels_dropout.hip) on poisoned, guard-banded outputs (tests/memcheck.py): no store outside an output,
every output byte written, the same bits under two fills. Shapes: 15 rows of 128 (no multiple of the 8-row workgroup of the
16-byte kernel, two images inside one workgroup) and 18 rows of 96 (the generic-width kernel, a partial 4-row workgroup); the
element-wise operators also at 1 731 elements (a last group of three). Needs an MI355X."""
import pytest
import torch

from tests import dropout_ref as R
from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 128), (2, 9, 96)]
KINDS = [("f32", _lib.OCM_LN_F32, 4), ("bf16", _lib.OCM_LN_BF16, 2), ("split", _lib.OCM_LN_SPLIT, 4)]
PRECS = [("fp32", 4), ("bf16", 2), ("bf16x3", 4)]  # bytes per element of the operand output
SEED, SITE, RATE = 2 ** 40 + 7, 1, 0.5
THRESH, INV_KEEP = R.threshold(RATE)
IK = float(INV_KEEP)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


@pytest.fixture(scope="module")
def seeds(lib):
    return torch.tensor([5, SEED], dtype=torch.int64, device="cuda")


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


def _factors(n):
    return torch.from_numpy(R.factors(SEED, n, RATE))


@pytest.mark.parametrize("count", [15 * 128, 18 * 96, 1731])
def test_mask_and_elementwise_operators_guarded(lib, seeds, count):
    f = _factors(count)
    out = _run(lib, "dropout_mask", {"keep": count},
               lambda o: lib.ocm_op_dropout_mask(seeds.data_ptr(), SITE, count, THRESH, o["keep"], None))
    assert torch.equal(out["keep"].cpu(), (f > 0).to(torch.uint8))
    g = torch.Generator().manual_seed(count)
    h, dg = (3 * torch.randn(count, generator=g)).cuda(), torch.randn(count, generator=g).cuda()
    if count % 4 == 0:
        out = _run(lib, "dropout", {"y": count * 4},
                   lambda o: lib.ocm_op_dropout(h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, o["y"], count, None))
        assert torch.equal(out["y"].view(torch.float32).cpu(), h.cpu() * f)
    for name, width in PRECS:
        if name == "bf16x3" and count % 32:
            continue
        out = _run(lib, f"gelu_dropout {name}", {"out": count * width, "out32": count * 4},
                   lambda o: lib.ocm_op_gelu_dropout(_lib.PRECISIONS[name], h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, o["out"],
                                                     o["out32"], count, None))
        g32 = out["out32"].view(torch.float32).cpu()
        assert torch.isfinite(g32).all() and not g32[f == 0].any() and g32[f > 0].any()
    out = _run(lib, "gelu_dropout_backward", {"dh": count * 4, "g32": count * 4},
               lambda o: lib.ocm_op_gelu_dropout_backward(dg.data_ptr(), h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, o["dh"],
                                                          o["g32"], count, None))
    dh = out["dh"].view(torch.float32).cpu()
    assert torch.isfinite(dh).all() and not dh[f == 0].any() and dh[f > 0].any()


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dropout_layernorm_guarded(lib, seeds, shape, scaled):
    B, N, D = shape
    x, br, scale, gamma, beta = _inputs(shape)
    n = x.numel()
    f = _factors(n).reshape(shape)
    for name, kind, width in KINDS:
        out = _run(lib, f"dropout_layernorm {name}", {"x_out": n * 4, "y": n * width},
                   lambda o: lib.ocm_op_dropout_layernorm(x.data_ptr(), br.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK,
                                                          scale.data_ptr() if scaled else None, gamma.data_ptr(), beta.data_ptr(),
                                                          o["x_out"], o["y"], kind, B, N, D, 1e-6, None))
        xo = out["x_out"].view(torch.float32).reshape(B, N, D).cpu()
        assert torch.isfinite(xo).all()
        assert torch.equal(xo[f == 0], x.cpu()[f == 0])  # a dropped element keeps the residual stream's value
        if scaled:
            assert torch.equal(xo[0], x[0].cpu())  # the dropped image keeps its rows


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dropout_backward_guarded(lib, seeds, shape, scaled):
    B, N, D = shape
    _, dout, scale, _, _ = _inputs(shape)
    n = dout.numel()
    f = _factors(n).reshape(shape)
    for name, width in PRECS:
        outs = {"d32": n * 4}
        if name != "fp32":
            outs["d_op"] = n * width
        out = _run(lib, f"dropout_backward {name}", outs,
                   lambda o: lib.ocm_op_dropout_backward(_lib.PRECISIONS[name], dout.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK,
                                                         scale.data_ptr() if scaled else None, o["d32"], o.get("d_op"), B, N, D,
                                                         None))
        d32 = out["d32"].view(torch.float32).reshape(B, N, D).cpu()
        assert torch.isfinite(d32).all() and not d32[f == 0].any()
        want = dout.cpu() * f
        assert torch.equal(d32[1], want[1] * 1.25 if scaled else want[1])
