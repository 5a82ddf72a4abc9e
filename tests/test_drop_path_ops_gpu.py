"""ocm_op_drop_path_layernorm and ocm_op_drop_path_backward (kernels_drop_path.hip), bit for bit: the residual sum against numpy's
fp32 x + branch * scale (product rounded, then the sum), the LayerNorm output against ocm_op_layernorm of that sum in the three
output kinds, the in-place forms, the backward's fp32 output against numpy and its operand output against ocm_op_cast_bf16 /
ocm_op_cast_split, and the refusals. Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu

# (batch, tokens, dim): 15 rows are no multiple of the 8-row and 4-row workgroups and put two images inside one workgroup;
# 192 and 96 take the generic-width kernel, the others the 16-byte one
SHAPES = [(3, 5, 128), (2, 17, 384), (2, 9, 256), (3, 5, 192), (2, 9, 96), (1, 3, 1024)]
KINDS = {"f32": (_lib.OCM_LN_F32, torch.float32), "bf16": (_lib.OCM_LN_BF16, torch.bfloat16),
         "split": (_lib.OCM_LN_SPLIT, torch.int32)}
EPS = 1e-6
KEEP = 0.75


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _inputs(shape):
    """x with a large row mean (+50: the two-pass statistics matter), a branch, scales holding a 0, a 1 / keep and 1.7."""
    B, N, D = shape
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + D)
    x = torch.randn(B, N, D, generator=g) + 50.0
    br = torch.randn(B, N, D, generator=g) * 3.0
    table = {3: [1.0 / KEEP, 0.0, 1.7], 2: [1.7, 0.0] if D == 384 else [0.0, 1.0 / KEEP], 1: [1.7]}
    scale = torch.tensor(table[B], dtype=torch.float32)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    return x, br, scale, gamma, beta


def _expected_sum(x, br, scale):
    prod = (br.numpy() * scale.numpy()[:, None, None]).astype(np.float32)  # rounded product, then the rounded sum
    return torch.from_numpy(x.numpy() + prod)


def _layernorm(lib, x, gamma, beta, kind, dtype):
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    D = x.shape[-1]
    _lib.check(lib.ocm_op_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), kind, x.numel() // D, D, EPS,
                                    None))
    return y


def _fused(lib, x, br, scale, gamma, beta, x_out, kind, dtype):
    B, N, D = x.shape
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.check(lib.ocm_op_drop_path_layernorm(x.data_ptr(), br.data_ptr(), scale.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                              x_out.data_ptr(), y.data_ptr(), kind, B, N, D, EPS, None))
    return y


def _bits(t):
    """The tensor as integers of its element width: -0.0 and 0.0 differ, equal NaNs agree."""
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype))


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_is_the_rounded_sum_and_its_layernorm(lib, shape, kind):
    k, dtype = KINDS[kind]
    x, br, scale, gamma, beta = _inputs(shape)
    want_sum = _expected_sum(x, br, scale)
    xd, bd, sd, gd, ed = (t.cuda() for t in (x, br, scale, gamma, beta))
    x_out = torch.full_like(xd, float("nan"))
    y = _fused(lib, xd, bd, sd, gd, ed, x_out, k, dtype)
    torch.cuda.synchronize()
    assert_same_bits(_bits(x_out).cpu(), _bits(want_sum), f"x_out {shape}")
    assert_same_bits(xd.cpu(), x, "x untouched")
    assert_same_bits(bd.cpu(), br, "branch untouched")
    want_y = _layernorm(lib, want_sum.cuda(), gd, ed, k, dtype)
    assert_same_bits(_bits(y).cpu(), _bits(want_y).cpu(), f"y {shape} {kind}")
    # in place over x, and over branch: the same bits
    for which in ("x", "branch"):
        xa, ba = xd.clone(), bd.clone()
        dst = xa if which == "x" else ba
        ya = _fused(lib, xa, ba, sd, gd, ed, dst, k, dtype)
        torch.cuda.synchronize()
        assert_same_bits(_bits(dst).cpu(), _bits(want_sum), f"x_out aliasing {which} {shape}")
        assert_same_bits(_bits(ya).cpu(), _bits(want_y).cpu(), f"y with x_out aliasing {which} {shape} {kind}")


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_scales_and_casts_in_one_pass(lib, shape, prec):
    B, N, D = shape
    pc = _lib.PRECISIONS[prec]
    _, dout, scale, _, _ = _inputs(shape)
    want = torch.from_numpy((dout.numpy() * scale.numpy()[:, None, None]).astype(np.float32))
    dd, sd = dout.cuda(), scale.cuda()
    d32 = torch.full_like(dd, float("nan"))
    if prec == "fp32":
        _lib.check(lib.ocm_op_drop_path_backward(pc, dd.data_ptr(), sd.data_ptr(), d32.data_ptr(), None, B, N, D, None))
        torch.cuda.synchronize()
        assert_same_bits(_bits(d32).cpu(), _bits(want), f"dbranch fp32 {shape}")
        return
    dtype = torch.bfloat16 if prec == "bf16" else torch.int32
    d_op, want_op = torch.empty(dd.shape, dtype=dtype, device="cuda"), torch.empty(dd.shape, dtype=dtype, device="cuda")
    _lib.check(lib.ocm_op_drop_path_backward(pc, dd.data_ptr(), sd.data_ptr(), d32.data_ptr(), d_op.data_ptr(), B, N, D, None))
    cast = lib.ocm_op_cast_bf16 if prec == "bf16" else lib.ocm_op_cast_split
    _lib.check(cast(d32.data_ptr(), want_op.data_ptr(), d32.numel(), None))
    torch.cuda.synchronize()
    assert_same_bits(_bits(d32).cpu(), _bits(want), f"dbranch fp32 {shape}")
    assert_same_bits(_bits(d_op).cpu(), _bits(want_op).cpu(), f"dbranch operand {shape} {prec}")


def test_bad_arguments_are_refused_before_any_launch(lib):
    B, N, D = 2, 3, 48  # 48 % 32 != 0: no split pairs
    t = torch.full((B, N, D), float("nan"), device="cuda")
    p, s, v = t.data_ptr(), torch.ones(B, device="cuda").data_ptr(), torch.ones(D, device="cuda").data_ptr()
    E = _lib.OCM_EINVAL

    def fwd(x=p, br=p, sc=s, g=v, b=v, xo=p, y=p, kind=_lib.OCM_LN_F32, batch=B, tokens=N, dim=D):
        return lib.ocm_op_drop_path_layernorm(x, br, sc, g, b, xo, y, kind, batch, tokens, dim, EPS, None)

    def bwd(prec=_lib.OCM_PREC_FP32, d=p, sc=s, o=p, o_op=None, batch=B, tokens=N, dim=D):
        return lib.ocm_op_drop_path_backward(prec, d, sc, o, o_op, batch, tokens, dim, None)

    assert fwd(kind=_lib.OCM_LN_SPLIT) == E
    for name in ("x", "br", "sc", "g", "b", "xo", "y"):
        assert fwd(**{name: None}) == E, name
    assert fwd(batch=0) == E and fwd(tokens=0) == E and fwd(batch=-1) == E and fwd(tokens=-2) == E
    assert fwd(dim=0) == E and fwd(dim=47) == E and fwd(dim=1026) == E and fwd(kind=3) == E
    assert bwd(prec=_lib.OCM_PREC_BF16X3, o_op=p) == E
    assert bwd(prec=_lib.OCM_PREC_BF16, o_op=None) == E and bwd(prec=7) == E
    for name in ("d", "sc", "o"):
        assert bwd(**{name: None}) == E, name
    assert bwd(batch=0) == E and bwd(tokens=0) == E and bwd(batch=-3) == E and bwd(dim=44) == E
    torch.cuda.synchronize()
    assert torch.isnan(t).all()  # nothing was launched
    assert bwd() == _lib.OCM_OK  # fp32 without an operand output is accepted (in place over dout here)
    torch.cuda.synchronize()
