"""The dropout operators (kernels_dropout.hip), bit for bit: the device mask against the numpy restatement of csrc/philox.h
(tests/dropout_ref.py); ocm_op_dropout against numpy's rounded product, signed zeros included; ocm_op_dropout_layernorm's sum
against numpy's three rounded steps and its LayerNorm against ocm_op_layernorm of that sum; the backward and the GELU pair against
the chains of operators they replace; every refusal. Shapes are tests/test_drop_path_ops_gpu.py's. Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dropout_ref as R
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu

# (batch, tokens, dim): 15 rows are no multiple of the 8-row and 4-row workgroups and put two images inside one workgroup;
# 192 and 96 take the generic-width kernel, the others the 16-byte one
SHAPES = [(3, 5, 128), (2, 17, 384), (2, 9, 256), (3, 5, 192), (2, 9, 96), (1, 3, 1024)]
GELU_COUNTS = [32, 96, 4128] + [b * n * d for b, n, d in SHAPES]
KINDS = {"f32": (_lib.OCM_LN_F32, torch.float32), "bf16": (_lib.OCM_LN_BF16, torch.bfloat16),
         "split": (_lib.OCM_LN_SPLIT, torch.int32)}
EPS = 1e-6
RATE = 0.25
SEEDS = [2 ** 40 + 7, 61, 2 ** 62 - 1]  # a seed table of three sites: the operators read seeds[site]
SITE = 2
THRESH, INV_KEEP = R.threshold(RATE)
IK = float(INV_KEEP)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


@pytest.fixture(scope="module")
def seeds(lib):
    return torch.tensor(SEEDS, dtype=torch.int64, device="cuda")


def _factors(n, site=SITE):
    return R.factors(SEEDS[site], n, RATE)


def _inputs(shape):
    """x with a large row mean (+50: the two-pass statistics matter), a branch, scales holding a 0, a 1 / keep and 1.7."""
    B, N, D = shape
    g = torch.Generator().manual_seed(B * 1000 + N * 10 + D)
    x = torch.randn(B, N, D, generator=g) + 50.0
    br = torch.randn(B, N, D, generator=g) * 3.0
    table = {3: [4.0 / 3.0, 0.0, 1.7], 2: [1.7, 0.0] if D == 384 else [0.0, 4.0 / 3.0], 1: [1.7]}
    scale = torch.tensor(table[B], dtype=torch.float32)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    return x, br, scale, gamma, beta


def _bits(t):
    """The tensor as integers of its element width: -0.0 and 0.0 differ, equal NaNs agree."""
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _dropout(lib, seeds, x, y=None, site=SITE):
    y = torch.empty_like(x) if y is None else y
    _lib.check(lib.ocm_op_dropout(x.data_ptr(), seeds.data_ptr(), site, THRESH, IK, y.data_ptr(), x.numel(), None))
    return y


def _cast(lib, t32, prec):
    if prec == "fp32":
        return t32
    out = torch.empty(t32.shape, dtype=torch.bfloat16 if prec == "bf16" else torch.int32, device=t32.device)
    fn = lib.ocm_op_cast_bf16 if prec == "bf16" else lib.ocm_op_cast_split
    _lib.check(fn(t32.data_ptr(), out.data_ptr(), t32.numel(), None))
    return out


# ---- the mask ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1023, 1025, 4099, 2 * 17 * 384])
def test_device_mask_equals_the_numpy_mask(lib, seeds, count):
    for site in range(len(SEEDS)):
        keep = torch.full((count + 8,), 7, dtype=torch.uint8, device="cuda")
        _lib.check(lib.ocm_op_dropout_mask(seeds.data_ptr(), site, count, THRESH, keep.data_ptr(), None))
        torch.cuda.synchronize()
        got = keep.cpu().numpy()
        assert np.array_equal(got[:count], R.keep_mask(SEEDS[site], count, THRESH)), (site, count)
        assert (got[count:] == 7).all()
    host = np.zeros(count, dtype=np.uint8)
    assert lib.ocm_dropout_keep_host(SEEDS[0], 0, count, THRESH, C.c_void_p(host.ctypes.data)) == 0
    assert np.array_equal(host, R.keep_mask(SEEDS[0], count, THRESH))


# ---- y = x * factor -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dropout_is_the_rounded_product(lib, seeds, shape):
    x = _inputs(shape)[1]
    x.view(-1)[::7] = -3.0  # dropped ones of these become -0.0
    x.view(-1)[3::11] = 0.0
    f = _factors(x.numel()).reshape(shape)
    want = torch.from_numpy((x.numpy() * f).astype(np.float32))
    assert bool((torch.signbit(want) & (want == 0)).any()) and bool((want > 0).any())
    xd = x.cuda()
    y = _dropout(lib, seeds, xd, torch.full_like(xd, float("nan")))
    torch.cuda.synchronize()
    assert_same_bits(_bits(y).cpu(), _bits(want), f"dropout {shape}")
    assert_same_bits(xd.cpu(), x, "x untouched")
    _dropout(lib, seeds, xd, xd)  # in place
    torch.cuda.synchronize()
    assert_same_bits(_bits(xd).cpu(), _bits(want), f"dropout in place {shape}")
    other = _dropout(lib, seeds, x.cuda(), site=0)
    assert not torch.equal(other.cpu(), want)  # another site, another mask


# ---- x_out = x + (branch * factor) * scale, y = LayerNorm(x_out) ------------------------------------------------------------------
def _expected_sum(x, br, scale):
    d = (br.numpy() * _factors(br.numel()).reshape(br.shape)).astype(np.float32)
    if scale is not None:
        d = (d * scale.numpy()[:, None, None]).astype(np.float32)
    return torch.from_numpy(x.numpy() + d)


def _layernorm(lib, x, gamma, beta, kind, dtype):
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    D = x.shape[-1]
    _lib.check(lib.ocm_op_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), kind, x.numel() // D, D, EPS,
                                    None))
    return y


def _fused(lib, seeds, x, br, scale, gamma, beta, x_out, kind, dtype):
    B, N, D = x.shape
    y = torch.empty(x.shape, dtype=dtype, device=x.device)
    _lib.check(lib.ocm_op_dropout_layernorm(x.data_ptr(), br.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK,
                                            None if scale is None else scale.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                            x_out.data_ptr(), y.data_ptr(), kind, B, N, D, EPS, None))
    return y


@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layernorm_forward_is_the_rounded_sum_and_its_layernorm(lib, seeds, shape, kind, scaled):
    k, dtype = KINDS[kind]
    x, br, scale, gamma, beta = _inputs(shape)
    if not scaled:
        scale = None
    want_sum = _expected_sum(x, br, scale)
    xd, bd, gd, ed = (t.cuda() for t in (x, br, gamma, beta))
    sd = None if scale is None else scale.cuda()
    x_out = torch.full_like(xd, float("nan"))
    y = _fused(lib, seeds, xd, bd, sd, gd, ed, x_out, k, dtype)
    torch.cuda.synchronize()
    assert_same_bits(_bits(x_out).cpu(), _bits(want_sum), f"x_out {shape}")
    assert_same_bits(xd.cpu(), x, "x untouched")
    assert_same_bits(bd.cpu(), br, "branch untouched")
    want_y = _layernorm(lib, want_sum.cuda(), gd, ed, k, dtype)
    assert_same_bits(_bits(y).cpu(), _bits(want_y).cpu(), f"y {shape} {kind}")
    for which in ("x", "branch"):  # in place over x, and over branch: the same bits
        xa, ba = xd.clone(), bd.clone()
        dst = xa if which == "x" else ba
        ya = _fused(lib, seeds, xa, ba, sd, gd, ed, dst, k, dtype)
        torch.cuda.synchronize()
        assert_same_bits(_bits(dst).cpu(), _bits(want_sum), f"x_out aliasing {which} {shape}")
        assert_same_bits(_bits(ya).cpu(), _bits(want_y).cpu(), f"y with x_out aliasing {which} {shape} {kind}")


# ---- the backward: ocm_op_dropout -> ocm_op_drop_path_backward (or -> the cast) -----------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_equals_dropout_then_drop_path_backward(lib, seeds, shape, prec, scaled):
    B, N, D = shape
    pc = _lib.PRECISIONS[prec]
    _, dout, scale, _, _ = _inputs(shape)
    dd, sd = dout.cuda(), scale.cuda()
    masked = _dropout(lib, seeds, dd)
    want32 = torch.empty_like(dd)
    op_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.int32}[prec]
    if scaled:
        want_op = want32 if prec == "fp32" else torch.empty(dd.shape, dtype=op_dtype, device="cuda")
        _lib.check(lib.ocm_op_drop_path_backward(pc, masked.data_ptr(), sd.data_ptr(), want32.data_ptr(),
                                                 None if prec == "fp32" else want_op.data_ptr(), B, N, D, None))
    else:
        want32 = masked
        want_op = _cast(lib, masked, prec)
    d32 = torch.full_like(dd, float("nan"))
    d_op = d32 if prec == "fp32" else torch.empty(dd.shape, dtype=op_dtype, device="cuda")
    _lib.check(lib.ocm_op_dropout_backward(pc, dd.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, sd.data_ptr() if scaled else None,
                                           d32.data_ptr(), None if prec == "fp32" else d_op.data_ptr(), B, N, D, None))
    torch.cuda.synchronize()
    assert_same_bits(_bits(d32).cpu(), _bits(want32).cpu(), f"dbranch fp32 {shape}")
    assert_same_bits(_bits(d_op).cpu(), _bits(want_op).cpu(), f"dbranch operand {shape} {prec}")
    f = _factors(dout.numel()).reshape(shape)
    ref = (dout.numpy() * f).astype(np.float32)
    if scaled:
        ref = (ref * scale.numpy()[:, None, None]).astype(np.float32)
    assert_same_bits(_bits(d32).cpu(), _bits(torch.from_numpy(ref)), f"dbranch fp32 against numpy {shape}")


# ---- the GELU pair ----------------------------------------------------------------------------------------------------------------
def _gelu_inputs(n):
    g = torch.Generator().manual_seed(n)
    return (3 * torch.randn(n, generator=g)).cuda(), torch.randn(n, generator=g).cuda()


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
@pytest.mark.parametrize("count", GELU_COUNTS)
def test_gelu_dropout_equals_gelu_then_dropout_then_the_cast(lib, seeds, count, prec):
    pc = _lib.PRECISIONS[prec]
    h, _ = _gelu_inputs(count)
    op_dtype = {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": torch.int32}[prec]
    g32, scratch = torch.empty_like(h), torch.empty(count, dtype=op_dtype, device="cuda")
    _lib.check(lib.ocm_op_gelu(pc, h.data_ptr(), scratch.data_ptr(), g32.data_ptr(), count, None))
    want32 = _dropout(lib, seeds, g32)
    want_op = _cast(lib, want32, prec)
    out, out32 = torch.empty(count, dtype=op_dtype, device="cuda"), torch.full_like(h, float("nan"))
    _lib.check(lib.ocm_op_gelu_dropout(pc, h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, out.data_ptr(), out32.data_ptr(),
                                       count, None))
    out_only = torch.empty(count, dtype=op_dtype, device="cuda")
    _lib.check(lib.ocm_op_gelu_dropout(pc, h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, out_only.data_ptr(), None, count,
                                       None))
    torch.cuda.synchronize()
    assert_same_bits(_bits(out32).cpu(), _bits(want32).cpu(), f"gelu_dropout fp32 {count}")
    assert_same_bits(_bits(out).cpu(), _bits(want_op).cpu(), f"gelu_dropout operand {count} {prec}")
    assert_same_bits(_bits(out_only).cpu(), _bits(want_op).cpu(), f"gelu_dropout operand without out_f32 {count} {prec}")


@pytest.mark.parametrize("count", GELU_COUNTS)
def test_gelu_dropout_backward_equals_dropout_then_gelu_backward(lib, seeds, count):
    h, dg = _gelu_inputs(count)
    masked = _dropout(lib, seeds, dg)
    want_dh = torch.empty_like(h)
    _lib.check(lib.ocm_op_gelu_backward(masked.data_ptr(), h.data_ptr(), want_dh.data_ptr(), None, count, None))
    fwd32, scratch = torch.empty_like(h), torch.empty_like(h)
    _lib.check(lib.ocm_op_gelu_dropout(_lib.OCM_PREC_FP32, h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, scratch.data_ptr(),
                                       fwd32.data_ptr(), count, None))
    dh, g32 = torch.full_like(h, float("nan")), torch.full_like(h, float("nan"))
    _lib.check(lib.ocm_op_gelu_dropout_backward(dg.data_ptr(), h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, dh.data_ptr(),
                                                g32.data_ptr(), count, None))
    inplace = dg.clone()
    _lib.check(lib.ocm_op_gelu_dropout_backward(inplace.data_ptr(), h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK,
                                                inplace.data_ptr(), None, count, None))
    torch.cuda.synchronize()
    assert_same_bits(_bits(dh).cpu(), _bits(want_dh).cpu(), f"gelu_dropout_backward dh {count}")
    assert_same_bits(_bits(g32).cpu(), _bits(fwd32).cpu(), f"gelu_dropout_backward g_f32 against the forward's {count}")
    assert_same_bits(_bits(inplace).cpu(), _bits(want_dh).cpu(), f"gelu_dropout_backward dh over dg {count}")


def test_gelu_dropout_takes_counts_that_are_no_multiple_of_four(lib, seeds):
    """ocm_op_gelu's conditions: any positive count for bf16 and fp32. 4099 elements: the last group holds three."""
    count = 4099
    h, dg = _gelu_inputs(count)
    g32 = torch.empty_like(h)
    _lib.check(lib.ocm_op_gelu(_lib.OCM_PREC_FP32, h.data_ptr(), g32.data_ptr(), None, count, None))
    torch.cuda.synchronize()
    want = torch.from_numpy((g32.cpu().numpy() * _factors(count)).astype(np.float32))
    for prec in ("fp32", "bf16"):
        out = torch.full((count + 4,), 7.0, dtype=torch.float32 if prec == "fp32" else torch.bfloat16, device="cuda")
        out32 = torch.full((count + 4,), 7.0, device="cuda")
        _lib.check(lib.ocm_op_gelu_dropout(_lib.PRECISIONS[prec], h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, out.data_ptr(),
                                           out32.data_ptr(), count, None))
        torch.cuda.synchronize()
        assert_same_bits(_bits(out32[:count]).cpu(), _bits(want), f"gelu_dropout {prec} fp32 output")
        assert_same_bits(_bits(out[:count]).cpu(), _bits(want.to(out.dtype)), f"gelu_dropout {prec} output")
        assert bool((out[count:] == 7).all()) and bool((out32[count:] == 7).all())
    dh = torch.full((count + 4,), 7.0, device="cuda")
    g = torch.full((count + 4,), 7.0, device="cuda")
    _lib.check(lib.ocm_op_gelu_dropout_backward(dg.data_ptr(), h.data_ptr(), seeds.data_ptr(), SITE, THRESH, IK, dh.data_ptr(),
                                                g.data_ptr(), count, None))
    torch.cuda.synchronize()
    assert_same_bits(_bits(g[:count]).cpu(), _bits(want), "gelu_dropout_backward g_f32")
    assert bool((dh[count:] == 7).all()) and bool((g[count:] == 7).all()) and bool(torch.isfinite(dh[:count]).all())
    dropped = torch.from_numpy(_factors(count) == 0)
    assert not bool(dh[:count].cpu()[dropped].any()) and bool(dh[:count].cpu()[~dropped].any())


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch(lib, seeds):
    B, N, D = 2, 3, 48  # 48 % 32 != 0: no split pairs
    t = torch.full((B, N, D), float("nan"), device="cuda")
    p, s, v, sp = t.data_ptr(), torch.ones(B, device="cuda").data_ptr(), torch.ones(D, device="cuda").data_ptr(), seeds.data_ptr()
    n = t.numel()
    E = _lib.OCM_EINVAL

    def mask(sd=sp, site=0, count=n, keep=p):
        return lib.ocm_op_dropout_mask(sd, site, count, THRESH, keep, None)

    def drop(x=p, sd=sp, site=0, y=p, count=n):
        return lib.ocm_op_dropout(x, sd, site, THRESH, IK, y, count, None)

    def fwd(x=p, br=p, sd=sp, site=0, sc=s, g=v, b=v, xo=p, y=p, kind=_lib.OCM_LN_F32, batch=B, tokens=N, dim=D):
        return lib.ocm_op_dropout_layernorm(x, br, sd, site, THRESH, IK, sc, g, b, xo, y, kind, batch, tokens, dim, EPS, None)

    def bwd(prec=_lib.OCM_PREC_FP32, d=p, sd=sp, site=0, sc=s, o=p, o_op=None, batch=B, tokens=N, dim=D):
        return lib.ocm_op_dropout_backward(prec, d, sd, site, THRESH, IK, sc, o, o_op, batch, tokens, dim, None)

    def gelu(prec=_lib.OCM_PREC_FP32, h=p, sd=sp, site=0, out=p, out32=None, count=n):
        return lib.ocm_op_gelu_dropout(prec, h, sd, site, THRESH, IK, out, out32, count, None)

    def gelu_bwd(dg=p, h=p, sd=sp, site=0, dh=p, g=None, count=n):
        return lib.ocm_op_gelu_dropout_backward(dg, h, sd, site, THRESH, IK, dh, g, count, None)

    assert mask(sd=None) == E and mask(keep=None) == E and mask(count=0) == E and mask(site=-1) == E
    assert drop(x=None) == E and drop(sd=None) == E and drop(y=None) == E and drop(count=0) == E and drop(count=n - 2) == E
    assert drop(site=-1) == E
    assert fwd(kind=_lib.OCM_LN_SPLIT) == E
    for name in ("x", "br", "sd", "g", "b", "xo", "y"):
        assert fwd(**{name: None}) == E, name
    assert fwd(batch=0) == E and fwd(tokens=0) == E and fwd(batch=-1) == E and fwd(tokens=-2) == E and fwd(site=-1) == E
    assert fwd(dim=0) == E and fwd(dim=47) == E and fwd(dim=1026) == E and fwd(kind=3) == E and fwd(kind=-1) == E
    assert bwd(prec=_lib.OCM_PREC_BF16X3, o_op=p) == E
    assert bwd(prec=_lib.OCM_PREC_BF16, o_op=None) == E and bwd(prec=7) == E and bwd(site=-1) == E
    for name in ("d", "sd", "o"):
        assert bwd(**{name: None}) == E, name
    assert bwd(batch=0) == E and bwd(tokens=0) == E and bwd(batch=-3) == E and bwd(dim=44) == E and bwd(dim=0) == E
    assert gelu(prec=7) == E and gelu(h=None) == E and gelu(sd=None) == E and gelu(out=None) == E and gelu(count=0) == E
    assert gelu(prec=_lib.OCM_PREC_BF16X3, count=48) == E and gelu(site=-1) == E
    assert gelu_bwd(dg=None) == E and gelu_bwd(h=None) == E and gelu_bwd(sd=None) == E and gelu_bwd(dh=None) == E
    assert gelu_bwd(count=0) == E and gelu_bwd(site=-1) == E
    torch.cuda.synchronize()
    assert torch.isnan(t).all()  # nothing was launched
    assert fwd(sc=None) == _lib.OCM_OK and bwd(sc=None) == _lib.OCM_OK  # the scale table is optional
    torch.cuda.synchronize()
