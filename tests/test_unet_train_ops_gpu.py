"""The operators build_unet's training adds (kernels_conv_train.hip), each on the smallest shapes at which it can go wrong.
Inputs are column slices of wider buffers whose other columns hold NaN; outputs are column slices of guard-banded, NaN-poisoned
payloads (tests/memcheck.py) whose other columns must keep the poison; every operator runs twice and the bits are compared.

Bounds. The gathers and the pool backward are bit exact (the pool backward against the CPU's F.max_pool2d backward plus one fp32
add). ocm_op_bn_relu is one fma: within 2^-23 (|y scale| + |shift|) of float64. The classifier's backward and the up-convolution's
backward, assembled from the gather and the existing GEMMs, are held to the project's operator bounds (conv_helpers.TOL: fp32
2e-5, split-bf16 2e-4, bf16 3e-2 of each output's max)."""
import pytest
import torch
import torch.nn.functional as F

from tests.conv_helpers import PRECS, TOL, _rows, _slice_in
from tests.memcheck import PATTERNS, Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu

NAN_WORD = PATTERNS["nan"] - (1 << 32)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


class _Out:
    """Columns [lo, lo + width) of a guard-banded (rows, ld) payload, everything NaN-poisoned."""

    def __init__(self, rows, width, dev, lo=8, hi=4):
        self.rows, self.width, self.lo, self.ld = rows, width, lo, lo + width + hi
        self.g = Guarded(rows * self.ld * 4, dev, pattern="nan")
        self.view = self.g.payload(torch.int32, (rows, self.ld))
        self.ptr = self.g.ptr + 4 * lo

    def take(self, what):
        """Guards intact, the other columns still poison: the slice's bits as int32 (rows, width) on the CPU."""
        torch.cuda.synchronize()
        assert self.g.check() is None, f"{what}: {self.g.check()}"
        others = torch.cat([self.view[:, :self.lo], self.view[:, self.lo + self.width:]], dim=1)
        assert bool((others == NAN_WORD).all()), f"{what}: columns outside the output slice were written"
        return self.view[:, self.lo:self.lo + self.width].clone().cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f32(bits):
    return bits.view(torch.float32)


# ---- max-pool backward -----------------------------------------------------------------------------------------------------
def _pool_case(B, h, w, C, seed, plant):
    g = _gen(seed)
    z = torch.randn(B, C, h, w, generator=g).clamp_min(0)  # what a ReLU leaves: about half of it zeros, all-zero windows among them
    if plant:
        z[0, 0, 0:2, 0:2] = torch.tensor([[1.5, 1.5], [0.5, 1.5]])      # equal values: the first one keeps the gradient
        z[0, 1, 0:2, 2:4] = torch.tensor([[-0.0, 0.0], [0.0, -0.0]])    # -0 / +0 compare equal
        z[0, 2, 2:4, 0:2] = torch.tensor([[0.0, -0.0], [-0.0, 0.0]])
        z[1, 3, 0:2, 0:2] = 0.0                                         # an all-zero window
        z[1, 4, 2:4, 4:6] = torch.tensor([[2.0, float("nan")], [3.0, 1.0]])   # a NaN wins and keeps winning
        z[1, 5, 0:2, 4:6] = torch.tensor([[2.0, 1.0], [3.0, float("nan")]])   # a NaN in the last position
        z[0, 6, 2:4, 2:4] = torch.tensor([[0.25, 0.5], [0.5, 0.25]])    # the two largest equal, in the middle of the scan
    dpool = torch.randn(B, C, h // 2, w // 2, generator=g)
    add = torch.randn(B, C, h, w, generator=g)
    zc = z.clone().requires_grad_(True)
    F.max_pool2d(zc, 2).backward(dpool)
    return z, dpool, add, zc.grad


def _run_pool_backward(lib, dev, B, h, w, C, seed, plant, z_ld_extra):
    z, dpool, add, want = _pool_case(B, h, w, C, seed, plant)
    Mr = B * h * w
    zbuf, z_ptr, ld_z = _slice_in(_rows(z), dev, pad_left=z_ld_extra, pad_right=0)  # the right part of a wider buffer
    dpbuf, dp_ptr, ld_dp = _slice_in(_rows(dpool), dev)
    abuf, a_ptr, ld_a = _slice_in(_rows(add), dev, pad_left=C, pad_right=0)
    for with_add in (False, True):
        ref = _rows(want + add if with_add else want)  # one fp32 add per element
        first = None
        for _ in range(2):
            out = _Out(Mr, C, dev)
            rc = lib.ocm_op_maxpool2x2_backward(z_ptr, ld_z, dp_ptr, ld_dp, a_ptr if with_add else None, ld_a if with_add else 0,
                                                out.ptr, out.ld, B, h, w, C, _s())
            assert rc == 0, lib.ocm_last_error()
            got = out.take(f"maxpool2x2_backward add={with_add}")
            assert_same_bits(got, _bits(ref), f"maxpool2x2_backward ({B}, {h}, {w}, {C}) add={with_add} vs the CPU", ("row", "channel"))
            if first is not None:
                assert_same_bits(first, got, "maxpool2x2_backward run to run", ("row", "channel"))
            first = got


def test_maxpool2x2_backward_planted_ties(lib, dev):
    _run_pool_backward(lib, dev, 2, 4, 6, 8, 51, True, 8)  # z: the right half of a 2 C buffer


def test_maxpool2x2_backward_second_trip_of_the_grid_stride_loop(lib, dev):
    """65 x 64 windows x 128 lanes = 532 480 lanes against the launch's 2 048 x 256 = 524 288."""
    _run_pool_backward(lib, dev, 1, 130, 128, 512, 52, False, 8)


# ---- the gathers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (1, 1, 5, 4), (3, 2, 2, 36)])
def test_upconv2x2_gather(lib, dev, shape):
    B, h, w, O = shape
    dout = torch.randn(B, O, 2 * h, 2 * w, generator=_gen(61))
    inbuf, in_ptr, ld = _slice_in(_rows(dout), dev)
    want = _rows(dout).reshape(B, h, 2, w, 2, O).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, 4 * O)
    first = None
    for _ in range(2):
        out = _Out(B * h * w, 4 * O, dev, lo=0, hi=0)  # g is dense
        assert lib.ocm_op_upconv2x2_gather(in_ptr, ld, out.ptr, B, h, w, O, _s()) == 0, lib.ocm_last_error()
        got = out.take(f"upconv2x2_gather {shape}")
        assert_same_bits(got, _bits(want), f"upconv2x2_gather {shape} vs torch indexing", ("row", "column"))
        if first is not None:
            assert_same_bits(first, got, "upconv2x2_gather run to run")
        first = got


@pytest.mark.parametrize("shape", [(2, 6, 7), (1, 1, 5), (3, 16, 16)])
def test_im2col3x3_image(lib, dev, shape):
    B, h, w = shape
    big = torch.full((B, 3, h + 3, w + 5), float("nan"))
    img = torch.randn(B, 3, h, w, generator=_gen(62))
    big[:, :, 1:1 + h, 2:2 + w] = img
    view = big.to(dev)[:, :, 1:1 + h, 2:2 + w]  # not contiguous: the strides are the big tensor's
    assert not view.is_contiguous() and view.stride(3) == 1
    cols = F.unfold(img, 3, padding=1).reshape(B, 3, 9, h * w).permute(0, 3, 2, 1).reshape(B * h * w, 27)  # (ky*3 + kx)*3 + c
    want = F.pad(cols, (0, 5))
    first = None
    for _ in range(2):
        out = _Out(B * h * w, 32, dev, lo=0, hi=0)
        rc = lib.ocm_op_im2col3x3_image(view.data_ptr(), view.stride(0), view.stride(1), view.stride(2), out.ptr, B, h, w, _s())
        assert rc == 0, lib.ocm_last_error()
        got = out.take(f"im2col3x3_image {shape}")
        assert_same_bits(got, _bits(want), f"im2col3x3_image {shape} vs unfold", ("row", "column"))
        if first is not None:
            assert_same_bits(first, got, "im2col3x3_image run to run")
        first = got


# ---- BatchNorm affine + ReLU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(37, 12), (300, 8)])
def test_bn_relu_values_and_gate(lib, dev, rows, C):
    g = _gen(71)
    y = torch.randn(rows, C, generator=g)
    scale = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    shift = torch.randn(C, generator=g)
    # rows whose pre-activation is a few ulps either side of 0: y = -shift / scale, moved by k ulps
    root = (-shift / scale)
    for i, k in enumerate((-3, -2, -1, 0, 1, 2, 3)):
        y[2 * i] = _f32(_bits(root) + k)
    pre = y.double() * scale.double() + shift.double()
    assert int(((pre.abs() < 1e-5) & (pre != 0)).sum()) >= 4 * C  # the planted rows do sit next to the threshold
    yd, sd, hd = y.to(dev), scale.to(dev), shift.to(dev)
    first = None
    for _ in range(2):
        out = _Out(rows, C, dev)
        assert lib.ocm_op_bn_relu(yd.data_ptr(), sd.data_ptr(), hd.data_ptr(), out.ptr, out.ld, rows, C, _s()) == 0, lib.ocm_last_error()
        got = out.take("bn_relu")
        if first is not None:
            assert_same_bits(first, got, "bn_relu run to run")
        first = got
    z = _f32(first)
    assert bool(torch.isfinite(z).all()) and bool((z >= 0).all())
    bound = 2.0 ** -23 * ((y.double() * scale.double()).abs() + shift.double().abs())
    err = (z.double() - pre.clamp_min(0)).abs()
    assert bool((err <= bound).all()), f"bn_relu: {float((err - bound).max()):.3e} over the fma's round-off"
    # the gate of the backward: with dz = 1, dbeta[c] counts the rows that pass it — the rows whose z is positive
    ones = torch.ones(rows, C, device=dev)
    zero, one = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dy, dgam, dbet = torch.empty(rows, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
    nbytes = lib.ocm_channel_reduce_workspace_bytes(rows, C)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    rc = lib.ocm_op_bn_relu_backward(ones.data_ptr(), yd.data_ptr(), zero.data_ptr(), one.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                     dy.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), rows, C, ws.data_ptr(), nbytes, _s())
    assert rc == 0, lib.ocm_last_error()
    assert torch.equal(dbet.cpu().to(torch.int64), (z > 0).sum(0)), "the backward's gate and the forward's z > 0 disagree"


# ---- the classifier's backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,hw,C", [(2, 300, 64), (1, 600, 4), (3, 7, 64)])
def test_conv1x1_planes_backward(lib, dev, B, hw, C):
    """600 rows are three chunks of the row split (256 rows a workgroup at the least)."""
    g = _gen(81)
    rows = B * hw
    x, w, dl = torch.randn(rows, C, generator=g), torch.randn(C, generator=g), torch.randn(rows, generator=g)
    inbuf, in_ptr, ld_in = _slice_in(x, dev)
    wd, dld = w.to(dev), dl.to(dev)
    nbytes = lib.ocm_conv1x1_planes_backward_workspace_bytes(rows, C)
    want_din = dl.double()[:, None] * w.double()[None, :]
    want_dw, want_db = dl.double() @ x.double(), dl.double().sum()
    first = None
    for _ in range(2):
        out = _Out(rows, C, dev)
        wsg = Guarded(nbytes, dev, pattern="nan")
        small = Guarded((C + 4) * 4, dev, pattern="nan")  # dw, then db at a 16-byte boundary
        rc = lib.ocm_op_conv1x1_planes_backward(dld.data_ptr(), in_ptr, ld_in, wd.data_ptr(), out.ptr, out.ld, small.ptr,
                                                small.ptr + 4 * C, B, hw, C, wsg.ptr, nbytes, _s())
        assert rc == 0, lib.ocm_last_error()
        din = out.take("conv1x1_planes_backward din")
        assert wsg.check() is None and small.check() is None, (wsg.check(), small.check())
        sm = small.payload(torch.float32).cpu()
        assert bool(torch.isnan(sm[C + 1:]).all())
        got = (din, _bits(sm[:C + 1].clone()))
        if first is not None:
            assert_same_bits(first[0], got[0], "din run to run")
            assert_same_bits(first[1], got[1], "dw, db run to run")
        first = got
    din, dw, db = _f32(first[0]).double(), _f32(first[1])[:C].double(), _f32(first[1])[C].double()
    for name, gv, wv in (("din", din, want_din), ("dw", dw, want_dw)):
        err = float((gv - wv).abs().max() / wv.abs().max())
        print(f"GPUTEST conv1x1_planes_backward rows={rows} C={C} {name}: relative error {err:.3e} (bound {TOL['fp32']:.0e})")
        assert err <= TOL["fp32"], f"{name}: {err:.3e}"
    # db is a sum of `rows` terms of either sign: its error is bounded against the terms' size, sum |dlogits|
    err = float((db - want_db).abs() / dl.double().abs().sum())
    assert err <= TOL["fp32"], f"db: {err:.3e}"
    # frozen weights: no dw, no db, the same din
    out = _Out(rows, C, dev)
    wsg = Guarded(nbytes, dev, pattern="nan")
    rc = lib.ocm_op_conv1x1_planes_backward(dld.data_ptr(), None, 0, wd.data_ptr(), out.ptr, out.ld, None, None, B, hw, C, wsg.ptr,
                                            nbytes, _s())
    assert rc == 0, lib.ocm_last_error()
    assert_same_bits(out.take("din alone"), first[0], "din without dw / db")


# ---- the up-convolution's backward, assembled ------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("shape", [(2, 3, 5, 64, 32), (1, 2, 2, 1024, 512)])
def test_upconv2x2_backward_assembled(lib, dev, shape, precision):
    """gather -> dIn = ocm_op_linear(g, W^T), dW = ocm_op_weight_grad(g, in), db = its db summed over the four groups: what
    _UNetTrain.backward runs, against float64 autograd of F.conv_transpose2d."""
    B, h, w, C, O = shape
    g = _gen(91)
    pc = _lib.PRECISIONS[precision]
    x = torch.randn(B, C, h, w, generator=g)
    wt = torch.randn(C, O, 2, 2, generator=g) / C ** 0.5
    dout = torch.randn(B, O, 2 * h, 2 * w, generator=g)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    br = torch.zeros(O, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(xr, wr, br, stride=2).backward(dout.double())
    Ms = B * h * w
    dbuf, d_ptr, ld = _slice_in(_rows(dout), dev, pad_left=0, pad_right=O)  # the left half of an [up | skip] gradient
    xd = _rows(x).to(dev)
    results = []
    for _ in range(2):
        gout = _Out(Ms, 4 * O, dev, lo=0, hi=0)
        assert lib.ocm_op_upconv2x2_gather(d_ptr, ld, gout.ptr, B, h, w, O, _s()) == 0, lib.ocm_last_error()
        grows = _f32(gout.take("gather")).to(dev)
        dw, db = M._weight_grad(pc, grows, xd, True)
        w_t = to_operand(M._rows_up2x2_t(wt.to(dev)).contiguous(), pc)
        din = M._linear(lib, pc, to_operand(grows, pc), w_t, torch.zeros(C, device=dev), None, Ms, C, 4 * O)
        torch.cuda.synchronize()
        results.append((din.cpu(), dw.reshape(2, 2, O, C).permute(3, 2, 0, 1).cpu(), db.reshape(4, O).sum(0).cpu()))
    for a, b in zip(*results):
        assert_same_bits(a, b, "up-convolution backward run to run")
    din, dw, db = results[0]
    want = {"din": _rows(xr.grad), "dw": wr.grad, "db": br.grad}
    for name, gv in (("din", din), ("dw", dw), ("db", db)):
        err = float((gv.double() - want[name]).abs().max() / want[name].abs().max())
        print(f"GPUTEST upconv2x2 backward {shape} {precision} {name}: relative error {err:.3e} (bound {TOL[precision]:.0e})")
        assert err <= TOL[precision], f"{name} {precision}: {err:.3e}"
