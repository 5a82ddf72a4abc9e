"""The shared training operators at the shapes training dispatches, not only at the shapes of the feature that introduced them:
ocm_op_weight_grad with N and K that leave the last tile partly or wholly outside dW and M below one 32-row stage,
ocm_op_layernorm_backward at widths that are not a multiple of 64, row counts that are not a multiple of 4 or exceed the
saturated chunk plan, and without a residual gradient; the grid-stride elementwise kernels past one trip of their capped grid;
GELU and its backward in the tails. A census test runs one Swin-T and two MIM training steps with the Python wrappers of the two
shared operators recorded, and asserts that every dispatched shape class is in the operator lists of this file.

Every comparison is against float64 torch on the CPU, every operator runs twice (torch.equal) and every output starts as NaN.
Needs an MI355X."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.memcheck import assert_same_bits
from tests.test_mim_train_memcheck_gpu import _run
from tests.test_train_ops_gpu import TOL
from vit_ocm_wmsegmentation_amd import _lib as L
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu

# (M, N, K). Swin-T at 224^2, batch 8: stage 0 (25088 rows, C 96: q|k|v N 288, o_proj, fc1, fc2, the patch embedding with K 48
# padded to 64), the merges, the later stages, the classifier (5 labels padded to 32; 1024 = a 1000-label head); small shapes
# below one stage / one tile; 50176 rows = batch 16 (32 slices, channel chunks above 256 rows)
WGRAD_ISSUE = [(25088, 288, 96), (25088, 96, 96), (25088, 384, 96), (25088, 96, 384), (25088, 96, 64), (1568, 192, 384),
               (392, 768, 3072), (8, 1024, 768), (1, 32, 32), (31, 96, 32), (257, 160, 192), (50176, 96, 96)]
# what the census adds: the rest of Swin-T's step, and MIM at 64^2 (130 token rows, 128 patch rows) and 384^2 (4610 / 4608)
WGRAD_CENSUS = [(6272, 192, 384), (6272, 192, 768), (6272, 768, 192), (6272, 192, 192), (6272, 576, 192), (1568, 384, 768),
                (1568, 384, 1536), (1568, 1536, 384), (1568, 384, 384), (1568, 1152, 384), (392, 768, 1536), (392, 3072, 768),
                (392, 768, 768), (392, 2304, 768), (8, 32, 768),
                (130, 1152, 384), (130, 384, 384), (130, 1536, 384), (130, 384, 1536), (128, 384, 192), (128, 192, 384),
                (4610, 1152, 384), (4610, 384, 384), (4610, 1536, 384), (4610, 384, 1536), (4608, 384, 192), (4608, 192, 384)]
WGRAD_SHAPES = WGRAD_ISSUE + WGRAD_CENSUS
WGRAD_GUARDED = [(33, 96, 96), (8, 1024, 768), (257, 160, 192), (4097, 288, 96), (1, 32, 32)]

# (rows, dim)
LN_ISSUE = [(1, 96), (3, 100), (5, 192), (777, 768), (1568, 1536), (392, 3072), (32769, 96), (50176, 96)]
LN_CENSUS = [(25088, 96), (6272, 192), (6272, 384), (1568, 384), (1568, 768), (392, 768), (392, 1536), (130, 384), (4610, 384)]
LN_GUARDED = [(3, 100), (5, 192), (32769, 96)]

GRID_CAP = 8192 * 256  # threads of the capped grid of the elementwise kernels: one trip covers 2^21 elements


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _worst(got, want, den=None):
    """(max |got - want| / den, index, got there, want there); den defaults to max |want|."""
    d = (got.detach().double().cpu() - want).abs()
    i = int(d.argmax())
    den = float(want.abs().max()) if den is None else den
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), d.shape))
    return float(d.flatten()[i]) / max(den, 1e-300), idx, float(got.detach().flatten()[i]), float(want.flatten()[i])


def _assert_close(got, want, bound, what, den=None):
    e, idx, g, w = _worst(got, want, den)
    print(f"GPUTEST {what}: {e:.3e} (bound {bound:.1e})")
    assert e <= bound, f"{what}: {e:.3e} > {bound:.1e}, worst at {idx}: got {g!r}, want {w!r}"


def wgrad_class(lib, M, N, K):
    """(N, K) and what M decides: less than one 32-row stage, a partial last stage, more than one slice."""
    sliced = lib.ocm_weight_grad_workspace_bytes(M, N, K) > lib.ocm_channel_reduce_workspace_bytes(M, N)
    return (N, K, M < 32, M % 32 != 0, bool(sliced))


def ln_class(rows, dim):
    return (dim, rows % 4 != 0, rows > 32768)


# ---- A. weight gradient ------------------------------------------------------------------------------------------------
def _wgrad_inputs(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    dy[torch.rand(M, generator=g) < 0.5] *= 1e-3  # half of the rows three decades down
    x = (torch.randn(M, K, generator=g, dtype=torch.float64) + 0.5).relu()  # a per-column mean offset and exact zeros
    if K == 64:
        x[:, 48:] = 0.0  # the patch embedding: 48 columns zero-padded to the 32-column step
    return dy.float(), x.float()


def _wgrad(lib, pc, dy, x):
    M, N = dy.shape
    K = x.shape[1]
    nb = lib.ocm_weight_grad_workspace_bytes(M, N, K)
    ws = torch.full((nb // 4 + 1,), float("nan"), device="cuda")
    dw = torch.full((N, K), float("nan"), device="cuda")
    db = torch.full((N,), float("nan"), device="cuda")
    rc = lib.ocm_op_weight_grad(pc, _p(dy), _p(x), _p(dw), _p(db), M, N, K, _p(ws), nb, _s())
    assert rc == 0, lib.ocm_last_error()
    return dw, db


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("M,N,K", WGRAD_SHAPES)
def test_weight_grad_dispatched_shapes_match_float64(lib, dev, M, N, K, precision):
    dy, x = _wgrad_inputs(M, N, K)
    want, want_db = dy.double().T @ x.double(), dy.double().sum(0)
    dyd, xd = dy.cuda(), x.cuda()
    dw, db = _wgrad(lib, L.PRECISIONS[precision], dyd, xd)
    dw2, db2 = _wgrad(lib, L.PRECISIONS[precision], dyd, xd)
    torch.cuda.synchronize()
    assert_same_bits(dw, dw2, "dW run to run")
    assert_same_bits(db, db2, "db run to run")
    what = f"weight_grad {precision} {M}x{N}x{K}"
    _assert_close(dw, want, TOL[precision], what + " dW")
    _assert_close(db, want_db, 2e-5, what + " db")  # an fp32 column sum in every precision
    if K == 64:
        assert bool((dw[:, 48:] == 0).all()), f"{what}: dW of the zero-padded columns is not exactly 0.0"


@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", WGRAD_GUARDED)
def test_weight_grad_dispatched_shapes_guarded(lib, dev, M, N, K, precision):
    """No byte outside dW, db or the stated workspace size touched, every element of dW and db written, the same bits whatever
    the outputs and the workspace held."""
    pc = L.PRECISIONS[precision]
    dy, x = (t.cuda() for t in _wgrad_inputs(M, N, K))
    nb = lib.ocm_weight_grad_workspace_bytes(M, N, K)
    out = _run(lib, f"weight_grad {precision} {M}x{N}x{K}", {"dw": (N * K * 4, torch.float32), "db": (N * 4, torch.float32)}, nb,
               lambda o, ws: lib.ocm_op_weight_grad(pc, dy.data_ptr(), x.data_ptr(), o["dw"], o["db"], M, N, K, ws, nb, _s()))
    assert bool(torch.isfinite(out["dw"]).all()) and bool(torch.isfinite(out["db"]).all())
    _assert_close(out["dw"].reshape(N, K), dy.double().cpu().T @ x.double().cpu(), TOL[precision],
                  f"weight_grad guarded {precision} {M}x{N}x{K} dW")


# ---- D. LayerNorm backward -----------------------------------------------------------------------------------------------
def _ln_inputs(rows, dim, offset, seed=1):
    g = torch.Generator().manual_seed(seed + rows + dim)
    x = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    x = x + offset * torch.randn(rows, 1, generator=g, dtype=torch.float64).abs()
    w = 1 + 0.1 * torch.randn(dim, generator=g, dtype=torch.float64)
    dy = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    res = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    return [t.float() for t in (x, w, dy, res)]


def _ln_reference(x, w, dy, res, eps):
    dim = x.shape[1]
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    br = torch.zeros(dim, dtype=torch.float64, requires_grad=True)
    dx, dg, db = torch.autograd.grad(F.layer_norm(xr, (dim,), wr, br, eps), (xr, wr, br), dy.double())
    return (dx + res.double() if res is not None else dx), dg, db


def _ln_case(lib, rows, dim, offset, with_res, eps):
    x, w, dy, res = _ln_inputs(rows, dim, offset)
    if not with_res:
        res = None
    want = _ln_reference(x, w, dy, res, eps)
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    resd = res.cuda() if with_res else None
    nbytes = lib.ocm_layernorm_backward_workspace_bytes(rows, dim)
    outs = []
    for _ in range(2):
        dx = torch.full((rows, dim), float("nan"), device="cuda")
        dg, db = torch.full((dim,), float("nan"), device="cuda"), torch.full((dim,), float("nan"), device="cuda")
        ws = torch.full((nbytes // 4 + 1,), float("nan"), device="cuda")
        rc = lib.ocm_op_layernorm_backward(_p(dyd), _p(xd), _p(wd), _p(resd), _p(dx), _p(dg), _p(db), rows, dim, eps, _p(ws), nbytes,
                                           _s())
        assert rc == 0, lib.ocm_last_error()
        outs.append((dx, dg, db))
    torch.cuda.synchronize()
    what = f"layernorm_backward {rows}x{dim} offset {offset} dres {with_res} eps {eps}"
    for name, a, b, ref in zip(("dx", "dgamma", "dbeta"), outs[0], outs[1], want):
        assert_same_bits(a, b, f"{what} {name} run to run")
        _assert_close(a, ref, 1e-5, f"{what} {name}")


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("offset", [0.0, 30.0])
@pytest.mark.parametrize("rows,dim", LN_ISSUE)
def test_layernorm_backward_shapes_match_float64(lib, dev, rows, dim, offset, with_res, eps):
    _ln_case(lib, rows, dim, offset, with_res, eps)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("rows,dim", LN_CENSUS)
def test_layernorm_backward_census_shapes_match_float64(lib, dev, rows, dim, with_res):
    """The remaining (rows, dim) of a Swin-T and of the MIM steps, rows 30 sigma off zero, Swin's eps."""
    _ln_case(lib, rows, dim, 30.0, with_res, 1e-5)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("rows,dim", LN_GUARDED)
def test_layernorm_backward_shapes_guarded(lib, dev, rows, dim, with_res):
    """dgamma and dbeta are exactly `dim` floats with a guard band right behind them: with dim = 100 the channel reduction's
    second block of 64 has 28 idle threads, and none of them may store."""
    x, w, dy, res = (t.cuda() for t in _ln_inputs(rows, dim, 30.0))
    nbytes = lib.ocm_layernorm_backward_workspace_bytes(rows, dim)
    out = _run(lib, f"layernorm_backward {rows}x{dim}", {"dx": (rows * dim * 4, torch.float32), "dg": (dim * 4, torch.float32),
                                                       "db": (dim * 4, torch.float32)}, nbytes,
               lambda o, ws: lib.ocm_op_layernorm_backward(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                                                           res.data_ptr() if with_res else None, o["dx"], o["dg"], o["db"], rows,
                                                           dim, 1e-5, ws, nbytes, _s()))
    assert out["dg"].numel() == dim and out["db"].numel() == dim
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    want = _ln_reference(x.cpu(), w.cpu(), dy.cpu(), res.cpu() if with_res else None, 1e-5)
    for name, ref in zip(("dx", "dg", "db"), want):
        _assert_close(out[name].reshape(ref.shape), ref, 1e-5, f"layernorm_backward guarded {rows}x{dim} {name}")


# ---- the census ----------------------------------------------------------------------------------------------------------
def test_training_steps_dispatch_only_listed_shape_classes(lib, dev, monkeypatch):
    """One training step of Swin-T (224^2, batch 8) and of the MIM cases wrap_mim_hd128 and mim384, with model._weight_grad and
    model._ln_backward recorded (swin.py imports both by name): every (N, K, M class) and (dim, rows class) they are called with
    is the class of a shape in the operator lists above, so the literal lists cannot drift from the call sites."""
    from tests import test_mim_train_gpu as TM
    from tests import test_swin_train_gpu as TS
    from vit_ocm_wmsegmentation_amd import model as M
    from vit_ocm_wmsegmentation_amd import swin as SW

    seen_w, seen_ln = {}, {}
    real_w, real_ln = M._weight_grad, M._ln_backward

    def rec_w(prec, dy, x, want_bias):
        seen_w.setdefault(wgrad_class(lib, dy.shape[0], dy.shape[1], x.shape[1]), (dy.shape[0], dy.shape[1], x.shape[1]))
        return real_w(prec, dy, x, want_bias)

    def rec_ln(lib_, dy, x, w, dres, rows, dim, eps):
        seen_ln.setdefault(ln_class(rows, dim), (rows, dim))
        return real_ln(lib_, dy, x, w, dres, rows, dim, eps)

    for mod in (M, SW):
        monkeypatch.setattr(mod, "_weight_grad", rec_w)
        monkeypatch.setattr(mod, "_ln_backward", rec_ln)

    m, x, labels, up = TS._model("swin_t", "bf16x3", dev)
    TS._loss(m, x, labels, up).backward()
    n_swin = (len(seen_w), len(seen_ln))
    assert n_swin[0] >= 15 and n_swin[1] >= 5, n_swin  # the wrappers were reached (21 GEMM shapes, 5 LayerNorm widths)
    del m
    for name in ("wrap_mim_hd128", "mim384"):
        mim, xm, mask = TM._model(name, "bf16x3", dev)
        _, rec, _ = mim(xm, mask)
        rec.backward(TM._upstream(rec.shape).to(device=dev, dtype=torch.float32))
        del mim
    torch.cuda.synchronize()
    assert len(seen_w) > n_swin[0]
    listed_w = {wgrad_class(lib, *s) for s in WGRAD_SHAPES}
    listed_ln = {ln_class(*s) for s in LN_ISSUE + LN_CENSUS}
    print(f"GPUTEST census: {len(seen_w)} weight-gradient classes {sorted(seen_w.values())}, "
          f"{len(seen_ln)} LayerNorm classes {sorted(seen_ln.values())}")
    missing_w = {c: s for c, s in seen_w.items() if c not in listed_w}
    missing_ln = {c: s for c, s in seen_ln.items() if c not in listed_ln}
    assert not missing_w, f"dispatched weight-gradient shapes with no operator test: {sorted(missing_w.values())}"
    assert not missing_ln, f"dispatched LayerNorm shapes with no operator test: {sorted(missing_ln.values())}"


# ---- E. elementwise kernels past one grid trip, GELU tails -------------------------------------------------------------------
def _gelu_all(lib, dev, h, dg):
    """gelu in the three operand types (+ fp32) and the backward, each twice from NaN; returns (out32, dh, g32)."""
    n = h.numel()
    out32 = None
    for name, prec in L.PRECISIONS.items():
        adt = {L.OCM_PREC_BF16: torch.bfloat16, L.OCM_PREC_FP32: torch.float32, L.OCM_PREC_BF16X3: torch.int32}[prec]
        runs = []
        for _ in range(2):
            out = torch.full((n,), float("nan"), device=dev).to(adt) if adt != torch.int32 else \
                torch.full((n,), -1, dtype=torch.int32, device=dev)
            o32 = torch.full((n,), float("nan"), device=dev)
            assert lib.ocm_op_gelu(prec, _p(h), _p(out), _p(o32), n, _s()) == 0, lib.ocm_last_error()
            runs.append((out, o32))
        assert_same_bits(runs[0][1], runs[1][1], f"gelu {name} fp32 run to run")
        assert torch.equal(runs[0][0], runs[1][0]), name
        assert torch.equal(runs[0][0], to_operand(runs[0][1], prec)), f"gelu {name}: the operand is not the fp32 value converted"
        if out32 is not None:
            assert_same_bits(runs[0][1], out32, f"gelu {name} fp32 output against the first precision's")
        out32 = runs[0][1]
    runs = []
    for _ in range(2):
        dh, g32 = torch.full((n,), float("nan"), device=dev), torch.full((n,), float("nan"), device=dev)
        assert lib.ocm_op_gelu_backward(_p(dg), _p(h), _p(dh), _p(g32), n, _s()) == 0, lib.ocm_last_error()
        runs.append((dh, g32))
    torch.cuda.synchronize()
    assert_same_bits(runs[0][0], runs[1][0], "gelu_backward dh run to run")
    assert_same_bits(runs[0][1], runs[1][1], "gelu_backward g32 run to run")
    return out32, runs[0][0], runs[0][1]


def _gelu_reference(h, dg):
    hr = h.double().cpu().requires_grad_(True)
    y = F.gelu(hr)
    (dh,) = torch.autograd.grad(y, hr, dg.double().cpu())
    return y.detach(), dh


def test_gelu_past_one_grid_trip(lib, dev):
    """2^21 + 3 * 256 + 96 elements: a multiple of 32 (split pairs) but not of 256; the grid-stride loops take a second trip in
    the first 864 threads only."""
    n = GRID_CAP + 3 * 256 + 96
    assert n % 32 == 0 and n % 256
    g = torch.Generator().manual_seed(4)
    h, dg = (3 * torch.randn(n, generator=g)).to(dev), torch.randn(n, generator=g).to(dev)
    out32, dh, g32 = _gelu_all(lib, dev, h, dg)
    y, dh_ref = _gelu_reference(h, dg)
    _assert_close(out32, y, 1e-6, "gelu second trip")
    _assert_close(g32, y, 1e-6, "gelu_backward g32 second trip")
    _assert_close(dh, dh_ref, 1e-5, "gelu_backward dh second trip")
    tail = slice(GRID_CAP, n)  # the second trip on its own scale
    _assert_close(out32[tail], y[tail], 1e-6, "gelu second trip, elements past 2^21")
    _assert_close(dh[tail], dh_ref[tail], 1e-5, "gelu_backward second trip, elements past 2^21")


def test_gelu_tails(lib, dev):
    """h over [-40, 40]. Over the whole grid the bounds of test_gelu_and_backward_match_float64 (relative to the maximum) and no
    NaN / Inf; in the tails what float64 says fp32 must give: Phi(9) = 1 - 1.1e-19 and 9 phi(9) = 9e-18, so for h >= 9 gelu(h)
    and dh are h and dg to fp32 rounding (2^-22 allows the kernels' two roundings), and for h <= -9 both are below 1e-15 of
    their scale: anything larger is erf_as or the exp2 saturating or underflowing wrongly, not rounding."""
    special = torch.tensor([0.0, 1e-30, 6.0, 9.0, 13.0, 38.0, 40.0])
    grid = torch.cat([torch.linspace(-40, 40, 16001), special, -special])
    g = torch.Generator().manual_seed(6)
    grid = torch.cat([grid, grid[torch.randperm(grid.numel(), generator=g)][: 32 - grid.numel() % 32]])  # split pairs: n % 32
    assert bool((grid == 0).any()) and bool((torch.signbit(grid) & (grid == 0)).any())  # both zeros
    dg = torch.randn(grid.numel(), generator=g)
    dg = torch.where(dg.abs() < 0.1, torch.ones_like(dg), dg)
    h, dgd = grid.to(dev), dg.to(dev)
    out32, dh, g32 = _gelu_all(lib, dev, h, dgd)
    for name, t in (("gelu", out32), ("gelu_backward dh", dh), ("gelu_backward g32", g32)):
        assert bool(torch.isfinite(t).all()), f"{name}: NaN or Inf at h = {grid[~torch.isfinite(t.cpu())][:8].tolist()}"
    y, dh_ref = _gelu_reference(h, dgd)
    _assert_close(out32, y, 1e-6, "gelu [-40, 40]")
    _assert_close(g32, y, 1e-6, "gelu_backward g32 [-40, 40]")
    _assert_close(dh, dh_ref, 1e-5, "gelu_backward dh [-40, 40]")
    h64, dg64 = grid.double(), dg.double()
    hi, lo = h64 >= 9, h64 <= -9
    for name, t in (("gelu", out32), ("gelu_backward g32", g32)):
        t64 = t.double().cpu()
        e = ((t64 - h64).abs() / h64.abs().clamp_min(1))[hi]
        assert float(e.max()) <= 2.0 ** -22, f"{name}: h >= 9 off by {float(e.max()):.3e} h at h = {float(h64[hi][e.argmax()])}"
        e = t64.abs()[lo]
        assert float(e.max()) <= 1e-15, f"{name}: h <= -9 gives {float(e.max()):.3e} at h = {float(h64[lo][e.argmax()])}"
    d64 = dh.double().cpu()
    e = ((d64 - dg64).abs() / dg64.abs())[hi]
    assert float(e.max()) <= 2.0 ** -22, f"gelu_backward: h >= 9 off by {float(e.max()):.3e} dg at h = {float(h64[hi][e.argmax()])}"
    e = (d64.abs() / dg64.abs())[lo]
    assert float(e.max()) <= 1e-15, f"gelu_backward: h <= -9 gives {float(e.max()):.3e} dg at h = {float(h64[lo][e.argmax()])}"


def test_patch_embed_backward_past_one_grid_trip(lib, dev):
    """3 x 1001 x 699 = 2 099 097 elements (odd). dpatch is one product per element; the mask token's gradient is an fp32 column sum
    over 3003 rows (the bias-gradient bound of the weight-gradient tests, 2e-5), the position gradient a sum of three terms."""
    B, N, D = 3, 1002, 699
    total = B * (N - 1) * D
    assert total > GRID_CAP + 3 * 256 and total % 256
    g = torch.Generator().manual_seed(8)
    dt64 = torch.randn(B, N, D, generator=g, dtype=torch.float64)
    w64 = (torch.rand(B, N - 1, generator=g) < 0.6).double()
    dt, w = dt64.float().to(dev), w64.float().to(dev)
    dt64 = dt.double().cpu()
    nbytes = lib.ocm_patch_embed_backward_workspace_bytes(B, N, D)
    res = []
    for _ in range(2):
        dpatch, dmask, dpos = (torch.full(s, float("nan"), device=dev) for s in ((B * (N - 1), D), (D,), (N, D)))
        ws = torch.full((nbytes // 4 + 1,), float("nan"), device=dev)
        rc = lib.ocm_op_patch_embed_backward(_p(dt), _p(w), _p(dpatch), _p(dmask), _p(dpos), B, N, D, _p(ws), nbytes, _s())
        assert rc == 0, lib.ocm_last_error()
        res.append((dpatch, dmask, dpos))
    torch.cuda.synchronize()
    for name, a, b in zip(("dpatch", "dmask", "dpos"), *res):
        assert_same_bits(a, b, f"patch_embed_backward {name} run to run")
    wv = w64.unsqueeze(-1)
    dpatch, dmask, dpos = res[0]
    assert torch.equal(dpatch.cpu().double(), ((1 - wv) * dt64[:, 1:]).reshape(-1, D))  # w is 0 or 1: the product is exact
    _assert_close(dmask, (wv * dt64[:, 1:]).sum((0, 1)), 2e-5, "patch_embed_backward dmask second trip")
    _assert_close(dpos, dt64.sum(0), 1e-6, "patch_embed_backward dpos second trip")


def test_patch_unfold_and_pixel_shuffle_backward_past_one_grid_trip(lib, dev):
    """3 x 837 x 837 = 2 101 707 elements (odd), patches / shuffle blocks of 9: permutations, bit exact."""
    Cc, S, p = 3, 837, 9
    hp = S // p
    total = Cc * S * S
    assert total > GRID_CAP + 3 * 256 and total % 256
    img = torch.randn(1, Cc, S, S, generator=torch.Generator().manual_seed(9))
    imgd = img.to(dev)
    res = []
    for _ in range(2):
        cols = torch.full((hp * hp, Cc * p * p), float("nan"), device=dev)
        lin = torch.full((hp * hp, Cc * p * p), float("nan"), device=dev)
        assert lib.ocm_op_patch_unfold(_p(imgd), _p(cols), 1, Cc, S, S, p, _s()) == 0, lib.ocm_last_error()
        assert lib.ocm_op_pixel_shuffle_backward(_p(imgd), _p(lin), 1, hp, hp, Cc, p, _s()) == 0, lib.ocm_last_error()
        res.append((cols, lin))
    torch.cuda.synchronize()
    assert_same_bits(res[0][0], res[1][0], "patch_unfold run to run")
    assert_same_bits(res[0][1], res[1][1], "pixel_shuffle_backward run to run")
    assert_same_bits(res[0][0].cpu(), F.unfold(img, p, stride=p).transpose(1, 2).reshape(-1, Cc * p * p), "patch_unfold")
    assert_same_bits(res[0][1].cpu(), F.pixel_unshuffle(img, p).permute(0, 2, 3, 1).reshape(hp * hp, -1), "pixel_unshuffle")
