"""The DINO row operators (kernels_dino.hip, ocm_op_ema_update) against float64 on an MI355X: l2_normalize, weight_norm and the
DINO loss forward and backward, the centre, the EMA, and every operator twice for equal bits.

Error measure: max |a - a64| / max |a64| per tensor. The bound of the three fp32 row kernels is not a fixed number: on the same
cases the test evaluates the same formulas with torch's own fp32 operators on the device (tests/dino_ref.py, autograd for the
gradients), takes the worst error of that evaluation against float64 per output kind, and allows 4 x it, because the kernels'
fixed summation order differs from ATen's. Measured on an MI355X (worst over the cases below; -s prints the table per case):

  output kind          torch fp32   these kernels   bound (4 x torch fp32)
  l2 y                 8.7e-08      6.9e-08         3.5e-07
  l2 dx                9.7e-08      9.1e-08         3.9e-07
  weight_norm w        9.2e-08      7.1e-08         3.7e-07
  weight_norm dg       1.1e-07      6.7e-08         4.3e-07
  weight_norm dv       1.4e-07      9.4e-08         5.8e-07
  loss                 1.8e-07      1.9e-07         7.3e-07
  loss dS              1.0e-06      1.2e-06         4.0e-06
  centre               7.6e-08      7.6e-08         3.0e-07

The worst loss gradients are the K = 65536 case at teacher_temp 0.04 (kernel 1.2e-6, torch 3.8e-7) and the misaligned K = 1003
case (1.0e-6 both): z = (T - c) / 0.04 reaches 100, where one fp32 rounding of z moves exp(z) by up to 4e-6 relative in either
evaluation. The overflow guard (student logits x 50, teacher logits and centre near 1e3) is 2e-7 for both: its softmaxes are
nearly one-hot. With K = 1 the loss is 0 in float64 and the measure is absolute (kernel 1.5e-7, torch 0). The batch sum of the
centre and the EMA are compared bit for bit with torch's fp32 statements."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import dino_ref as R
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.dino import utils as DU
from vit_ocm_wmsegmentation_amd.optimizer import optim_limits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L2_CASES = {"1x1": (1, 1, None), "5x32": (5, 32, None), "7x256": (7, 256, None), "3x1000": (3, 1000, None),
            "5x32_zero_row": (5, 32, 2)}
WN_CASES = {"32x64": (32, 64), "96x256": (96, 256), "33x40": (33, 40)}
# name -> (B, V, K, misaligned, guard)
LOSS_CASES = {"1_2_1": (1, 2, 1, False, False), "1_2_32": (1, 2, 32, False, False), "3_4_2080": (3, 4, 2080, False, False),
              "2_10_4096": (2, 10, 4096, False, False), "2_3_65536": (2, 3, 65536, False, False),
              "2_3_1003_misaligned": (2, 3, 1003, True, False), "2_4_2080_guard": (2, 4, 2080, False, True)}
TEMPS = (0.04, 0.07)
STUDENT_TEMP = 0.1
GRAD_LOSS = 1.7


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _offset_copy(t):
    """A copy of t on the device that starts one float past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


# ---- the operators, on device tensors ----
def l2_forward(x):
    lib = _lib.load()
    y, norm = torch.empty_like(x), torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _lib.check(lib.ocm_op_l2_normalize(_p(x), _p(y), _p(norm), x.shape[0], x.shape[1], _stream()))
    return y, norm


def l2_backward(dy, y, norm):
    dx = torch.empty_like(dy)
    _lib.check(_lib.load().ocm_op_l2_normalize_backward(_p(dy), _p(y), _p(norm), _p(dx), dy.shape[0], dy.shape[1], _stream()))
    return dx


def wn_forward(v, g):
    w, norm = torch.empty_like(v), torch.empty(v.shape[0], dtype=torch.float32, device=v.device)
    _lib.check(_lib.load().ocm_op_weight_norm(_p(v), _p(g), _p(w), _p(norm), v.shape[0], v.shape[1], _stream()))
    return w, norm


def wn_backward(dw, v, g, norm, want_dg=True, want_dv=True):
    dg = torch.empty(v.shape[0], dtype=torch.float32, device=v.device) if want_dg else None
    dv = torch.empty_like(v) if want_dv else None
    _lib.check(_lib.load().ocm_op_weight_norm_backward(_p(dw), _p(v), _p(g), _p(norm), _p(dg), _p(dv), v.shape[0], v.shape[1],
                                                       _stream()))
    return dg, dv


def loss_forward(s, t, c, tt, B, V):
    lib, K = _lib.load(), s.shape[1]
    loss = torch.empty((), dtype=torch.float32, device=s.device)
    stats = torch.empty(((V + 2) * B, 2), dtype=torch.float64, device=s.device)
    nbytes = lib.ocm_dino_loss_workspace_bytes(B, V, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=s.device)
    _lib.check(lib.ocm_op_dino_loss(_p(s), _p(t), _p(c), STUDENT_TEMP, tt, B, V, K, _p(loss), _p(stats), _p(ws), nbytes, _stream()))
    return loss, stats


def loss_backward(g, s, t, c, tt, B, V, stats, out=None):
    ds = torch.empty_like(s) if out is None else out
    _lib.check(_lib.load().ocm_op_dino_loss_backward(_p(g), _p(s), _p(t), _p(c), STUDENT_TEMP, tt, B, V, s.shape[1], _p(stats),
                                                     _p(ds), _stream()))
    return ds


def center_sum(t):
    out = torch.empty(t.shape[1], dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().ocm_op_dino_center(_lib.OCM_DINO_CENTER_SUM, _p(t), t.shape[0], t.shape[1], _p(out), None, 0.0, 0.0,
                                              _stream()))
    return out


def center_update(center, batch_sum, count, momentum):
    _lib.check(_lib.load().ocm_op_dino_center(_lib.OCM_DINO_CENTER_UPDATE, None, 0, center.numel(), _p(batch_sum), _p(center),
                                              float(count), momentum, _stream()))
    return center


# ---- inputs and the three evaluations (float64 on the CPU, torch fp32 on the device, the kernels) per case ----
def _l2_inputs(name):
    rows, dim, zero = L2_CASES[name]
    x, dy = _randn((rows, dim), 1), _randn((rows, dim), 2)
    if zero is not None:
        x[zero] = 0
    return x, dy


def _l2_torch(x, dy):
    x = x.clone().requires_grad_(True)
    y, _ = R.l2_normalize(x)
    y.backward(dy)
    return y.detach(), x.grad


@functools.lru_cache(maxsize=None)
def _l2_measured(name):
    x, dy = _l2_inputs(name)
    y64, dx64 = _l2_torch(x.double(), dy.double())
    y32, dx32 = _l2_torch(x.to(DEV), dy.to(DEV))
    y, norm = l2_forward(x.to(DEV))
    dx = l2_backward(dy.to(DEV), y, norm)
    return {"l2 y": (R.rel(y32, y64), R.rel(y, y64)), "l2 dx": (R.rel(dx32, dx64), R.rel(dx, dx64))}, (y, norm, dx, y64)


def _wn_inputs(name):
    N, K = WN_CASES[name]
    return _randn((N, K), 3, 0.05), 1.0 + _randn((N,), 4, 0.2), _randn((N, K), 5)


def _wn_torch(v, g, dw):
    v, g = v.clone().requires_grad_(True), g.clone().requires_grad_(True)
    w, _ = R.weight_norm(v, g)
    w.backward(dw)
    return w.detach(), g.grad, v.grad


@functools.lru_cache(maxsize=None)
def _wn_measured(name):
    v, g, dw = _wn_inputs(name)
    w64, dg64, dv64 = _wn_torch(v.double(), g.double(), dw.double())
    w32, dg32, dv32 = _wn_torch(v.to(DEV), g.to(DEV), dw.to(DEV))
    w, norm = wn_forward(v.to(DEV), g.to(DEV))
    dg, dv = wn_backward(dw.to(DEV), v.to(DEV), g.to(DEV), norm)
    return {"weight_norm w": (R.rel(w32, w64), R.rel(w, w64)), "weight_norm dg": (R.rel(dg32, dg64), R.rel(dg, dg64)),
            "weight_norm dv": (R.rel(dv32, dv64), R.rel(dv, dv64))}, (w, norm, dg, dv)


def _loss_inputs(name):
    B, V, K, misaligned, guard = LOSS_CASES[name]
    s, t, c = _randn((V * B, K), 6), _randn((2 * B, K), 7), _randn((K,), 8, 0.3)
    if guard:  # a softmax that does not subtract its row maximum overflows: exp(50 * 3 / 0.1), exp(1e3 / 0.04)
        s, t, c = s * 50, t + 1e3, c + 1e3
    return s, t, c


def _loss_torch(s, t, c, tt, V):
    s = s.clone().requires_grad_(True)
    loss = R.dino_loss(s, t, c, STUDENT_TEMP, tt, V)
    (loss * GRAD_LOSS).backward()
    return loss.detach(), s.grad


def _on_device(name, *tensors):
    put = _offset_copy if LOSS_CASES[name][3] else (lambda t: t.to(DEV))
    return [put(t) for t in tensors]


@functools.lru_cache(maxsize=None)
def _loss_measured(name, tt):
    B, V, K, _, _ = LOSS_CASES[name]
    s, t, c = _loss_inputs(name)
    l64, ds64 = _loss_torch(s.double(), t.double(), c.double(), tt, V)
    l32, ds32 = _loss_torch(s.to(DEV), t.to(DEV), c.to(DEV), tt, V)
    sd, td, cd = _on_device(name, s, t, c)
    loss, stats = loss_forward(sd, td, cd, tt, B, V)
    g = torch.tensor([GRAD_LOSS], dtype=torch.float32, device=DEV)
    ds = loss_backward(g, sd, td, cd, tt, B, V, stats, out=_on_device(name, torch.zeros_like(s))[0])
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(ds).all())
    return {"loss": (R.rel(l32, l64), R.rel(loss, l64)), "loss dS": (R.rel(ds32, ds64), R.rel(ds, ds64))}, (loss, ds)


def _center_measured(rows, K):
    t, c = _randn((rows, K), 9), _randn((K,), 10, 0.3)
    want64 = R.center_update(c.double(), t.double().sum(0), rows, 0.9)
    torch32 = R.center_update(c.to(DEV), t.to(DEV).sum(0), rows, 0.9)
    ours = center_update(c.to(DEV), center_sum(t.to(DEV)), rows, 0.9)
    return {"centre": (R.rel(torch32, want64), R.rel(ours, want64))}


CENTER_CASES = [(4, 1), (6, 37), (4, 4099), (128, 1000)]


@functools.lru_cache(maxsize=None)
def _bounds():
    """{output kind: 4 x the worst torch-fp32 error over the cases}, with the table it comes from."""
    rows = []
    for name in L2_CASES:
        rows += [(name, k, v) for k, v in _l2_measured(name)[0].items()]
    for name in WN_CASES:
        rows += [(name, k, v) for k, v in _wn_measured(name)[0].items()]
    for name in LOSS_CASES:
        for tt in TEMPS:
            rows += [(f"{name} tt={tt}", k, v) for k, v in _loss_measured(name, tt)[0].items()]
    for case in CENTER_CASES:
        rows += [(f"centre {case}", k, v) for k, v in _center_measured(*case).items()]
    worst = {}
    for case, kind, (e32, ours) in rows:
        print(f"{case:28s} {kind:16s} torch fp32 {e32:.3e}   kernel {ours:.3e}")
        w = worst.setdefault(kind, [0.0, 0.0])
        w[0], w[1] = max(w[0], e32), max(w[1], ours)
    for kind, (e32, ours) in worst.items():
        print(f"worst {kind:16s} torch fp32 {e32:.3e}   kernel {ours:.3e}   bound {4 * e32:.3e}")
    return {kind: 4 * e32 for kind, (e32, _) in worst.items()}


def _assert_within(measured):
    bounds = _bounds()
    for kind, (e32, ours) in measured.items():
        assert bounds[kind] > 0
        assert ours <= bounds[kind], f"{kind}: {ours:.3e} > 4 x torch fp32's worst {bounds[kind] / 4:.3e} (this case: {e32:.3e})"


@pytest.mark.parametrize("name", list(L2_CASES))
def test_l2_normalize(dev, name):
    measured, (y, norm, dx, y64) = _l2_measured(name)
    _assert_within(measured)
    x, dy = _l2_inputs(name)
    want_norm = x.double().norm(dim=1).clamp_min(1e-12)
    assert R.rel(norm, want_norm) <= 2e-7  # one fp32 rounding of a float64 sum
    zero = L2_CASES[name][2]
    if zero is not None:  # the clamp: y = 0 / 1e-12, dx = dy / 1e-12, as torch's graph gives
        assert float(norm[zero]) == np.float32(1e-12) and float(y[zero].abs().max()) == 0.0
        assert_same_bits(dx[zero].cpu(), dy[zero] / np.float32(1e-12), "dx of the clamped row")
    y2, norm2 = l2_forward(x.to(DEV))
    assert_same_bits(y, y2, "l2 y twice")
    assert_same_bits(norm, norm2, "l2 norm twice")
    assert_same_bits(dx, l2_backward(dy.to(DEV), y, norm), "l2 dx twice")
    inplace = dy.to(DEV)
    _lib.check(_lib.load().ocm_op_l2_normalize_backward(_p(inplace), _p(y), _p(norm), _p(inplace), *x.shape, _stream()))
    assert_same_bits(dx, inplace, "l2 dx written over dy")


@pytest.mark.parametrize("name", list(WN_CASES))
def test_weight_norm(dev, name):
    measured, (w, norm, dg, dv) = _wn_measured(name)
    _assert_within(measured)
    v, g, dw = (t.to(DEV) for t in _wn_inputs(name))
    assert R.rel(norm, v.double().norm(dim=1)) <= 2e-7
    w2, norm2 = wn_forward(v, g)
    assert_same_bits(w, w2, "weight_norm w twice")
    assert_same_bits(norm, norm2, "weight_norm norms twice")
    dg2, dv2 = wn_backward(dw, v, g, norm)
    assert_same_bits(dg, dg2, "dg twice")
    assert_same_bits(dv, dv2, "dv twice")
    only_dg, none = wn_backward(dw, v, g, norm, want_dv=False)
    assert none is None
    assert_same_bits(dg, only_dg, "dg with dv NULL")
    none, only_dv = wn_backward(dw, v, g, norm, want_dg=False)
    assert none is None
    assert_same_bits(dv, only_dv, "dv with dg NULL")


@pytest.mark.parametrize("tt", TEMPS)
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_dino_loss(dev, name, tt):
    measured, (loss, ds) = _loss_measured(name, tt)
    _assert_within(measured)
    B, V, K, _, _ = LOSS_CASES[name]
    sd, td, cd = _on_device(name, *_loss_inputs(name))
    loss2, stats = loss_forward(sd, td, cd, tt, B, V)
    assert_same_bits(loss.reshape(1), loss2.reshape(1), "loss twice")
    g = torch.tensor([GRAD_LOSS], dtype=torch.float32, device=DEV)
    assert_same_bits(ds, loss_backward(g, sd, td, cd, tt, B, V, stats), "dS twice (and wherever it lies)")
    # the gradient is linear in grad_loss
    ds1 = loss_backward(torch.ones(1, device=DEV), sd, td, cd, tt, B, V, stats)
    assert R.rel(ds, ds1.double() * GRAD_LOSS) <= 3e-7


def test_dino_loss_module_matches_the_operator(dev):
    """DINOLoss.forward: the schedule's temperature, crop-major rows, the backward's grad_loss from the graph, the centre moved."""
    B, V, K = 3, 4, 2080
    s, t, c = _loss_inputs("3_4_2080")
    mod = DU.DINOLoss(K, V, 0.04, 0.07, 3, 5).to(DEV)
    mod.center.copy_(c.reshape(1, K))
    version = mod.center._version
    sd = s.to(DEV).requires_grad_(True)
    loss = mod(sd, t.to(DEV), 1)  # epoch 1: (0.04 + 0.07) / 2
    assert loss.dim() == 0 and mod.center._version > version
    (loss * GRAD_LOSS).backward()
    tt = float(np.linspace(0.04, 0.07, 3)[1])
    want, stats = loss_forward(s.to(DEV), t.to(DEV), c.to(DEV), tt, B, V)
    assert_same_bits(loss.detach().reshape(1), want.reshape(1), "module loss")
    g = torch.tensor([GRAD_LOSS], dtype=torch.float32, device=DEV)
    assert_same_bits(sd.grad, loss_backward(g, s.to(DEV), t.to(DEV), c.to(DEV), tt, B, V, stats), "module dS")
    moved = center_update(c.to(DEV), center_sum(t.to(DEV)), 2 * B, 0.9)
    assert_same_bits(mod.center.reshape(-1), moved, "module centre")
    with pytest.raises(ValueError, match="crops"):
        mod(s.to(DEV)[:-1], t.to(DEV), 0)


@pytest.mark.parametrize("rows,K", CENTER_CASES)
def test_center(dev, rows, K):
    _assert_within(_center_measured(rows, K))
    t, c = _randn((rows, K), 9), _randn((K,), 10, 0.3)
    for view in (lambda x: x.to(DEV), _offset_copy):
        td = view(t)
        s = center_sum(td)
        assert_same_bits(s.cpu(), R.sequential_sum(t), "batch sum, rows added in rising order")
        assert_same_bits(s, center_sum(td), "batch sum twice")
        for count in (rows, 3 * rows):  # one rank; three ranks' rows in the divisor
            got = center_update(view(c), s, count, 0.9)
            want = R.center_update(c, s.cpu(), count, 0.9)  # torch's three fp32 statements
            assert_same_bits(got.cpu(), want, f"centre update, count {count}")


def _ema_tables():
    T, chunk = optim_limits()
    counts = [0, 1, 5, chunk // 2 + 3, 4096 + 3]
    return {"one": [4096 + 3], "three": [5, 0, 4096 + 3], "many": [counts[i % len(counts)] for i in range(T + 8)],
            "chunks": [3 * chunk + 5, 1]}


@pytest.mark.parametrize("table", ["one", "three", "many", "chunks"])
@pytest.mark.parametrize("momentum", [0.996, 0.9])
def test_ema_update(dev, table, momentum):
    counts = _ema_tables()[table]
    teacher, student, twin = [], [], []
    for i, n in enumerate(counts):
        p, q = _randn((n,), 20 + i), _randn((n,), 60 + i)
        put = _offset_copy if (i % 3 == 1 and n) else (lambda t: t.to(DEV))  # every third tensor starts off a 16-byte boundary
        teacher.append(put(p))
        student.append(put(q) if i % 2 else q.to(DEV))
        twin.append(p.to(DEV))
    versions = [t._version for t in teacher]
    DU.ema_update(teacher, student, momentum)
    assert all(t._version > v for t, v in zip(teacher, versions))
    for p, q in zip(twin, student):
        p.mul_(momentum).add_((1 - momentum) * q)  # torch's own statements on the device
    for i, (a, b) in enumerate(zip(teacher, twin)):
        assert_same_bits(a, b, f"tensor {i} of {len(counts)} ({counts[i]} elements)")
    again = [p.to(DEV) for p in (_randn((n,), 20 + i) for i, n in enumerate(counts))]
    DU.ema_update(again, student, momentum)
    for i, (a, b) in enumerate(zip(again, twin)):
        assert_same_bits(a, b, f"tensor {i} wherever it lies")


def test_clip_gradients_matches_the_reference_rule(dev):
    lin = torch.nn.Sequential(torch.nn.Linear(37, 5), torch.nn.Linear(5, 3)).to(DEV)
    grads = [_randn(p.shape, 80 + i, s) for i, (p, s) in enumerate(zip(lin.parameters(), (1.0, 0.01, 3.0, 1e-4)))]
    for p, g in zip(lin.parameters(), grads):
        p.grad = g.to(DEV)
    norms = DU.clip_gradients(lin, 0.5)
    for p, g, n in zip(lin.parameters(), grads, norms):
        want_norm = float(g.double().norm())
        assert abs(n - want_norm) <= 1e-6 * want_norm
        coef = 0.5 / (want_norm + 1e-6)
        want = g.double() * coef if coef < 1 else g.double()
        assert R.rel(p.grad, want) <= 1e-6
        if coef >= 1:
            assert_same_bits(p.grad.cpu(), g, "an unclipped gradient keeps its bits")
