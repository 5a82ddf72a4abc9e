"""Memory behaviour of kernels_dino.hip and ocm_op_ema_update through the C ABI with tests.memcheck.Guarded, at the odd-sized cases
of tests/test_dino_ops_gpu.py: every output in a guard-banded buffer sized exactly (the guards stay intact, every payload element
is written: none keeps the NaN it held), the loss's workspace sized exactly by ocm_dino_loss_workspace_bytes and pre-filled with
nan / ones / big (identical results). Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.optimizer import optim_limits

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _guarded_input(t, dev):
    """t in a guard-banded buffer of exactly its size: a read past either end takes NaN in."""
    g = Guarded(4 * t.numel(), dev, pattern="nan")
    g.payload(torch.float32).copy_(t.reshape(-1))
    return g


def _out(n, dev, pattern="nan", esz=4):
    return Guarded(esz * n, dev, pattern=pattern)


def _written(g, what, dtype=torch.float32):
    assert g.check() is None, (what, g.check())
    v = g.payload(dtype).clone()
    assert bool(torch.isfinite(v).all()), f"{what}: an element was not written, or a read left its row"
    return v


@pytest.mark.parametrize("rows,dim", [(1, 1), (5, 33), (3, 1000), (2, 1027)])
def test_l2_normalize(lib, dev, rows, dim):
    x, dy = _guarded_input(_randn((rows, dim), 1), dev), _guarded_input(_randn((rows, dim), 2), dev)
    y, norm, dx = _out(rows * dim, dev), _out(rows, dev), _out(rows * dim, dev)
    _lib.check(lib.ocm_op_l2_normalize(x.ptr, y.ptr, norm.ptr, rows, dim, _stream()))
    _lib.check(lib.ocm_op_l2_normalize_backward(dy.ptr, y.ptr, norm.ptr, dx.ptr, rows, dim, _stream()))
    torch.cuda.synchronize()
    yv = _written(y, "y").reshape(rows, dim)
    _written(norm, "norm")
    _written(dx, "dx")
    assert float((yv.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    assert x.check() is None and dy.check() is None


@pytest.mark.parametrize("N,K", [(1, 1), (33, 40), (7, 1027)])
def test_weight_norm(lib, dev, N, K):
    v, g, dw = (_guarded_input(t, dev) for t in (_randn((N, K), 3, 0.05), 1.0 + _randn((N,), 4, 0.2), _randn((N, K), 5)))
    w, norm, dg, dv = _out(N * K, dev), _out(N, dev), _out(N, dev), _out(N * K, dev)
    _lib.check(lib.ocm_op_weight_norm(v.ptr, g.ptr, w.ptr, norm.ptr, N, K, _stream()))
    _lib.check(lib.ocm_op_weight_norm_backward(dw.ptr, v.ptr, g.ptr, norm.ptr, dg.ptr, dv.ptr, N, K, _stream()))
    torch.cuda.synchronize()
    for buf, what in ((w, "w"), (norm, "norm"), (dg, "dg"), (dv, "dv")):
        _written(buf, what)
    only = _out(N, dev)
    _lib.check(lib.ocm_op_weight_norm_backward(dw.ptr, v.ptr, g.ptr, norm.ptr, only.ptr, None, N, K, _stream()))
    torch.cuda.synchronize()
    assert_same_bits(_written(only, "dg alone"), dg.payload(torch.float32), "dg with dv NULL")


@pytest.mark.parametrize("B,V,K", [(1, 2, 1), (3, 4, 2081), (2, 3, 4099), (1, 5, 8195)])
def test_dino_loss(lib, dev, B, V, K):
    s, t, c = (_guarded_input(x, dev) for x in (_randn((V * B, K), 6), _randn((2 * B, K), 7), _randn((K,), 8, 0.3)))
    nbytes = lib.ocm_dino_loss_workspace_bytes(B, V, K)
    assert nbytes == B * -(-K // 4096) * 2 * V * 8
    grad = torch.tensor([1.7], dtype=torch.float32, device=dev)
    results = []
    for pattern in ("nan", "ones", "big"):
        ws = Guarded(nbytes, dev, pattern=pattern)
        loss, stats, ds = _out(1, dev, pattern), _out((V + 2) * B * 2, dev, pattern, esz=8), _out(V * B * K, dev, pattern)
        _lib.check(lib.ocm_op_dino_loss(s.ptr, t.ptr, c.ptr, 0.1, 0.04, B, V, K, loss.ptr, stats.ptr, ws.ptr, nbytes, _stream()))
        _lib.check(lib.ocm_op_dino_loss_backward(grad.data_ptr(), s.ptr, t.ptr, c.ptr, 0.1, 0.04, B, V, K, stats.ptr, ds.ptr,
                                                 _stream()))
        torch.cuda.synchronize()
        assert ws.check() is None, (pattern, ws.check())
        results.append((_written(loss, "loss"), _written(stats, "row statistics", torch.float64), _written(ds, "dS")))
        assert float(results[-1][2].abs().max()) < 1e3  # ("big" would show as 3.4e38)
    for other in results[1:]:
        for a, b, what in zip(other, results[0], ("loss", "row statistics", "dS")):
            assert_same_bits(a, b, f"{what} across workspace and output patterns")
    assert s.check() is None and t.check() is None and c.check() is None


@pytest.mark.parametrize("rows,K", [(1, 1), (6, 37), (3, 4099)])
def test_center(lib, dev, rows, K):
    t, c = _guarded_input(_randn((rows, K), 9), dev), _guarded_input(_randn((K,), 10, 0.3), dev)
    s = _out(K, dev)
    _lib.check(lib.ocm_op_dino_center(_lib.OCM_DINO_CENTER_SUM, t.ptr, rows, K, s.ptr, None, 0.0, 0.0, _stream()))
    _lib.check(lib.ocm_op_dino_center(_lib.OCM_DINO_CENTER_UPDATE, None, 0, K, s.ptr, c.ptr, float(rows), 0.9, _stream()))
    torch.cuda.synchronize()
    _written(s, "batch sum")
    _written(c, "centre")
    assert t.check() is None


def test_ema_stays_inside_its_tensors(lib, dev):
    chunk = optim_limits()[1]
    sizes = [1, 5, chunk + 1, 0, 4096 + 3]
    teacher = [_guarded_input(_randn((n,), 20 + i), dev) for i, n in enumerate(sizes)]
    student = [_guarded_input(_randn((n,), 40 + i), dev) for i, n in enumerate(sizes)]
    before = [g.payload(torch.float32).clone() for g in teacher]
    table = np.ascontiguousarray(np.array([[t.ptr, s.ptr, 0, 0, n] for t, s, n in zip(teacher, student, sizes)], dtype=np.int64))
    _lib.check(lib.ocm_op_ema_update(table.ctypes.data, len(sizes), 0.9, _stream()))
    torch.cuda.synchronize()
    for t, s, b, n in zip(teacher, student, before, sizes):
        v = _written(t, f"teacher tensor of {n}")
        assert s.check() is None
        assert n == 0 or not torch.equal(v, b)
