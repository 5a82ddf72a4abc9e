"""Memory behaviour of kernels_optim.hip through the C ABI with tests.memcheck.Guarded: param, m and v of sizes 1, 5 and C + 1 each
in a guard-banded buffer (the guards stay intact after a step), and the gradient norm's workspace sized exactly by
ocm_grad_norm_workspace_bytes and pre-filled with nan / ones / zero (identical results, guards intact). Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import optim_cases as OC
from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu


def _sizes():
    return [1, 5, OC.limits()[1] + 1]


def _table(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.int64))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("rule", ["adamw", "adam", "sgd"])
def test_step_stays_inside_its_tensors(lib, dev, rule):
    gen = torch.Generator().manual_seed(11)
    bufs, rows, host = [], [], []
    for n in _sizes():
        vals = [torch.randn(n, generator=gen) for _ in range(2)] + [torch.rand(n, generator=gen)]  # p, m, v
        g = torch.randn(n, generator=gen).to(dev)
        guarded = [Guarded(4 * n, dev, pattern="nan") for _ in range(3)]
        for gd, val in zip(guarded, vals):
            gd.payload(torch.float32).copy_(val)
        bufs.append((guarded, g))
        host.append((vals, g.cpu()))
        rows.append([guarded[0].ptr, g.data_ptr(), guarded[1].ptr, guarded[2].ptr, n])
    table = _table(rows)
    hyper = _lib.OcmOptimHyper(rule={"adamw": 0, "adam": 1, "sgd": 2}[rule], nesterov=1, first_step=0, lr=1e-2, beta1=0.9, beta2=0.999,
                               eps=1e-8, weight_decay=0.05, step_size=1e-2 / (1 - 0.9 ** 3),
                               bias_correction2_sqrt=(1 - 0.999 ** 3) ** 0.5, momentum=0.9, dampening=0.0)
    _lib.check(lib.ocm_op_optim_step(table.ctypes.data, len(rows), C.byref(hyper), _stream()))
    torch.cuda.synchronize()
    for (guarded, _), (vals, g) in zip(bufs, host):
        for gd, name in zip(guarded, ("param", "m", "v")):
            assert gd.check() is None, (rule, name, gd.nbytes, gd.check())
        p, m, v = (gd.payload(torch.float32).cpu() for gd in guarded)
        assert torch.isfinite(p).all() and not torch.equal(p, vals[0])
        assert not torch.equal(m, vals[1])
        if rule == "sgd":
            assert_same_bits(v, vals[2], "v is not touched by SGD")
        else:
            assert torch.isfinite(v).all() and not torch.equal(v, vals[2])


def test_norm_workspace_needs_no_initialisation(lib, dev):
    gen = torch.Generator().manual_seed(12)
    grads = [torch.randn(n, generator=gen).to(dev) for n in _sizes() + [0, 3 * OC.limits()[1]]]
    table = _table([[0, g.data_ptr(), 0, 0, g.numel()] for g in grads])
    nbytes = lib.ocm_grad_norm_workspace_bytes(table.ctypes.data, len(grads))
    chunk = OC.limits()[1]
    assert nbytes == 8 * sum(-(-g.numel() // chunk) for g in grads)
    results = []
    for pattern in ("nan", "ones", "zero"):
        ws = Guarded(nbytes, dev, pattern=pattern)
        out = Guarded(16, dev, pattern=pattern)
        scaled = [Guarded(4 * g.numel(), dev, pattern=pattern) for g in grads]
        for s, g in zip(scaled, grads):
            s.payload(torch.float32).copy_(g)
        tab2 = _table([[0, s.ptr, 0, 0, g.numel()] for s, g in zip(scaled, grads)])
        _lib.check(lib.ocm_op_grad_norm(tab2.ctypes.data, len(grads), 1.0, out.ptr, out.ptr + 8, out.ptr + 12, ws.ptr, nbytes,
                                        _stream()))
        _lib.check(lib.ocm_op_grad_scale(tab2.ctypes.data, len(grads), out.ptr + 12, _stream()))
        torch.cuda.synchronize()
        assert ws.check() is None and out.check() is None, (pattern, ws.check(), out.check())
        for s in scaled:
            assert s.check() is None, (pattern, s.nbytes, s.check())
        results.append((out.payload(torch.float32).cpu().clone(), [s.payload(torch.float32).cpu().clone() for s in scaled]))
    want = float(torch.cat([g.double().cpu() for g in grads]).square().sum().sqrt())
    assert abs(float(results[0][0][2]) - want) <= 1.2e-7 * want
    assert float(results[0][0][3]) < 1.0
    for out, scaled in results[1:]:
        assert_same_bits(out, results[0][0], "sum of squares, norm and coefficient across workspace patterns")
        for a, b in zip(scaled, results[0][1]):
            assert_same_bits(a, b, "scaled gradients across workspace patterns")
