"""Memory behaviour of the k-means kernels (kernels_cluster.hip) with the tests/memcheck.py helpers: every output in its
own guard-banded buffer, every workspace an exactly sized guarded payload filled with a poison pattern. Each case asserts
OCM_OK, intact guards, outputs fully written (the same bits from `nan`- and `zero`-filled outputs) and outputs that do
not depend on the workspace's previous contents. Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.memcheck import Guarded, PATTERNS, assert_same_bits

pytestmark = pytest.mark.gpu

POISON = list(PATTERNS)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _g(t_bytes, dev, pattern):
    return Guarded(t_bytes, dev, pattern)


def _run(dev, lib, S, D, ws_pattern, out_pattern, inputs):
    """zscore -> dist (with and without closest) -> lloyd (full and assign-only), every buffer guarded."""
    n = S * S
    x, cand, cen, lab_old = inputs
    X = _g(n * D * 4, dev, out_pattern)
    X.payload(torch.float32, (n, D)).copy_(x)
    stats = _g(4 * D * 8, dev, out_pattern)
    zws = _g(lib.ocm_kmeans_zscore_workspace_bytes(S, D), dev, ws_pattern)
    assert lib.ocm_op_kmeans_zscore(C.c_void_p(X.ptr), S, D, C.c_void_p(stats.ptr), C.c_void_p(zws.ptr), zws.nbytes,
                                    _s()) == 0, lib.ocm_last_error()
    c = torch.from_numpy(cand).to(dev)
    d1 = _g(n * 8, dev, out_pattern)
    d3 = _g(3 * n * 8, dev, out_pattern)
    assert lib.ocm_op_kmeans_dist(C.c_void_p(X.ptr), S, D, C.c_void_p(c.data_ptr()), 1, None, C.c_void_p(d1.ptr),
                                  _s()) == 0
    assert lib.ocm_op_kmeans_dist(C.c_void_p(X.ptr), S, D, C.c_void_p(c[1:].data_ptr()), 3, C.c_void_p(d1.ptr),
                                  C.c_void_p(d3.ptr), _s()) == 0
    ce = torch.from_numpy(cen).to(dev)
    lo = torch.from_numpy(lab_old).to(dev)
    lws = _g(lib.ocm_kmeans_lloyd_workspace_bytes(S, D), dev, ws_pattern)
    outs = dict(labels=_g(n * 4, dev, out_pattern), new=_g(2 * D * 4, dev, out_pattern),
                sums=_g(2 * D * 8, dev, out_pattern), info=_g(7 * 8, dev, out_pattern),
                labels_a=_g(n * 4, dev, out_pattern), info_a=_g(7 * 8, dev, out_pattern))
    p = {k: C.c_void_p(v.ptr) for k, v in outs.items()}
    assert lib.ocm_op_kmeans_lloyd(C.c_void_p(X.ptr), S, D, C.c_void_p(ce.data_ptr()), C.c_void_p(lo.data_ptr()),
                                   p["labels"], p["new"], p["sums"], p["info"], 0, C.c_void_p(lws.ptr), lws.nbytes,
                                   _s()) == 0
    assert lib.ocm_op_kmeans_lloyd(C.c_void_p(X.ptr), S, D, C.c_void_p(ce.data_ptr()), None, p["labels_a"], None, None,
                                   p["info_a"], 1, C.c_void_p(lws.ptr), lws.nbytes, _s()) == 0
    torch.cuda.synchronize()
    for name, buf in [("X", X), ("stats", stats), ("zscore ws", zws), ("d1", d1), ("d3", d3), ("lloyd ws", lws)] + \
            list(outs.items()):
        assert buf.check() is None, (name, buf.check())
    res = {"X": X.payload(torch.float32).clone(), "stats": stats.payload(torch.float64).clone(),
           "d1": d1.payload(torch.float64).clone(), "d3": d3.payload(torch.float64).clone()}
    for k in ("labels", "labels_a"):
        res[k] = outs[k].payload(torch.int32).clone()
    res["new"] = outs["new"].payload(torch.float32).clone()
    for k in ("sums", "info", "info_a"):
        res[k] = outs[k].payload(torch.float64).clone()
    return res


@pytest.mark.parametrize("S,D", [(24, 384), (7, 12), (33, 1024), (5, 192), (6, 640), (5, 768), (6, 896)])
@pytest.mark.parametrize("poison", POISON)
def test_kmeans_kernels_guarded(dev, lib, S, D, poison):
    rs = np.random.RandomState(S + D)
    x = torch.from_numpy(rs.standard_normal((S * S, D)).astype(np.float32) * 2 + 1)
    cand = rs.standard_normal((4, D)).astype(np.float32)
    cen = rs.standard_normal((2, D)).astype(np.float32)
    lab_old = rs.randint(0, 2, S * S).astype(np.int32)
    inputs = (x, cand, cen, lab_old)
    a = _run(dev, lib, S, D, poison, "nan", inputs)
    b = _run(dev, lib, S, D, poison, "zero", inputs)
    c = _run(dev, lib, S, D, "zero", "nan", inputs)
    for k in a:
        assert_same_bits(a[k], b[k], f"{k} (nan- vs zero-filled outputs, workspace {poison})")
        assert_same_bits(a[k], c[k], f"{k} (workspace {poison} vs zero)")
        if a[k].is_floating_point():
            assert not bool(torch.isnan(a[k]).any()), k
