"""Memory behaviour of ocm_op_kmeans_px (kernels_kmeans_px.hip) with the tests/memcheck.py helpers: labels, centers,
compactness, iters, best, mask and an exactly sized workspace each in a guard-banded buffer, pre-filled with the `nan`, `ones`
and `zero` patterns in turn. Each case asserts OCM_OK, intact guards, and results identical across the patterns (nothing reads a
slot it did not write in the same call). Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kmeans_px_ref as R
from tests.memcheck import Guarded, assert_same_bits

pytestmark = pytest.mark.gpu

T = 512
PATTERNS = ["nan", "ones", "zero"]
SIZES = [2, T + 1, 4 * T + 5]
P = 3


def _run(dev, lib, px, u, pattern, n, attempts):
    sizes = dict(labels=P * n, centers=P * 6 * 4, compactness=P * attempts * 8, iters=P * attempts * 4, best=P * 4, mask=P * 3 * n,
                 ws=lib.ocm_kmeans_px_workspace_bytes(P, n, attempts))
    assert sizes["ws"] > 0
    g = {k: Guarded(v, dev, pattern) for k, v in sizes.items()}
    rc = lib.ocm_op_kmeans_px(px.data_ptr(), P, n, u.data_ptr(), attempts, 10, 1.0, *(C.c_void_p(g[k].ptr) for k in
                              ("labels", "centers", "compactness", "iters", "best", "mask", "ws")), g["ws"].nbytes,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ocm_last_error().decode()
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.check() is None, (name, pattern, buf.check())
    views = dict(labels=torch.uint8, centers=torch.int32, compactness=torch.int64, iters=torch.int32, best=torch.int32,
                 mask=torch.uint8)  # the floats as bits
    return {k: g[k].payload(t).clone() for k, t in views.items()}


@pytest.mark.parametrize("attempts", [1, 10])
@pytest.mark.parametrize("n", SIZES)
def test_kmeans_px_guarded(dev, lib, n, attempts):
    imgs = np.stack([R.plateaus(n, 3), R.noise(n, 5), R.constant(n, 90)])  # the constant image takes the relocation pass
    uni, _ = R.uniforms_for(P, attempts)
    px, u = torch.from_numpy(imgs).to(dev), torch.from_numpy(uni).to(dev)
    res = {pat: _run(dev, lib, px, u, pat, n, attempts) for pat in PATTERNS}
    first = res[PATTERNS[0]]
    for pat in PATTERNS[1:]:
        for k in first:
            assert_same_bits(first[k], res[pat][k], f"{k}: pattern {PATTERNS[0]} vs {pat} at N = {n}, {attempts} attempts")
    labels, mask = first["labels"].cpu().numpy().reshape(P, n), first["mask"].cpu().numpy().reshape(P, 3 * n)
    centers = first["centers"].view(torch.float32).cpu().numpy().reshape(P, 2, 3)
    assert np.isfinite(first["compactness"].view(torch.float64).cpu().numpy()).all()
    for p in range(P):  # the exact comparison of every output: test_kmeans_px_gpu.py
        ref = R.segment(imgs[p], uni[p], lib)
        assert np.array_equal(labels[p], ref["labels"]) and np.array_equal(mask[p], ref["mask"])
        assert np.array_equal(centers[p].view(np.uint32), ref["centers"].view(np.uint32))
        assert first["iters"].cpu().numpy().reshape(P, attempts)[p].tolist() == ref["iters"].tolist()
        assert int(first["best"][p]) == ref["best"]
