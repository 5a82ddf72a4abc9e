"""Memory behaviour of ocm_op_chan_vese (kernels_levelset.hip) with the tests/memcheck.py helpers: phi, mask, iters and an
exactly sized workspace each in a guard-banded buffer, pre-filled with the `nan`, `ones` and `zero` patterns in turn. Each case
asserts OCM_OK, intact guards, and results identical across the patterns (nothing reads a slot it did not write in the same
call). Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import chan_vese_ref as R
from tests.memcheck import Guarded, assert_same_bits

pytestmark = pytest.mark.gpu

T = 32
PATTERNS = ["nan", "ones", "zero"]
SIZES = [(1, 1), (T - 1, T + 1), (2 * T + 3, 3 * T + 1), (37, 53)]
B = 3


def _run(dev, lib, image, phi0, pattern, max_num_iter):
    _, h, w = image.shape
    n = h * w
    g = dict(phi=Guarded(B * n * 8, dev, pattern), mask=Guarded(B * n, dev, pattern), iters=Guarded(B * 4, dev, pattern),
             ws=Guarded(lib.ocm_chan_vese_workspace_bytes(B, h, w), dev, pattern))
    g["phi"].payload(torch.float64).copy_(phi0.reshape(-1))
    rc = lib.ocm_op_chan_vese(image.data_ptr(), C.c_void_p(g["phi"].ptr), C.c_void_p(g["mask"].ptr), C.c_void_p(g["iters"].ptr),
                              B, h, w, 0.25, 1.0, 1.0, 1e-3, max_num_iter, 0.5, C.c_void_p(g["ws"].ptr), g["ws"].nbytes,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ocm_last_error().decode()
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.check() is None, (name, pattern, buf.check())
    return dict(phi=g["phi"].payload(torch.int64).clone(), mask=g["mask"].payload(torch.uint8).clone(),
                iters=g["iters"].payload(torch.int32).clone())


@pytest.mark.parametrize("max_num_iter", [0, 1, 8])
@pytest.mark.parametrize("h,w", SIZES)
def test_chan_vese_guarded(dev, lib, h, w, max_num_iter):
    imgs = np.stack([R.normalize(R.blobs(h, w, 3)), R.normalize(R.noise(h, w, 5)), R.normalize(R.step_image(h, w))])
    starts = np.stack([R.checkerboard(h, w), R.random_start(h, w, 7), R.checkerboard(h, w)])
    image, phi0 = torch.from_numpy(imgs).to(dev), torch.from_numpy(starts).to(dev)
    res = {pat: _run(dev, lib, image, phi0, pat, max_num_iter) for pat in PATTERNS}
    first = res[PATTERNS[0]]
    for pat in PATTERNS[1:]:
        for k in first:  # phi compared as bits
            assert_same_bits(first[k], res[pat][k], f"{k}: pattern {PATTERNS[0]} vs {pat} at {h}x{w}, {max_num_iter} iterations")
    phi = first["phi"].view(torch.float64).cpu().numpy().reshape(B, h, w)
    assert np.isfinite(phi).all()
    assert np.array_equal(first["mask"].cpu().numpy().reshape(B, h, w), (phi > 0).astype(np.uint8))
    for b in range(B):
        ref = R.evolve(imgs[b], starts[b], max_num_iter=max_num_iter)
        assert int(first["iters"][b]) == ref["iters"]
        assert np.abs(phi[b] - ref["phi"]).max() <= (0.0 if max_num_iter == 0 else 1e-9)  # the exact bounds: test_chan_vese_gpu.py
