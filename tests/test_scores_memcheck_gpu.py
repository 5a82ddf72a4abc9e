"""Memory behaviour of ocm_op_mask_scores (kernels_score.hip) with the tests/memcheck.py helpers: counts, scores and an exactly
sized workspace each in a guard-banded buffer, pre-filled with the `nan`, `ones` and `zero` patterns in turn. Each case asserts
OCM_OK, intact guards, and results identical across the patterns (nothing reads a slot it did not write in the same call).
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import scores_ref as R
from tests.memcheck import Guarded, assert_same_bits

pytestmark = pytest.mark.gpu

PATTERNS = ["nan", "ones", "zero"]
B = R.B


def _run(dev, lib, pred, target, n, pattern):
    g = dict(counts=Guarded(B * 4 * 8, dev, pattern), scores=Guarded(B * 7 * 8, dev, pattern),
             ws=Guarded(lib.ocm_mask_scores_workspace_bytes(B, n), dev, pattern))
    rc = lib.ocm_op_mask_scores(C.c_void_p(pred.data_ptr()), int(pred.dtype == torch.uint8), C.c_void_p(target.data_ptr()), B, n, 1.0,
                                C.c_void_p(g["counts"].ptr), C.c_void_p(g["scores"].ptr), C.c_void_p(g["ws"].ptr), g["ws"].nbytes,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ocm_last_error().decode()
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.check() is None, (name, pattern, buf.check())
    return dict(counts=g["counts"].payload(torch.int64).clone(), scores=g["scores"].payload(torch.int64).clone())  # scores as bits


@pytest.mark.parametrize("n", [1, 4097, 37 * 53])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_mask_scores_guarded(dev, lib, kind, n):
    pred, target, want_scores, want_counts = R.case(kind, n)
    assert lib.ocm_mask_scores_workspace_bytes(B, n) == B * -(-n // R.SPAN) * R.PART_BYTES
    x, t = torch.tensor(pred, device=dev), torch.tensor(target, device=dev)
    res = {pat: _run(dev, lib, x, t, n, pat) for pat in PATTERNS}
    first = res[PATTERNS[0]]
    for pat in PATTERNS[1:]:
        for k in first:
            assert_same_bits(first[k], res[pat][k], f"{k}: pattern {PATTERNS[0]} vs {pat} at {kind} n={n}")
    assert np.array_equal(first["counts"].cpu().numpy().reshape(B, 4), want_counts)
    scores = first["scores"].view(torch.float64).cpu().numpy().reshape(B, 7)
    assert R.same_bits(scores[:, :6], want_scores[:, :6])
    assert np.abs(scores[:, 6] - want_scores[:, 6]).max() <= R.DICE_BOUND
