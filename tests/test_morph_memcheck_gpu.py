"""Memory behaviour of the region-query operators (kernels_morph.hip) with the tests/memcheck.py helpers: every output in its
own guard-banded buffer, every workspace an exactly sized guarded payload, all of them pre-filled with the `nan`, `ones`
and `zero` patterns in turn. Each case asserts OCM_OK, intact guards, results equal to tests/morph_ref.py and identical
across the patterns (nothing reads a slot it did not write in the same call). Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import morph_ref as R
from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import utils

pytestmark = pytest.mark.gpu

T = 32
PATTERNS = ["nan", "ones", "zero"]
SIZES = [(1, 1), (T - 1, T + 1), (2 * T + 3, 3 * T + 1), (37, 53)]
GROUP = ["noise", "serpentine", "sizes"]  # three different images per batch


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(dev, lib, masks, pattern, rows, sel, offsets):
    B, h, w = masks.shape
    n = h * w
    m = torch.from_numpy(masks.astype(np.uint8)).to(dev)
    nmax = 8 if n < 64 else 600
    size, bits = utils.footprint_bits(R.DISK2)
    g = dict(labels=Guarded(B * n * 4, dev, pattern), counts=Guarded(B * 4, dev, pattern),
             label_ws=Guarded(lib.ocm_label8_workspace_bytes(B, h, w), dev, pattern),
             removed=Guarded(B * n, dev, pattern),
             remove_ws=Guarded(lib.ocm_remove_small_objects_workspace_bytes(B, h, w), dev, pattern),
             dilated=Guarded(B * n, dev, pattern), closed=Guarded(B * n, dev, pattern), ge=Guarded(B * n, dev, pattern),
             area=Guarded(B * nmax * 8, dev, pattern), sum_row=Guarded(B * nmax * 8, dev, pattern),
             sum_col=Guarded(B * nmax * 8, dev, pattern), bbox=Guarded(B * nmax * 16, dev, pattern),
             qmean=Guarded(rows.shape[0] * rows.shape[3] * 4, dev, pattern))
    p = {k: C.c_void_p(v.ptr) for k, v in g.items()}
    ok = lambda rc: rc == 0 or pytest.fail(lib.ocm_last_error().decode())  # noqa: E731
    ok(lib.ocm_op_label8(m.data_ptr(), p["labels"], p["counts"], B, h, w, p["label_ws"], g["label_ws"].nbytes, _s()))
    ok(lib.ocm_op_remove_small_objects(m.data_ptr(), p["removed"], B, h, w, 20, p["remove_ws"], g["remove_ws"].nbytes, _s()))
    ok(lib.ocm_op_binary_morph(m.data_ptr(), p["dilated"], B, h, w, bits, size, 0, 0, _s()))
    ok(lib.ocm_op_binary_morph(p["dilated"], p["closed"], B, h, w, bits, size, 1, 1, _s()))
    ok(lib.ocm_op_mask_ge_u8(m.data_ptr(), p["ge"], B * n, 1, _s()))
    ok(lib.ocm_op_region_stats(p["labels"], B, h, w, nmax, p["area"], p["sum_row"], p["sum_col"], p["bbox"], _s()))
    Tq, H, Rr, P = rows.shape
    ok(lib.ocm_op_query_mean(rows.data_ptr(), sel.data_ptr(), offsets.data_ptr(), p["qmean"], Tq, H, Rr, P, sel.numel(), _s()))
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.check() is None, (name, pattern, buf.check())
    dt = dict(labels=torch.int32, counts=torch.int32, area=torch.int64, sum_row=torch.int64, sum_col=torch.int64,
              bbox=torch.int32, qmean=torch.int32)  # the query mean as bits: its NaN rows compare equal
    return {k: g[k].payload(dt.get(k, torch.uint8)).clone() for k in g if not k.endswith("_ws")}


@pytest.mark.parametrize("h,w", SIZES)
def test_morph_operators_guarded(dev, lib, h, w):
    fam, ref = R.families(h, w, T), R.reference(h, w, T)
    masks = np.stack([fam[n] for n in GROUP])
    rs = np.random.RandomState(h * w)
    rows = torch.from_numpy(rs.standard_normal((3, 3, 4, 49)).astype(np.float32)).to(dev)
    sel = torch.tensor([2, 0, 2, 3, 1], dtype=torch.int32, device=dev)
    offsets = torch.tensor([0, 4, 4, 5], dtype=torch.int32, device=dev)
    res = {pat: _run(dev, lib, masks, pat, rows, sel, offsets) for pat in PATTERNS}
    first = res[PATTERNS[0]]
    for pat in PATTERNS[1:]:
        for k in first:
            assert_same_bits(first[k], res[pat][k], f"{k}: pattern {PATTERNS[0]} vs {pat} at {h}x{w}")
    B, n = 3, h * w
    assert np.array_equal(first["labels"].cpu().numpy().reshape(B, h, w), np.stack([ref[k]["labels"] for k in GROUP]))
    assert first["counts"].cpu().tolist() == [ref[k]["n"] for k in GROUP]
    assert np.array_equal(first["removed"].cpu().numpy().reshape(B, h, w), np.stack([ref[k]["removed"] for k in GROUP]))
    assert np.array_equal(first["closed"].cpu().numpy().reshape(B, h, w), np.stack([ref[k]["closed"] for k in GROUP]))
    assert np.array_equal(first["ge"].cpu().numpy().reshape(B, h, w), masks)
    nmax = first["area"].numel() // B
    for b, k in enumerate(GROUP):
        area, sr, sc, bbox = R.region_sums(ref[k]["labels"], nmax)
        assert np.array_equal(first["area"].cpu().numpy().reshape(B, nmax)[b], area)
        assert np.array_equal(first["sum_row"].cpu().numpy().reshape(B, nmax)[b], sr)
        assert np.array_equal(first["sum_col"].cpu().numpy().reshape(B, nmax)[b], sc)
        assert np.array_equal(first["bbox"].cpu().numpy().reshape(B, nmax, 4)[b], bbox)
    want = R.query_mean(rows.cpu().numpy(), [[2, 0, 2, 3], [], [1]])
    assert np.array_equal(first["qmean"].cpu().numpy().view(np.float32).reshape(3, 49), want, equal_nan=True)
