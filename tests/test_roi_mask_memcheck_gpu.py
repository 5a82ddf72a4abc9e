"""Memory behaviour of the ROI-mask operators (kernels_roi.hip) with the tests/memcheck.py helpers: the binary mask, `white`, the
result masks and `used` each in a guard-banded buffer, pre-filled with the `nan`, `ones` and `zero` patterns in turn (`white`
is zeroed by the operator itself, so a poisoned one must not show). Each case asserts OCM_OK, intact guards, results equal to
tests/roi_mask_ref.py and identical across the patterns. Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import morph_ref as M
from tests import roi_mask_ref as R
from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import utils

pytestmark = pytest.mark.gpu

T = 32
PATTERNS = ["nan", "ones", "zero"]
SIZES = [(1, 1, 1, 1), (T - 1, T + 1, 3, 5), (37, 53, 5, 7), (T, T + 4, 4, 6)]  # the last: the threshold's four-pixel path
GROUP = ["mixed", "count20", "dark"]  # three different images per batch


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _run(dev, lib, imgs, masks, pattern):
    B, Cc, h, w = imgs.shape
    gh, gw = masks.shape[1:]
    n = h * w
    x = torch.from_numpy(np.array(imgs)).to(dev)
    m = torch.from_numpy(np.array(masks)).to(dev)
    tables = torch.from_numpy(np.concatenate([utils.roi_sample_index(h, gh), utils.roi_sample_index(w, gw)])).to(dev)
    g = dict(binary=Guarded(B * n, dev, pattern), white=Guarded(B * 4, dev, pattern), out=Guarded(B * gh * gw * 8, dev, pattern),
             used=Guarded(B, dev, pattern))
    p = {k: C.c_void_p(v.ptr) for k, v in g.items()}
    grown = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
    closed = torch.empty_like(grown)
    labels = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.ocm_label8_workspace_bytes(B, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    size, bits = utils.footprint_bits(M.DISK2)
    ok = lambda rc: rc == 0 or pytest.fail(lib.ocm_last_error().decode())  # noqa: E731
    ok(lib.ocm_op_roi_threshold(x.data_ptr(), x.stride(0), x.stride(1), Cc, B, h, w, 10, p["binary"], p["white"], _s()))
    ok(lib.ocm_op_binary_morph(p["binary"], grown.data_ptr(), B, h, w, bits, size, 0, 0, _s()))
    ok(lib.ocm_op_binary_morph(grown.data_ptr(), closed.data_ptr(), B, h, w, bits, size, 1, 1, _s()))
    ok(lib.ocm_op_label8(closed.data_ptr(), labels.data_ptr(), counts.data_ptr(), B, h, w, ws.data_ptr(), nbytes, _s()))
    ok(lib.ocm_op_roi_apply(labels.data_ptr(), tables.data_ptr(), tables.data_ptr() + 4 * gh, p["white"], 20, m.data_ptr(), 8,
                            p["out"], p["used"], B, h, w, gh, gw, _s()))
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.check() is None, (name, pattern, buf.check())
    dt = dict(white=torch.int32, out=torch.int64)
    return {k: g[k].payload(dt.get(k, torch.uint8)).clone() for k in g}


@pytest.mark.parametrize("h,w,gh,gw", SIZES)
def test_roi_operators_guarded(dev, lib, h, w, gh, gw):
    assert lib.ocm_label8_tile() == T
    fam = R.families(h, w, gh, gw)
    imgs, masks = R.batch(fam, GROUP)
    res = {pat: _run(dev, lib, imgs, masks, pat) for pat in PATTERNS}
    first = res[PATTERNS[0]]
    for pat in PATTERNS[1:]:
        for k in first:
            assert_same_bits(first[k], res[pat][k], f"{k}: pattern {PATTERNS[0]} vs {pat} at {h}x{w}")
    B = len(GROUP)
    binary = np.stack([R.gray_u8(i) > 10 for i in imgs])
    assert np.array_equal(first["binary"].cpu().numpy().reshape(B, h, w), binary.astype(np.uint8))
    assert first["white"].cpu().tolist() == [int(b.sum()) for b in binary]
    want = [R.roi_mask(i, m) for i, m in zip(imgs, masks)]
    assert np.array_equal(first["out"].cpu().numpy().reshape(B, gh, gw), np.stack([m for m, _ in want]))
    assert first["used"].cpu().tolist() == [int(u) for _, u in want]
