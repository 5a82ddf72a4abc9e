"""Memory behaviour of ocm_op_resample_u8 (kernels_resample.hip) with the tests/memcheck.py helpers: the uint8 output, the
float32 output and an exactly sized workspace each in a guard-banded buffer, pre-filled with the `nan`, `ones` and `zero`
patterns in turn, for shared tables and for per-image crop rectangles. Each case asserts OCM_OK, intact guards, and results
identical across the patterns (nothing reads a byte of the intermediate it did not write in the same call) and equal to the
restatement. Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import resample_ref as R
from tests.memcheck import Guarded, assert_same_bits

pytestmark = pytest.mark.gpu

PATTERNS = ["nan", "ones", "zero"]
B = 3


def _tables(filt, sizes, out, flips, box=None):
    ks = [R.ksize_of(filt, *((0, n) if box is None else box), out) for n in sizes]
    tabs = [R.table(filt, n, *((0, n) if box is None else box), out, f, max(ks)) for n, f in zip(sizes, flips)]
    return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), max(ks)


def _run(dev, lib, x, chans, rects, tables, out_hw, pattern, outputs):
    (xb, xc, xk), (yb, yc, yk) = tables
    out_h, out_w = out_hw
    H, W = x.shape[1:3]
    tmp_rows = H if rects is None else int(rects[:, 2].max())
    sizes = dict(u8=B * out_h * out_w * chans, f32=B * chans * out_h * out_w * 4,
                 ws=lib.ocm_resample_u8_workspace_bytes(B, chans, tmp_rows, out_w))
    assert sizes["ws"] >= B * tmp_rows * out_w * chans
    g = {k: Guarded(v, dev, pattern) for k, v in sizes.items()}
    dev_tabs = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (xb, xc, yb, yc)]
    dev_rects = None if rects is None else torch.from_numpy(rects.astype(np.int32)).to(dev)
    rc = lib.ocm_op_resample_u8(x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), 1, B, chans, H, W,
                                None if dev_rects is None else C.c_void_p(dev_rects.data_ptr()), tmp_rows,
                                dev_tabs[0].data_ptr(), dev_tabs[1].data_ptr(), xk, dev_tabs[2].data_ptr(), dev_tabs[3].data_ptr(), yk,
                                int(xb.shape[0] > 1), out_h, out_w, C.c_void_p(g["u8"].ptr) if "u8" in outputs else None,
                                C.c_void_p(g["f32"].ptr) if "f32" in outputs else None, C.c_void_p(g["ws"].ptr), g["ws"].nbytes,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ocm_last_error().decode()
    torch.cuda.synchronize()
    for name, buf in g.items():
        assert buf.check() is None, (name, pattern, buf.check())
    return dict(u8=g["u8"].payload(torch.uint8).clone(), f32=g["f32"].payload(torch.int32).clone())  # the floats as bits


@pytest.mark.parametrize("outputs", [("u8", "f32"), ("u8",), ("f32",)], ids=lambda o: "+".join(o))
@pytest.mark.parametrize("chans", [1, 3])
@pytest.mark.parametrize("shape", [((37, 53), (24, 24)), ((9, 11), (64, 80))], ids=["37x53-24x24", "9x11-64x80"])
def test_resample_guarded(dev, lib, shape, chans, outputs):
    (H, W), (h, w) = shape
    imgs = np.stack([R.noise(H, W, 3, seed=s)[:, :, :chans] for s in (1, 2, 3)])
    x = torch.from_numpy(np.ascontiguousarray(imgs)).to(dev)
    filt = R.BICUBIC
    # shared tables over the whole source, then one rectangle (y0, x0, h, w) and one pair of flips per image
    rects = np.array([[0, 0, H, W], [2, 3, H - 4, W - 5], [H - 5, 1, 5, 7]])
    hf, vf = [False, True, True], [True, False, True]
    cases = {
        "shared": (None, (_tables(filt, [W], w, [False]), _tables(filt, [H], h, [False])),
                   [R.resize(im, (w, h), filt) for im in imgs]),
        "per image": (rects, (_tables(filt, rects[:, 3], w, hf), _tables(filt, rects[:, 2], h, vf)),
                      [R.resize(imgs[b], (w, h), filt, crop=(r[1], r[0], r[1] + r[3], r[0] + r[2]), hflip=hf[b], vflip=vf[b])
                       for b, r in enumerate(rects)]),
    }
    for name, (rc, tables, want) in cases.items():
        res = {pat: _run(dev, lib, x, chans, rc, tables, (h, w), pat, outputs) for pat in PATTERNS}
        first = res[PATTERNS[0]]
        for pat in PATTERNS[1:]:
            for k in outputs:
                assert_same_bits(first[k], res[pat][k], f"{name}, {k}: pattern {PATTERNS[0]} vs {pat}")
        want = np.stack(want).reshape(B, h, w, chans)
        if "u8" in outputs:
            assert np.array_equal(first["u8"].cpu().numpy().reshape(B, h, w, chans), want), name
        if "f32" in outputs:
            want_f = (want.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)).view(np.int32)
            assert np.array_equal(first["f32"].cpu().numpy().reshape(B, chans, h, w), want_f), name
        for k in {"u8", "f32"} - set(outputs):  # an output that was not asked for is not written
            untouched = first[k].view(torch.uint8)
            assert torch.equal(untouched, Guarded(untouched.numel(), dev, PATTERNS[0]).payload(torch.uint8)), (name, k)
