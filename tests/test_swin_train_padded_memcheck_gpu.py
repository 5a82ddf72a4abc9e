"""The padded-geometry operators of Swin training (ocm_op_swin_pad_rows / _crop_rows, ocm_op_swin_merge_gather_pad /
_scatter_pad) on guard-banded outputs (tests/memcheck.py) under two fills: no store outside an output, every output byte
written, the same bits under both fills. Each operator has a case whose padded row (or out-of-grid slot) is the very last of
the destination. Needs an MI355X."""
import pytest
import torch
import torch.nn.functional as F

from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _run(lib, what, nbytes, call):
    """`call(ptr)` writes an output of `nbytes` bytes; under a NaN fill and a zero fill -> the output as int32 words."""
    results = []
    for fill in ("nan", "zero"):
        g = Guarded(nbytes, "cuda", fill)
        torch.cuda.synchronize()
        rc = call(g.ptr)
        assert rc == 0, f"{what}: {lib.ocm_last_error().decode()}"
        torch.cuda.synchronize()
        assert g.check() is None, f"{what}: {g.check()}"
        results.append(g.payload(torch.int32).clone())
    assert_same_bits(results[0], results[1], f"{what} under two output fills")  # a byte left unwritten differs
    return results[0]


# the last destination row is a padded one in all but the identity; (1, 1, 1 -> 2, 2) has three padded rows to one real row
@pytest.mark.parametrize("B,H,W,Hp,Wp,row_bytes", [(2, 5, 3, 6, 4, 48), (1, 15, 15, 21, 21, 384), (65, 7, 7, 7, 7, 16),
                                                   (1, 1, 1, 2, 2, 1552), (3, 4, 4, 4, 6, 128)])
def test_pad_and_crop_rows_guarded(lib, B, H, W, Hp, Wp, row_bytes):
    n = row_bytes // 4
    g = torch.Generator().manual_seed(H + Hp)
    x = torch.randint(1, 2 ** 31 - 1, (B, H, W, n), generator=g, dtype=torch.int32).cuda()
    out = _run(lib, "pad_rows", B * Hp * Wp * row_bytes,
               lambda o: lib.ocm_op_swin_pad_rows(x.data_ptr(), o, B, H, W, Hp, Wp, row_bytes, None))
    assert torch.equal(out.view(B, Hp, Wp, n), F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H)))
    xp = torch.randint(1, 2 ** 31 - 1, (B, Hp, Wp, n), generator=g, dtype=torch.int32).cuda()
    out = _run(lib, "crop_rows", B * H * W * row_bytes,
               lambda o: lib.ocm_op_swin_crop_rows(xp.data_ptr(), o, B, H, W, Hp, Wp, row_bytes, None))
    assert torch.equal(out.view(B, H, W, n), xp[:, :H, :W].contiguous())


# odd sides: the last gathered row's x1 | x2 | x3 slots are out of the grid (the last 16 bytes of y are zeros the kernel wrote)
@pytest.mark.parametrize("B,H,W,Cn", [(3, 5, 5, 32), (1, 7, 9, 384), (1, 1, 1, 32), (2, 6, 3, 64), (2, 4, 6, 96)])
def test_merge_gather_scatter_pad_guarded(lib, B, H, W, Cn):
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    g = torch.Generator().manual_seed(H * 10 + W)
    x = (torch.rand(B, H, W, Cn, generator=g) + 0.5).cuda()
    y = _run(lib, "merge_gather_pad", B * H2 * W2 * 4 * Cn * 4,
             lambda o: lib.ocm_op_swin_merge_gather_pad(x.data_ptr(), o, B, H, W, Cn, None)).view(torch.float32)
    xp = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    want = torch.cat([xp[:, r::2, c::2, :] for c in range(2) for r in range(2)], -1).reshape(-1)
    assert torch.equal(y, want)
    if H % 2 and W % 2:
        assert not y[-3 * Cn:].any()
    dy = (torch.rand(B * H2 * W2, 4 * Cn, generator=g) + 0.5).cuda()
    dx = _run(lib, "merge_scatter_pad", B * H * W * Cn * 4,
              lambda o: lib.ocm_op_swin_merge_scatter_pad(dy.data_ptr(), o, B, H, W, Cn, None)).view(torch.float32)
    back = _run(lib, "merge_gather_pad of the scatter", B * H2 * W2 * 4 * Cn * 4,
                lambda o: lib.ocm_op_swin_merge_gather_pad(dx.data_ptr(), o, B, H, W, Cn, None)).view(torch.float32)
    assert torch.equal(back, dy.reshape(-1) * (want != 0))
