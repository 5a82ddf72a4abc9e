"""ROI-guided SimMIM masks on the device (kernels_roi.hip, data.roi_mask, data.SimMIMTransform): every mask and every `used`
flag bit-equal to tests/roi_mask_ref.py, on image families mixed within a batch so that one image leaking into another shows.
Needs an MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import roi_mask_ref as R
from vit_ocm_wmsegmentation_amd import data

pytestmark = pytest.mark.gpu

T = 32  # ocm_label8_tile(), asserted below: the (2T + 3, 7) geometry has components across label tiles
BATCHES = [["mixed", "dark", "count19", "count20", "disjoint", "gap", "count19", "mixed"],
           ["grey_a", "dark", "grey_b", "edge", "mixed", "count20"]]


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _check(new, used, want, what):
    new, used = new.cpu().numpy(), used.cpu().numpy()
    for b, (w_mask, w_used) in enumerate(want):
        assert bool(used[b]) == w_used, f"{what}: used of image {b}"
        assert np.array_equal(new[b], w_mask), f"{what}: mask of image {b}"


@pytest.mark.parametrize("h,w,gh,gw", R.geometries(T))
def test_families_bit_equal(dev, lib, h, w, gh, gw):
    assert lib.ocm_label8_tile() == T
    fam, ref = R.families(h, w, gh, gw), R.reference(h, w, gh, gw)
    for names in BATCHES:
        names = [n for n in names if n in fam]
        assert len(names) <= 8
        imgs, masks = R.batch(fam, names)
        new, used = data.roi_mask(_t(imgs, dev), _t(masks, dev))
        assert new.dtype == torch.int64 and new.shape == (len(names), gh, gw) and new.is_cuda
        assert used.dtype == torch.bool and used.shape == (len(names),) and used.is_cuda
        _check(new, used, [ref[n] for n in names], f"{h}x{w} -> {gh}x{gw} {names}")


def test_label_wrap(dev):
    """256 components: the cell that samples label 256 comes out 0 (the uint8 cast of the reference wraps), the other 255 stay."""
    img, m, (want, want_used) = R.wrap_case()
    dark = np.zeros_like(img)
    new, used = data.roi_mask(_t(np.stack([dark, img, img]), dev), _t(np.stack([m, m, m]), dev))
    _check(new, used, [(m, False), (want, want_used), (want, want_used)], "wrap")
    assert want_used and int(new[1].sum()) == 255 and int(new[1, 15, 15]) == 0


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.bool])
def test_mask_dtypes(dev, dtype):
    h, w, gh, gw = 37, 37, 5, 5
    fam, ref = R.families(h, w, gh, gw), R.reference(h, w, gh, gw)
    names = ["mixed", "dark", "count20", "disjoint"]
    imgs, masks = R.batch(fam, names)
    m = _t(masks, dev).to(dtype)
    if dtype == torch.uint8:
        m = m * 255  # any nonzero value is a masked cell; the result holds 0 / 1
    new, used = data.roi_mask(_t(imgs, dev), m)
    assert new.dtype == dtype and new.shape == m.shape
    _check(new.to(torch.int64), used, [ref[n] for n in names], f"dtype {dtype}")
    assert int(new.to(torch.int64).max()) == 1


def test_strided_and_single_channel_images(dev):
    h, w, gh, gw = 40, 56, 5, 8
    fam, ref = R.families(h, w, gh, gw), R.reference(h, w, gh, gw)
    names = ["mixed", "grey_a", "dark", "gap"]
    imgs, masks = R.batch(fam, names)
    want = [ref[n] for n in names]
    big = torch.full((2 * len(names), 4, h, w), 0.9, dtype=torch.float32, device=dev)  # bright everywhere else
    big[1::2, :3] = _t(imgs, dev)
    view = big[1::2, :3]
    assert not view.is_contiguous() and view.stride(0) == 2 * 4 * h * w
    new, used = data.roi_mask(view, _t(masks, dev))
    _check(new, used, want, "batch slice")
    column_major = _t(imgs, dev).transpose(2, 3).contiguous().transpose(2, 3)  # rows not dense: copied inside
    assert column_major.stride(3) != 1
    new, used = data.roi_mask(column_major, _t(masks, dev))
    _check(new, used, want, "transposed storage")
    flat = torch.zeros(imgs.size + 1, dtype=torch.float32, device=dev)  # one float off the 16-byte grid: one pixel per thread
    shifted = flat[1:].view(imgs.shape)
    shifted.copy_(_t(imgs, dev))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    new, used = data.roi_mask(shifted, _t(masks, dev))
    _check(new, used, want, "unaligned storage")
    grey = np.stack([fam[n][0][:1] for n in names])  # one plane is its own grey image
    new, used = data.roi_mask(_t(grey, dev), _t(masks, dev))
    _check(new, used, [R.roi_mask(g, m) for g, m in zip(grey, masks)], "one channel")


def test_same_call_twice_same_bits(dev):
    h, w, gh, gw = 2 * T + 3, 2 * T + 3, 7, 7
    imgs, masks = R.batch(R.families(h, w, gh, gw), BATCHES[0])
    x, m = _t(imgs, dev), _t(masks, dev)
    a, b = data.roi_mask(x, m), data.roi_mask(x, m)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_level_and_min_size_arguments(dev):
    h, w, gh, gw = 32, 32, 4, 4
    fam = R.families(h, w, gh, gw)
    names = ["grey_a", "count19", "count20"]
    imgs, masks = R.batch(fam, names)
    for level, min_size in [(9, 20), (11, 20), (10, 19), (10, 21)]:
        new, used = data.roi_mask(_t(imgs, dev), _t(masks, dev), level=level, min_size=min_size)
        _check(new, used, [R.roi_mask(i, m, level, min_size) for i, m in zip(imgs, masks)], f"level {level} min_size {min_size}")


# ---- SimMIMTransform ------------------------------------------------------------------------------------------------------------
def _args(roi):
    return SimpleNamespace(DATA=SimpleNamespace(IMG_SIZE=64, MASK_PATCH_SIZE=16, MASK_RATIO=0.5),
                           MODEL=SimpleNamespace(PATCH_SIZE=8), roi_masking=roi)


def _tiles(dev, batch=2):
    """uint8 (B,80,96,3): tissue-like bright noise on the left part, black elsewhere."""
    rs = np.random.RandomState(21)
    u = np.zeros((batch, 80, 96, 3), np.uint8)
    u[:, 8:60, 4:50] = rs.randint(40, 256, size=(batch, 52, 46, 1))
    return torch.from_numpy(u).to(dev)


def _draws(batch):
    gen = data.MaskGenerator(64, 16, 8, 0.5)
    return np.stack([gen() for _ in range(batch)]).astype(np.int64)


def test_transform_without_roi_masking(dev):
    tiles = _tiles(dev)
    np.random.seed(7)
    img, mask = data.SimMIMTransform(_args(False))(tiles, torch.Generator().manual_seed(11))
    np.random.seed(7)
    want_mask = _draws(2)
    assert img.dtype == torch.float32 and img.shape == (2, 3, 64, 64)
    assert torch.equal(img, data.simmim_images(tiles, 64, torch.Generator().manual_seed(11)))
    assert mask.dtype == torch.int64 and mask.is_cuda and np.array_equal(mask.cpu().numpy(), want_mask)


def test_transform_with_roi_masking_feeds_mim(dev):
    from tests import test_mim_train_gpu as TM
    tiles = _tiles(dev)
    np.random.seed(7)
    img, mask = data.SimMIMTransform(_args(True))(tiles, torch.Generator().manual_seed(11))
    np.random.seed(7)
    draws = _draws(2)
    assert torch.equal(img, data.simmim_images(tiles, 64, torch.Generator().manual_seed(11)))
    want, used = data.roi_mask(img, torch.from_numpy(draws).to(dev))
    assert mask.dtype == torch.int64 and mask.shape == (2, 8, 8) and torch.equal(mask, want)
    host = [R.roi_mask(i, m) for i, m in zip(img.cpu().numpy(), draws)]
    _check(mask, used, host, "transform")
    assert all(u for _, u in host) and not np.array_equal(mask.cpu().numpy(), draws)  # the ROI step did something
    # the pair feeds MIM.forward as it stands: the loss against the float64 twin, as tests/test_mim_train_gpu.py measures it
    name, precision = "wrap_p8_64", "fp32"
    mim, _, _ = TM._model(name, precision, dev)
    loss, rec, pixel_mask = mim(img, mask)
    loss64, _, _ = TM._twin(name, TM._twin_params(name), img.cpu(), mask.cpu())
    loss64 = float(loss64.detach())
    assert rec.shape == img.shape and pixel_mask.shape == (2, 1, 64, 64)
    assert abs(float(loss.detach()) - loss64) <= TM.FWD_TOL[precision] * max(1.0, abs(loss64))
