"""ocm_op_resample_u8 (kernels_resample.hip) and its Python surface — utils.pil_resize, data.py, sw_processing.prepare_slab —
against the numpy restatement tests/resample_ref.py (itself pinned on live Pillow by tests/test_resample_host.py). Every
comparison is exact: bytes, and float32 bit patterns. Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import resample_ref as R
from tests.helpers import CASES, build_module
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import data, sw_processing, utils

pytestmark = pytest.mark.gpu

FILTERS = [R.NEAREST, R.BILINEAR, R.BICUBIC]
ALL_SHAPES = R.SHAPES + R.tile_edge_shapes()


def _same(got, want, what):
    """a device tensor against a numpy array: the same shape, dtype and bits"""
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, tuple(got.shape), tuple(want.shape))
    g, w = got.cpu().contiguous(), want
    if g.dtype == torch.float32:
        g, w = g.view(torch.int32), w.view(torch.int32)
    assert_same_bits(g, w, what)


def _tensor_of(u8):
    """ToTensor as the issue states it: np.float32(u8) / np.float32(255), CHW"""
    t = R.to_tensor(u8)
    assert t.dtype == np.float32
    return t


@pytest.mark.parametrize("chans", [1, 3])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_shapes(dev, shape, chans):
    (H, W), (h, w) = shape
    img = R.noise(H, W, chans, seed=3 * H + W + chans)
    x = torch.from_numpy(img).to(dev)
    for filt in FILTERS:
        want = R.resize(img, (w, h), filt)
        u8, f32 = utils.pil_resize(x, (w, h), filt, to_tensor="both")
        _same(u8, want, f"{shape} C={chans} filter {filt}: uint8")
        _same(f32, _tensor_of(want), f"{shape} C={chans} filter {filt}: float32")


@pytest.mark.parametrize("chans", [1, 3])
def test_clamping(dev, chans):
    img = R.blocks(50, 70, chans)
    want, hsums, vsums = R.resize(img, (96, 128), R.BICUBIC, return_sums=True)
    for sums in (hsums, vsums):  # both clamps of both passes are exercised
        assert (sums < 0).any() and ((sums >> R.PRECISION_BITS) > 255).any()
    assert (want == 0).any() and (want == 255).any()
    u8, f32 = utils.pil_resize(torch.from_numpy(img).to(dev), (96, 128), R.BICUBIC, to_tensor="both")
    _same(u8, want, "0 / 255 blocks: uint8")
    _same(f32, _tensor_of(want), "0 / 255 blocks: float32")


@pytest.mark.parametrize("filt", FILTERS)
def test_per_image_tables_and_box(dev, filt):
    """Three images, each with its own crop rectangle (different sizes, so different ksize, padded to the largest) and its own
    flips; then the same batch with one fractional box, whose taps read outside it."""
    imgs = np.stack([R.noise(61, 83, 3, seed=s) for s in (1, 2, 3)])
    x = torch.from_numpy(imgs).to(dev)
    crops = [(5, 3, 83, 61), (0, 0, 30, 22), (40, 17, 41, 60)]  # (x0, y0, x1, y1): 78 x 58, 30 x 22, 1 x 43
    hf, vf = [False, True, True], [True, False, True]
    size = (24, 20)
    got = utils.pil_resize(x, size, filt, crop=crops, hflip=hf, vflip=vf, to_tensor="both")
    want = np.stack([R.resize(imgs[b], size, filt, crop=crops[b], hflip=hf[b], vflip=vf[b]) for b in range(3)])
    _same(got[0], want, f"per-image crops, filter {filt}: uint8")
    _same(got[1], np.stack([_tensor_of(w) for w in want]), f"per-image crops, filter {filt}: float32")
    # one rectangle and one flip for the whole batch: shared tables
    got = utils.pil_resize(x, size, filt, crop=crops[0], hflip=True)
    _same(got, np.stack([R.resize(im, size, filt, crop=crops[0], hflip=True) for im in imgs]), f"shared crop, filter {filt}")
    box = (3.3, 2.6, 71.2, 50.9)
    got = utils.pil_resize(x, size, filt, box=box)
    want_box = np.stack([R.resize(im, size, filt, box=box) for im in imgs])
    _same(got, want_box, f"fractional box, filter {filt}")
    if filt != R.NEAREST:  # a box is not a crop: the taps of its border pixels lie outside it
        as_crop = np.stack([R.resize(im, size, filt, crop=(3, 3, 71, 51)) for im in imgs])
        assert (want_box != as_crop).any()
    # a box inside per-image crops
    got = utils.pil_resize(x[:2], size, filt, crop=crops[:2], box=(1.5, 2.0, 28.25, 20.5))
    want = np.stack([R.resize(imgs[b], size, filt, crop=crops[b], box=(1.5, 2.0, 28.25, 20.5)) for b in range(2)])
    _same(got, want, f"box inside per-image crops, filter {filt}")


@pytest.mark.parametrize("to_tensor", [False, True, "both"])
def test_layouts_and_outputs(dev, to_tensor):
    imgs = np.stack([R.noise(37, 53, 3, seed=s) for s in (4, 5)])
    size, filt = (24, 24), R.BICUBIC
    want_u8 = np.stack([R.resize(im, size, filt) for im in imgs])
    want_f32 = np.stack([_tensor_of(w) for w in want_u8])

    def check(got, what, u8=want_u8, f32=want_f32):
        if to_tensor == "both":
            _same(got[0], u8, what + ": uint8")
            _same(got[1], f32, what + ": float32")
        else:
            _same(got, f32 if to_tensor else u8, what)

    hwc = torch.from_numpy(imgs).to(dev)
    check(utils.pil_resize(hwc, size, filt, to_tensor=to_tensor), "HWC")
    planar = hwc.permute(0, 3, 1, 2).contiguous()  # (B,3,H,W)
    check(utils.pil_resize(planar, size, filt, to_tensor=to_tensor), "planar")
    check(utils.pil_resize(planar, size, filt, to_tensor=to_tensor, layout="chw"), "planar, named")
    wide = torch.full((2, 40, 64, 3), 255, dtype=torch.uint8, device=dev)  # a row pitch wider than the image, and more rows
    wide[:, 2:39, 7:60] = hwc
    view = wide[:, 2:39, 7:60]
    assert not view.is_contiguous()
    check(utils.pil_resize(view, size, filt, to_tensor=to_tensor), "row pitch")
    wide_planar = torch.full((2, 3, 40, 64), 255, dtype=torch.uint8, device=dev)
    wide_planar[:, :, 2:39, 7:60] = planar
    check(utils.pil_resize(wide_planar[:, :, 2:39, 7:60], size, filt, to_tensor=to_tensor), "planar row pitch")
    # one image, with and without its channel axis
    check(utils.pil_resize(hwc[1], size, filt, to_tensor=to_tensor), "one (H,W,C) image", want_u8[1], want_f32[1])
    gray = np.ascontiguousarray(imgs[0, :, :, 1])
    want_gray = R.resize(gray, size, filt)
    check(utils.pil_resize(torch.from_numpy(gray).to(dev), size, filt, to_tensor=to_tensor), "(H,W) image", want_gray,
          _tensor_of(want_gray))
    check(utils.pil_resize(torch.from_numpy(gray[:, :, None].copy()).to(dev), size, filt, to_tensor=to_tensor), "(H,W,1) image",
          want_gray[:, :, None], _tensor_of(want_gray))


def test_resize_to_tensor(dev):
    """data.py:28-30 / :70-74: Resize + ToTensor + the cut to a multiple of 8, for images (BILINEAR, NEAREST) and labels."""
    imgs = np.stack([R.noise(45, 70, 3, seed=s) for s in (6, 7)])
    labels = (np.stack([R.blocks(45, 70, 0, seed=s, side=5) for s in (6, 7)]))
    x, lab = torch.from_numpy(imgs).to(dev), torch.from_numpy(labels).to(dev)
    for filt in (R.BILINEAR, R.NEAREST):
        got = data.resize_to_tensor(x, (37, 51), filt)
        want = np.stack([_tensor_of(R.resize(im, (51, 37), filt))[:, :32, :48] for im in imgs])
        _same(got, want, f"resize_to_tensor, filter {filt}")
    got = data.resize_to_tensor(lab[:, :, :, None], (37, 51), R.NEAREST)
    want = np.stack([_tensor_of(R.resize(la, (51, 37), R.NEAREST))[:, :32, :48] for la in labels])
    _same(got, want, "labels")
    assert set(np.unique(got.cpu().numpy())) <= {0.0, 1.0}
    got = data.resize_to_tensor(x[0], 30, R.BILINEAR)  # an int: the smaller edge, 45 x 70 -> 30 x 46
    _same(got, _tensor_of(R.resize(imgs[0], (46, 30), R.BILINEAR))[:, :24, :40], "resize_to_tensor, int size")


def test_simmim_images(dev):
    imgs = np.stack([R.noise(70, 90, 3, seed=s) for s in range(5)])
    x = torch.from_numpy(imgs).to(dev)
    got, (crops, hf, vf) = data.simmim_images(x, 32, torch.Generator().manual_seed(7), return_params=True)
    c2, h2, v2 = data.simmim_params(5, 70, 90, torch.Generator().manual_seed(7))
    assert np.array_equal(crops, c2) and np.array_equal(hf, h2) and np.array_equal(vf, v2)
    assert len({(c[2] - c[0], c[3] - c[1]) for c in crops.tolist()}) > 1  # rectangles of different sizes
    want = np.stack([_tensor_of(R.resize(imgs[b], (32, 32), R.BILINEAR, crop=tuple(crops[b]), hflip=hf[b], vflip=vf[b]))
                     for b in range(5)])
    _same(got, want, "simmim_images")


def _pillow_slab(img, size):
    """sw_processing.py:217-222, :229-231 with the live library where it is installed, with the restatement otherwise"""
    try:
        from PIL import Image
    except ImportError:
        rgb = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, 2)
        return _tensor_of(R.resize(rgb, size, R.BICUBIC))
    resized = np.asarray(Image.fromarray(img).convert("RGB").resize(size))
    return _tensor_of(resized)


def test_prepare_slab(dev):
    img = R.noise(150, 130, 3, seed=12) // 2 + R.blocks(150, 130, 3, seed=3, side=17) // 2
    size = (160, 160)
    want = _pillow_slab(img, size)
    assert np.array_equal(want.view(np.uint32), _tensor_of(R.resize(img, size, R.BICUBIC)).view(np.uint32))
    slab = sw_processing.prepare_slab(torch.from_numpy(img).to(dev), size)
    _same(slab, want, "prepare_slab")
    gray = np.ascontiguousarray(img[:, :, 0])
    _same(sw_processing.prepare_slab(torch.from_numpy(gray).to(dev), size), _pillow_slab(gray, size), "prepare_slab of a gray image")
    # either slab through the sweep: identical masks (the smallest model and window of the sliding-window tests)
    model = build_module(CASES["tiny_p8"], dev)
    sweep = sw_processing.SlidingWindowAttention(model, window=96, stride=32, batch_tiles=4)
    a, b = sweep.segment(slab), sweep.segment(torch.from_numpy(want).to(dev))
    for k in ("th", "th2", "th3", "gray", "result"):
        assert_same_bits(a[k], b[k], f"segment()[{k!r}]")
    assert_same_bits(a["heat"], b["heat"], "segment()['heat']")
    assert tuple(a["levels"]) == tuple(b["levels"])


def test_cropped_batch_feeds_segment_images(dev):
    from vit_ocm_wmsegmentation_amd.eval import segment_images
    imgs = np.stack([R.noise(70, 90, 3, seed=s) // 2 + R.blocks(70, 90, 3, seed=s, side=11) // 2 for s in (8, 9)])
    S, s = 64, 32
    got = data.cropped_batch(torch.from_numpy(imgs).to(dev), S, crop=4)
    want = np.empty((2, 4, 3, s, s), np.float32)
    for b in range(2):
        full = _tensor_of(R.resize(imgs[b], (S, S), R.BICUBIC))
        for i in range(2):
            for j in range(2):  # data.py:116-120: rows outside, columns inside
                want[b, 2 * i + j] = full[:, i * s:(i + 1) * s, j * s:(j + 1) * s]
    _same(got, want, "cropped_batch")
    model = build_module(CASES["tiny_p8"], dev)
    masks, maps = segment_images(model, got, method="ours")
    assert tuple(masks.shape) == (2, S, S) and masks.dtype == torch.uint8 and tuple(maps.shape) == (2, S, S)
    ref_masks, ref_maps = segment_images(model, torch.from_numpy(want).to(dev), method="ours")
    assert_same_bits(masks, ref_masks, "masks")
    assert_same_bits(maps, ref_maps, "maps")
    assert set(np.unique(masks.cpu().numpy())) <= {0, 255}
    # crop 16 on a size that leaves a rest: 4 x 4 crops of 70 // 4 = 17 pixels
    got16 = data.cropped_batch(torch.from_numpy(imgs).to(dev), 70, crop=16)
    full = _tensor_of(R.resize(imgs[1], (70, 70), R.BICUBIC))
    assert tuple(got16.shape) == (2, 16, 3, 17, 17)
    _same(got16[1, 4 * 3 + 2], full[:, 51:68, 34:51], "crop 16, row 3, column 2")
