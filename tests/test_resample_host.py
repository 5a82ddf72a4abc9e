"""Host side of the resample path (kernels_resample.hip's ocm_resample_ksize / ocm_resample_table, utils.pil_resize, data.py,
sw_processing.prepare_slab): the numpy restatement tests/resample_ref.py against live Pillow, the C tables against the
restatement's as integers, the C ABI's declarations and refusals, the kernel's tile constants, and torchvision's
RandomResizedCrop.get_params restated on a torch.Generator. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import resample_ref as R
from vit_ocm_wmsegmentation_amd import _lib, data, sw_processing, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc")
NEW_SYMBOLS = ["ocm_resample_ksize", "ocm_resample_table", "ocm_resample_u8_workspace_bytes", "ocm_op_resample_u8"]
FILTERS = [R.NEAREST, R.BILINEAR, R.BICUBIC]
ALL_SHAPES = R.SHAPES + R.tile_edge_shapes()


def _boxes(H, W):
    """none, integer, fractional (values no float32 holds exactly: Pillow rounds a box to floats)"""
    return [None, (1, 2, W - 3, H - 1), (0.3, 1.7, W - 2.4, H - 0.9)]


# ---- the restatement against live Pillow -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_restatement_equals_pillow(shape, filt):
    Image = pytest.importorskip("PIL.Image")
    (H, W), (h, w) = shape
    for c in (0, 3):  # "L" and "RGB"
        img = R.noise(H, W, c, seed=H + W + c)
        for box in _boxes(H, W):
            want = np.asarray(Image.fromarray(img).resize((w, h), filt, box=box))
            got = R.resize(img, (w, h), filt, box)
            assert got.shape == want.shape and np.array_equal(got, want), (shape, filt, c, box, int((got != want).sum()))


@pytest.mark.parametrize("filt", FILTERS)
def test_restatement_equals_pillow_on_crops_and_flips(filt):
    Image = pytest.importorskip("PIL.Image")
    img = R.noise(37, 53, 3, seed=9)
    pil = Image.fromarray(img)
    for crop in ((5, 3, 41, 30), (0, 0, 53, 37), (17, 9, 18, 36)):
        for hflip, vflip in ((False, False), (True, False), (False, True), (True, True)):
            want = pil.crop(crop).resize((24, 20), filt)
            if hflip:
                want = want.transpose(Image.FLIP_LEFT_RIGHT)
            if vflip:
                want = want.transpose(Image.FLIP_TOP_BOTTOM)
            got = R.resize(img, (24, 20), filt, crop=crop, hflip=hflip, vflip=vflip)
            assert np.array_equal(got, np.asarray(want)), (filt, crop, hflip, vflip)


def test_crop_box_and_pass_order_are_different_results():
    """What the device op must keep apart: a crop's taps stop at the rectangle and a box's do not; the horizontal pass runs
    first and its rounding to uint8 is part of the result."""
    img = R.noise(37, 53, 3, seed=2)
    rect = (6, 4, 46, 33)
    crop, box = R.resize(img, (24, 20), R.BICUBIC, crop=rect), R.resize(img, (24, 20), R.BICUBIC, box=rect)
    assert (crop != box).sum() > 100
    hv = R.resize(img, (24, 20), R.BICUBIC)
    vh = R.resize(img.transpose(1, 0, 2), (20, 24), R.BICUBIC).transpose(1, 0, 2)  # vertical first
    assert (hv != vh).sum() > 100


def test_block_pattern_exercises_both_clamps():
    """The device test's clamping input: the sums before the clip leave 0..255 on both sides in the horizontal pass alone."""
    _, hsums, vsums = R.resize(R.blocks(50, 70, 3), (96, 128), R.BICUBIC, return_sums=True)
    below, above = int((hsums < 0).sum()), int(((hsums >> R.PRECISION_BITS) > 255).sum())
    assert below > 1000 and above > 1000, (below, above)
    assert (vsums < 0).any() and ((vsums >> R.PRECISION_BITS) > 255).any()


# ---- ocm_resample_table against the restatement, as integers ----------------------------------------------------------------------
def _assert_table(filt, in_size, in0, in1, out, flip=False, pad=None):
    wb, wc, wk = R.table(filt, in_size, in0, in1, out, flip, pad)
    assert utils.resample_ksize(filt, in_size, in0, in1, out) == wk
    gb, gc = utils.resample_table(filt, in_size, in0, in1, out, flip, pad)
    what = (filt, in_size, in0, in1, out, flip, pad)
    assert gb.dtype == np.int32 and gc.dtype == np.int32 and gb.shape == wb.shape and gc.shape == wc.shape, what
    assert np.array_equal(gb, wb) and np.array_equal(gc, wc), what
    return gb, gc, wk


@pytest.mark.parametrize("filt", FILTERS)
def test_tables_equal_the_restatement(filt):
    for (H, W), (h, w) in ALL_SHAPES:
        for in_size, out in ((W, w), (H, h)):
            for in0, in1 in ((0, in_size), (1, in_size - 2), (0.3, in_size - 2.4)):
                for flip in (False, True):
                    _assert_table(filt, in_size, in0, in1, out, flip)
    # the slab and the SimMIM sizes of tools/bench_resample.py, and the 117 taps of 200 -> 7
    assert _assert_table(filt, 4096, 0, 4096, 1152)[2] == (1 if filt == R.NEAREST else 9 if filt == R.BILINEAR else 17)
    assert _assert_table(filt, 200, 0, 200, 7)[2] == (1 if filt == R.NEAREST else 59 if filt == R.BILINEAR else 117)
    _assert_table(filt, 8192, 0, 8192, 4096)


@pytest.mark.parametrize("filt", FILTERS)
def test_table_padding_flip_identity_and_one_pixel(filt):
    b, c, k = _assert_table(filt, 53, 0, 53, 24, pad=None)
    pb, pc, _ = _assert_table(filt, 53, 0, 53, 24, pad=k + 5)
    assert np.array_equal(pb, b) and np.array_equal(pc[:, :k], c) and not pc[:, k:].any()  # zero-padded
    fb, fc, _ = _assert_table(filt, 53, 0, 53, 24, flip=True, pad=k + 5)
    assert np.array_equal(fb, pb[::-1]) and np.array_equal(fc, pc[::-1])  # the rows reversed, nothing else
    for i in range(24):  # taps past a row's count are zero
        assert not pc[i, pb[i, 1]:].any()
    # scale == 1: the table is the identity (one weight of 2^22 per row, at the row's own pixel)
    ib, ic, _ = _assert_table(filt, 40, 0, 40, 40)
    for i in range(40):
        taps = {ib[i, 0] + j: int(ic[i, j]) for j in range(ib[i, 1]) if ic[i, j]}
        assert taps == {i: 1 << 22}, (i, taps)
    # one source pixel: every output pixel is that pixel
    ob, oc, _ = _assert_table(filt, 1, 0, 1, 5)
    assert np.array_equal(ob, np.array([[0, 1]] * 5)) and oc[:, 0].tolist() == [1 << 22] * 5 and not oc[:, 1:].any()
    assert (c.sum(1) - (1 << 22)).__abs__().max() <= k  # rows sum to one, up to the rounding of each weight


def test_nearest_uses_the_running_sum():
    """ImagingScaleAffine adds the step per pixel; (xx + 0.5) * a truncates to another pixel on 2 -> 7 (and 15 544 more of the
    axes up to 200 -> 400). Live Pillow sides with the running sum."""
    Image = pytest.importorskip("PIL.Image")
    for in_size, out in ((2, 7), (2, 15), (2, 21)):
        b, _, _ = _assert_table(R.NEAREST, in_size, 0, in_size, out)
        closed = np.array([int((xx + 0.5) * (in_size / out)) for xx in range(out)])
        assert (b[:, 1] == 1).all() and (closed != b[:, 0]).sum() == 1, (in_size, out)
        row = np.arange(in_size, dtype=np.uint8)[None] * 100 + 7
        want = np.asarray(Image.fromarray(row).resize((out, 1), R.NEAREST))
        assert np.array_equal(row[:, b[:, 0]], want) and np.array_equal(R.resize(row, (out, 1), R.NEAREST), want)


def test_table_refusals(lib):
    bounds, coeffs = np.empty((8, 2), np.int32), np.empty((8, 32), np.int32)
    bp, cp = bounds.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p)

    def table(filt=3, in_size=20, in0=0.0, in1=20.0, out=8, flip=0, pad=32, b=bp, c=cp):
        return lib.ocm_resample_table(filt, in_size, in0, in1, out, flip, pad, b, c)

    def refused(rc, word):
        assert rc == _lib.OCM_EINVAL, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    assert table() == _lib.OCM_OK
    for filt in (1, 4, 5, -1):  # BOX, HAMMING, LANCZOS are not built
        refused(table(filt=filt), "filter")
    for out in (0, -3):
        refused(table(out=out), "out_size")
    for in_size in (0, -1):
        refused(table(in_size=in_size), "in_size")
    refused(table(in0=5.0, in1=5.0), "empty box")
    refused(table(in0=6.0, in1=5.0), "empty box")
    refused(table(in0=float("nan")), "empty box")
    refused(table(in0=-0.5), "outside")
    refused(table(in1=20.5), "outside")
    refused(table(pad=4), "ksize_padded")  # 20 -> 8 bicubic has 11 taps
    assert lib.ocm_resample_ksize(3, 20, 0.0, 20.0, 8) == 11 and table(pad=11) == _lib.OCM_OK
    refused(table(b=None), "null")
    refused(table(c=None), "null")
    for bad in ((1, 20, 0.0, 20.0, 8), (3, 0, 0.0, 20.0, 8), (3, 20, 0.0, 20.0, 0), (3, 20, 3.0, 3.0, 8), (3, 20, -1.0, 20.0, 8),
                (3, 20, 0.0, 21.0, 8)):
        assert lib.ocm_resample_ksize(*bad) == -_lib.OCM_EINVAL, bad
    with pytest.raises(ValueError):
        utils.resample_table(3, 20, 0, 20, 8, ksize_padded=4)
    with pytest.raises(ValueError):
        utils.resample_ksize(3, 20, 0, 21, 8)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "ocm_vit.h")).read()
    assert re.search(r"#define OCM_ABI_VERSION 20\b", text) and lib.ocm_abi_version() == 20 == _lib.OCM_ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert "kernels_resample.hip" in open(os.path.join(CSRC, "Makefile")).read()
    for name, value in (("NEAREST", 0), ("BILINEAR", 2), ("BICUBIC", 3)):
        assert re.search(rf"#define OCM_RESAMPLE_{name} {value}\b", text) and getattr(utils, name) == value == getattr(R, name)


def test_tile_constants_are_what_the_device_tests_assume():
    src = open(os.path.join(CSRC, "kernels_resample.hip")).read()
    for name, value in R.TILE.items():
        assert re.search(rf"constexpr int {name} = {value};", src), name
    assert "constexpr int RS_VTILE = RS_THREADS * RS_VPACK;" in src and R.VTILE == 1024
    assert "__fdiv_rn((float)v[j], 255.0f)" in src  # ToTensor divides


def test_workspace_sizes_and_operator_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    f = lib.ocm_resample_u8_workspace_bytes
    assert f(1, 1, 1, 1) >= 1 and f(3, 3, 53, 24) >= 3 * 3 * 53 * 24 and f(1, 3, 8192, 4096) >= 8192 * 4096 * 3
    for bad in ((0, 3, 8, 8), (65536, 3, 8, 8), (1, 2, 8, 8), (1, 4, 8, 8), (1, 3, 0, 8), (1, 3, (1 << 19) + 1, 8), (1, 3, 8, 0),
                (1, 3, 8, (1 << 26) // 3 + 1)):
        assert f(*bad) == 0, bad
    p, big = C.c_void_p(4096), 1 << 40

    def call(src=p, strides=(0, 159, 3, 1), batch=1, chans=3, src_h=37, src_w=53, rects=None, tmp_rows=37, xb=p, xc=p, xk=7, yb=p,
             yc=p, yk=7, per_image=0, out_h=24, out_w=24, u8=p, f32=p, ws=p, nbytes=big):
        return lib.ocm_op_resample_u8(src, *strides, batch, chans, src_h, src_w, rects, tmp_rows, xb, xc, xk, yb, yc, yk, per_image,
                                      out_h, out_w, u8, f32, ws, nbytes, None)

    def refused(rc, word):
        assert rc == _lib.OCM_EINVAL, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    for name in ("src", "xb", "xc", "yb", "yc"):
        refused(call(**{name: None}), "null")
    refused(call(u8=None, f32=None), "null outputs")
    for batch in (0, -1, 65536):
        refused(call(batch=batch), "batch")
    for chans in (0, 2, 4):
        refused(call(chans=chans), "chans")
    for hw in ((0, 53), (37, 0), ((1 << 19) + 1, 53)):
        refused(call(src_h=hw[0], src_w=hw[1], tmp_rows=max(hw[0], 1)), "source size")
    for i in range(4):
        strides = [0, 159, 3, 1]
        strides[i] = -1
        refused(call(strides=tuple(strides)), "stride")
    for out in ((0, 24), (65536, 24), (24, 0)):
        refused(call(out_h=out[0], out_w=out[1]), "output size")
    refused(call(xk=0), "ksize")
    refused(call(yk=-1), "ksize")
    refused(call(tmp_rows=0), "tmp_rows")
    refused(call(tmp_rows=36), "tmp_rows")  # fewer rows than the source, and no rectangles
    refused(call(ws=C.c_void_p(4096 + 8)), "aligned")
    assert call(nbytes=16) == _lib.OCM_ENOMEM and call(ws=None) == _lib.OCM_ENOMEM
    assert call(nbytes=f(1, 3, 37, 24) - 1) == _lib.OCM_ENOMEM


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_python_surface_refusals():
    img = torch.zeros(9, 11, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError):  # no host fall-back
        utils.pil_resize(img, (5, 4))
    with pytest.raises(RuntimeError):
        sw_processing.prepare_slab(img, (5, 4))
    with pytest.raises(RuntimeError):
        data.resize_to_tensor(img, (8, 8))
    with pytest.raises(ValueError):
        utils.pil_resize(img.float(), (5, 4))
    with pytest.raises(ValueError):
        utils.pil_resize(img, (5, 4), resample=1)
    with pytest.raises(ValueError):
        utils.pil_resize(img, (0, 4))
    with pytest.raises(ValueError):
        utils.pil_resize(torch.zeros(9, 11, 2, dtype=torch.uint8), (5, 4))
    with pytest.raises(ValueError):
        utils.pil_resize(img, (5, 4), crop=(0, 0, 12, 9))  # wider than the image
    with pytest.raises(ValueError):
        utils.pil_resize(img, (5, 4), crop=[(0, 0, 5, 5), (0, 0, 5, 5)])  # two rectangles, one image
    with pytest.raises(ValueError):
        utils.pil_resize(img, (5, 4), hflip=[True, False])
    with pytest.raises(ValueError):
        sw_processing.prepare_slab(torch.zeros(3, 9, 11, dtype=torch.uint8), (5, 4))  # planar: not a decoded image
    with pytest.raises(ValueError):
        data.cropped_batch(torch.zeros(1, 9, 11, 3, dtype=torch.uint8), 8, crop=5)
    assert data._resize_size(100, 60, 30) == (50, 30) and data._resize_size(60, 100, 30) == (30, 50)  # torchvision's int rule
    assert data._resize_size(100, 60, (7, 9)) == (7, 9)


# ---- RandomResizedCrop.get_params ------------------------------------------------------------------------------------------------
def test_random_resized_crop_params():
    def draws(seed, n, h, w):
        g = torch.Generator().manual_seed(seed)
        return [data.random_resized_crop_params(h, w, generator=g) for _ in range(n)]

    a, b = draws(3, 50, 300, 260), draws(3, 50, 300, 260)
    assert a == b and a != draws(4, 50, 300, 260) and len(set(a)) > 40  # deterministic per generator
    for i, j, h, w in a:
        assert 0 <= i and 0 <= j and 0 < h and 0 < w and i + h <= 300 and j + w <= 260
        assert 0.67 * 300 * 260 * 0.97 <= h * w <= 300 * 260 and 0.74 <= w / h <= 1.35
    # 10 x 400: no rectangle of 67 % of the area and a ratio up to 4/3 fits the height, so the ten tries fail
    for params in draws(5, 8, 10, 400):
        assert params == (0, (400 - 13) // 2, 10, 13)
    for params in draws(5, 8, 400, 10):  # and the other way: w = 10, h = round(10 / (3/4)) = 13
        assert params == ((400 - 13) // 2, 0, 13, 10)
    g = torch.Generator().manual_seed(1)
    crops, hf, vf = data.simmim_params(64, 300, 260, g)
    assert crops.shape == (64, 4) and hf.dtype == bool and 8 < hf.sum() < 56 and 8 < vf.sum() < 56
    assert (crops[:, 0] >= 0).all() and (crops[:, 1] >= 0).all() and (crops[:, 2] <= 260).all() and (crops[:, 3] <= 300).all()
    c2, h2, v2 = data.simmim_params(64, 300, 260, torch.Generator().manual_seed(1))
    assert np.array_equal(crops, c2) and np.array_equal(hf, h2) and np.array_equal(vf, v2)


def test_mask_generator_is_the_reference_s():
    m = data.MaskGenerator(input_size=224, mask_patch_size=32, model_patch_size=16, mask_ratio=0.6)
    np.random.seed(0)
    mask = m()
    assert mask.shape == (14, 14) and mask.sum() == m.mask_count * 4 == 30 * 4 and set(np.unique(mask)) == {0, 1}
    assert np.array_equal(mask, mask[::2, ::2].repeat(2, 0).repeat(2, 1))
