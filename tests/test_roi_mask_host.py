"""Host side of the ROI-guided SimMIM masks (kernels_roi.hip, data.roi_mask / data.SimMIMTransform): the numpy restatement
tests/roi_mask_ref.py against the live libraries skimage 0.19.3 is made of — scipy.ndimage's zoom, dilation, erosion and label,
Pillow's convert('L'), torch's mul(255).byte(), numpy's float64 -> uint8 cast —, what the image families promise, the C ABI's
declarations and refusals, and the transform's host half. scikit-image itself is not installed: parity with it is unpinned.
No GPU needed."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import morph_ref as M
from tests import roi_mask_ref as R
from vit_ocm_wmsegmentation_amd import _lib, data, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32  # ocm_label8_tile(), asserted below
EXTRA_PAIRS = [(224, 14), (320, 40), (192, 48), (384, 48), (512, 64)]
SHORT_FORMULA_FAILS = [(30, 11), (52, 23), (2, 49), (12, 94)]  # named in DESIGN 3.32: floor((i + 0.5) * in / out) is wrong here


def _zoom_index(n_in, n_out):
    ndi = pytest.importorskip("scipy.ndimage")
    got = ndi.zoom(np.arange(n_in, dtype=np.float64), n_out / n_in, order=0, mode="mirror", grid_mode=True)
    assert got.shape == (n_out,)
    return got.astype(np.int32)


def test_sample_index_is_scipy_zoom():
    pairs = [(i, o) for i in range(1, 65) for o in range(1, 65)] + EXTRA_PAIRS + SHORT_FORMULA_FAILS
    for n_in, n_out in pairs:
        want = _zoom_index(n_in, n_out)
        got = utils.roi_sample_index(n_in, n_out)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n_in, n_out)
        assert np.array_equal(R.sample_index(n_in, n_out), want), (n_in, n_out)


@pytest.mark.parametrize("n_in,n_out", SHORT_FORMULA_FAILS)
def test_short_formula_fails_where_the_issue_says(n_in, n_out):
    want = _zoom_index(n_in, n_out)
    assert not np.array_equal(R.short_sample_index(n_in, n_out), want)
    assert np.array_equal(utils.roi_sample_index(n_in, n_out), want)


def test_sample_index_refuses_empty_axes():
    for bad in [(0, 4), (4, 0), (-1, 3)]:
        with pytest.raises(ValueError):
            utils.roi_sample_index(*bad)


def _pil_gray(img):
    Image = pytest.importorskip("PIL.Image")
    t = torch.from_numpy(np.array(img, np.float32))
    u8 = t.mul(255).byte().permute(1, 2, 0).contiguous().numpy()
    return np.asarray(Image.fromarray(u8 if u8.shape[2] == 3 else u8[:, :, 0]).convert("L"))


def test_gray_is_pillow_on_torch_bytes():
    rs = np.random.RandomState(5)
    rand = rs.uniform(0, 1, size=(3, 41, 29)).astype(np.float32)
    assert np.array_equal(R.gray_u8(rand), _pil_gray(rand))
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0))
    near = np.stack([np.nextafter(k, np.float32(0)), k, np.nextafter(k, np.float32(2))]).clip(0, 1).astype(np.float32)  # (3, 256)
    img = np.stack([near, near[::-1], near[[1, 2, 0]]])  # three channels, each value within one ulp of some k / 255
    assert np.array_equal(R.gray_u8(img), _pil_gray(img))
    one = near[None]
    assert np.array_equal(R.gray_u8(one), _pil_gray(one))
    assert np.array_equal(R.gray_u8(rand), M.gray_u8(rand))  # the arithmetic ocm_op_image_to_gray_u8 is tested against
    v = R.below_eleven()
    assert R.gray_u8(np.full((3, 1, 1), v, np.float32))[0, 0] == 10
    assert R.gray_u8(np.full((3, 1, 1), np.nextafter(v, np.float32(1)), np.float32))[0, 0] == 11
    assert R.gray_u8(R.from_u8(np.array(R.L10, np.uint8).reshape(3, 1, 1)))[0, 0] == 10
    assert R.gray_u8(R.from_u8(np.array(R.L11, np.uint8).reshape(3, 1, 1)))[0, 0] == 11
    u = rs.randint(0, 256, size=(3, 9, 9)).astype(np.uint8)
    assert np.array_equal((R.from_u8(u) * np.float32(255)).astype(np.int32), u)


def test_wrap_is_numpy_cast():
    labels = np.arange(0, 1025)
    with np.errstate(all="ignore"):
        want = np.float64(labels).astype(np.uint8) != 0
    assert np.array_equal(R.wrap_nonzero(labels), want)
    assert not want[256] and not want[512] and want[257] and want[784] and not want[0]


def test_remove_small_labels_is_the_total_count_rule():
    ar = np.zeros((10, 10), np.uint8)
    ar[::3, ::3] = 255  # 16 isolated pixels
    assert not R.remove_small_labels(ar, 20).any()
    ar[1, 1] = ar[1, 4] = ar[1, 7] = ar[4, 1] = 255  # 20, still one pixel per component
    assert np.array_equal(R.remove_small_labels(ar, 20), ar)


def _all_images():
    for h, w, gh, gw in R.geometries(T):
        for name, (img, _) in R.families(h, w, gh, gw).items():
            yield f"{name} {h}x{w}", img
    yield "wrap", R.wrap_case()[0]


def test_closing_and_labelling_are_scipy_on_the_test_images():
    ndi = pytest.importorskip("scipy.ndimage")
    for what, img in _all_images():
        b = R.gray_u8(img) > 10
        dil = ndi.binary_dilation(b, M.DISK2)
        assert np.array_equal(M.dilate(b, M.DISK2, 0), dil), what
        closed = ndi.binary_erosion(dil, M.DISK2, border_value=1)
        assert np.array_equal(M.erode(dil, M.DISK2, 1), closed) and np.array_equal(M.closing(b), closed), what
        want, n = ndi.label(closed, structure=np.ones((3, 3)))
        labels, got_n = M.label8(closed)
        assert got_n == n and np.array_equal(labels, want), what


def test_restatement_is_the_chain_on_live_libraries():
    """Steps 2-6 once more with scipy's zoom on the float64 label image and numpy's own cast, as the reference's lines read."""
    ndi = pytest.importorskip("scipy.ndimage")
    for h, w, gh, gw in R.geometries(T):
        for name, (img, mask) in R.families(h, w, gh, gw).items():
            binary = _pil_gray(img).copy()
            binary[binary > 10] = 255
            binary[binary <= 10] = 0
            if np.count_nonzero(binary) < 20:
                binary[:] = 0
            closed = ndi.binary_erosion(ndi.binary_dilation(binary, M.DISK2), M.DISK2, border_value=1)
            rois = ndi.label(closed, structure=np.ones((3, 3)))[0]
            rois = ndi.zoom(rois.astype(np.float64), (gh / h, gw / w), order=0, mode="mirror", grid_mode=True)
            assert rois.shape == (gh, gw)
            rois = rois.astype(np.uint8)
            rois[rois != 0] = 1
            new = mask * rois
            want = new if np.sum(new) != 0 else mask
            got, used = R.reference(h, w, gh, gw)[name]
            assert np.array_equal(got, want) and used == bool(np.sum(new) != 0), (name, h, w)


def test_families_hold_what_they_promise():
    for h, w, gh, gw in R.geometries(T):
        fam, ref = R.families(h, w, gh, gw), R.reference(h, w, gh, gw)
        ri, ci = R.sample_index(h, gh), R.sample_index(w, gw)
        assert {"mixed", "dark", "count19", "count20", "disjoint", "grey_a", "grey_b", "gap"} <= set(fam), (h, w, set(fam))
        white = {k: int((R.gray_u8(img) > 10).sum()) for k, (img, _) in fam.items()}
        new, used = ref["mixed"]
        assert used and new.sum() and not np.array_equal(new, fam["mixed"][1])
        assert white["dark"] == 0 and ref["dark"][1] is False and np.array_equal(ref["dark"][0], fam["dark"][1])
        # the total-count rule: single-pixel components, one of them on a sample point
        for n in (19, 20):
            b = R.gray_u8(fam[f"count{n}"][0]) > 10
            assert white[f"count{n}"] == n and M.label8(b)[1] == n and b[ri[0], ci[0]]
        assert ref["count19"][1] is False and ref["count19"][0].all()
        assert ref["count20"][1] is True and ref["count20"][0][0, 0] == 1 and not ref["count20"][0].all()
        assert white["disjoint"] >= 20 and ref["disjoint"][1] is False and np.array_equal(ref["disjoint"][0], fam["disjoint"][1])
        # grey levels: (10,10,10) and the L = 10 triple are background, (11,11,11) is ROI; L = 11, byte 10 and byte 11 likewise
        pts = R.spaced_points(h, w, gh, gw)
        a, b = ref["grey_a"][0], ref["grey_b"][0]
        assert ref["grey_a"][1] and ref["grey_b"][1] and white["grey_a"] >= 20 and white["grey_b"] >= 20
        assert (a[pts[0][2:]], a[pts[1][2:]], a[pts[2][2:]], a[pts[3][2:]]) == (0, 1, 0, 1), (h, w)
        assert (b[pts[0][2:]], b[pts[1][2:]], b[pts[2][2:]], b[pts[3][2:]]) == (1, 0, 1, 1), (h, w)
        # the gap is ROI only because of the closing
        g = R.gray_u8(fam["gap"][0]) > 10
        assert white["gap"] >= 20 and ref["gap"][1]
        assert np.count_nonzero(ref["gap"][0]) > np.count_nonzero(g[np.ix_(ri, ci)])
    # every pixel sampled: cells on columns 0 and 1 are ROI only because the erosion counts the outside as set
    fam, ref = R.families(64, 64, 64, 64), R.reference(64, 64, 64, 64)
    g = R.gray_u8(fam["edge"][0]) > 10
    border0 = M.erode(M.dilate(g, M.DISK2, 0), M.DISK2, 0)
    assert ref["edge"][0][10:50, 0].all() and ref["edge"][0][10:50, 1].all() and not border0[:, 0].any()
    assert "edge" in R.families(48, 48, 12, 12) and "edge" in R.families(40, 56, 5, 8)
    # 256 components: cell (15, 15) reads label 256 and comes out 0
    img, m, (new, used) = R.wrap_case()
    closed = M.closing(R.gray_u8(img) > 10)
    assert np.array_equal(closed, R.gray_u8(img) > 10) and M.label8(closed)[1] == 256
    assert used and new[15, 15] == 0 and new.sum() == 255


def test_entry_points_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ocm_vit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in ("ocm_op_roi_threshold", "ocm_op_roi_apply"):
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert lib.ocm_label8_tile() == T
    assert "kernels_roi.hip" in open(os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc", "Makefile")).read()


def test_argument_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced. The index tables
    are device memory, so their entries are not checked on the host: the kernel reads an entry outside the image as background."""
    p, q = C.c_void_p(4096), C.c_void_p(8192)
    E = _lib.OCM_EINVAL

    def refused(rc, word):
        assert rc == E, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    th = lib.ocm_op_roi_threshold
    refused(th(p, 48, 16, 3, 0, 4, 4, 10, p, p, None), "batch")
    refused(th(p, 48, 16, 2, 1, 4, 4, 10, p, p, None), "chans")
    refused(th(None, 48, 16, 3, 1, 4, 4, 10, p, p, None), "null")
    refused(th(p, 48, 16, 3, 1, 4, 4, 10, None, p, None), "null")
    refused(th(p, 48, 16, 3, 1, 4, 4, 10, p, None, None), "null")
    refused(th(p, 48, 16, 3, 1, 0, 4, 10, p, p, None), "image")
    refused(th(p, 48, 16, 3, 1, 4, 4, 256, p, p, None), "level")
    refused(th(p, 48, 16, 3, 1, 4, 4, -1, p, p, None), "level")
    refused(th(p, 48, 15, 3, 1, 4, 4, 10, p, p, None), "stride")
    refused(th(p, 15, 16, 3, 2, 4, 4, 10, p, p, None), "stride")
    ap = lib.ocm_op_roi_apply
    refused(ap(p, p, p, p, 20, p, 8, q, p, 0, 4, 4, 2, 2, None), "batch")
    refused(ap(p, p, p, p, 20, p, 8, q, p, 1, 4, 4, 0, 2, None), "grid")
    refused(ap(p, p, p, p, 20, p, 8, q, p, 1, 4, 4, 2, 0, None), "grid")
    refused(ap(p, p, p, p, 20, p, 8, q, p, 1, 4, -4, 2, 2, None), "image")
    refused(ap(p, p, p, p, -1, p, 8, q, p, 1, 4, 4, 2, 2, None), "min_size")
    refused(ap(p, p, p, p, 20, p, 4, q, p, 1, 4, 4, 2, 2, None), "mask_bytes")
    refused(ap(p, p, p, p, 20, p, 8, p, p, 1, 4, 4, 2, 2, None), "aliased")
    for k in (0, 1, 2, 3, 5, 7, 8):
        args = [p, p, p, p, 20, p, 8, q, p, 1, 4, 4, 2, 2, None]
        args[k] = None
        refused(ap(*args), "null")


def _args(img_size, mask_patch, patch, ratio, roi):
    return SimpleNamespace(DATA=SimpleNamespace(IMG_SIZE=img_size, MASK_PATCH_SIZE=mask_patch, MASK_RATIO=ratio),
                           MODEL=SimpleNamespace(PATCH_SIZE=patch), roi_masking=roi)


@pytest.mark.parametrize("img_size,mask_patch,patch,ratio,grid,masked", [
    (192, 32, 4, 0.6, 48, 22 * 64), (224, 32, 16, 0.6, 14, 30 * 4), (320, 8, 8, 0.3, 40, 480), (320, 16, 8, 0.4, 40, 160 * 4)])
def test_transform_without_a_device(img_size, mask_patch, patch, ratio, grid, masked):
    """G and the number of masked cells are the reference MaskGenerator's: ceil((S / mask_patch)^2 * ratio) cells of
    (mask_patch / patch)^2 patches each (data.py:163-186)."""
    t = data.SimMIMTransform(_args(img_size, mask_patch, patch, ratio, True))
    assert t.roi_masking is True and t.image_size == img_size
    np.random.seed(3)
    m = t.mask_generator()
    assert m.shape == (grid, grid) and int(m.sum()) == masked and set(np.unique(m)) <= {0, 1}
    state = np.random.get_state()[1].copy()
    with pytest.raises(RuntimeError):  # no host fall-back, and no draw is spent on the refusal
        t(torch.zeros((2, 40, 40, 3), dtype=torch.uint8))
    assert np.array_equal(np.random.get_state()[1], state)


def test_roi_mask_refuses_cpu_tensors():
    with pytest.raises(RuntimeError):
        data.roi_mask(torch.zeros(1, 3, 16, 16), torch.ones(1, 2, 2, dtype=torch.int64))
