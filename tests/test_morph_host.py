"""Host side of the region-query chain (kernels_morph.hip, utils.yen_threshold / get_ROIs / morphology_cleaning): the
pure-numpy reference tests/morph_ref.py against live scipy.ndimage on every input family of the device tests, the Yen
level against a brute-force evaluation of its criterion, the C ABI's declarations and argument refusals. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import morph_ref as R
from vit_ocm_wmsegmentation_amd import _lib, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ocm_op_mask_ge_u8", "ocm_label8_tile", "ocm_label8_workspace_bytes", "ocm_op_label8", "ocm_op_region_stats",
               "ocm_remove_small_objects_workspace_bytes", "ocm_op_remove_small_objects", "ocm_op_binary_morph",
               "ocm_op_query_mean"]
T = 32  # the labelling tile side (ocm_label8_tile(), asserted below)


@pytest.mark.parametrize("h,w", R.sizes(T) + [(64, 96)])
def test_reference_matches_scipy(h, w):
    ndi = pytest.importorskip("scipy.ndimage")
    s8 = np.ones((3, 3), bool)
    for name, m in R.families(h, w, T).items():
        labels, n = R.label8(m)
        want, wn = ndi.label(m, structure=s8)
        assert n == wn and np.array_equal(labels, want), name
        assert np.array_equal(R.dilate(m, R.DISK2, 0), ndi.binary_dilation(m, R.DISK2)), name
        assert np.array_equal(R.erode(m, R.DISK2, 1), ndi.binary_erosion(m, R.DISK2, border_value=1)), name
        assert np.array_equal(R.erode(m, R.DISK2, 0), ndi.binary_erosion(m, R.DISK2)), name
        closed = ndi.binary_erosion(ndi.binary_dilation(m, R.DISK2), R.DISK2, border_value=1)
        assert np.array_equal(R.closing(m), closed), name
        sizes = np.bincount(want.ravel(), minlength=wn + 1)
        keep = sizes >= 20
        keep[0] = False
        assert np.array_equal(R.remove_small_objects(m, 20), keep[want]), name
        area, sr, sc, bbox = R.region_sums(labels, max(n, 1))
        if n:
            idx = np.arange(1, n + 1)
            assert np.array_equal(area[:n], ndi.sum(m, want, idx).astype(np.int64)), name
            com = np.array(ndi.center_of_mass(m, want, idx))
            np.testing.assert_allclose(np.stack([sr[:n] / area[:n], sc[:n] / area[:n]], 1), com, rtol=1e-12, err_msg=name)
            for i, sl in enumerate(ndi.find_objects(want)):
                assert tuple(bbox[i]) == (sl[0].start, sl[1].start, sl[0].stop, sl[1].stop), name


def test_reference_families_hold_what_they_promise():
    f = R.families(2 * T + 3, 3 * T + 1, T)
    ref = R.reference(2 * T + 3, 3 * T + 1, T)
    assert ref["checkerboard"]["n"] == 1 and ref["serpentine"]["n"] == 1 and ref["full"]["n"] == 1 and ref["empty"]["n"] == 0
    assert ref["isolated"]["n"] == ((2 * T + 4) // 2) * ((3 * T + 2) // 2)
    assert ref["u_shape"]["n"] == 2 and ref["u_shape"]["labels"][0, 3 * T - 1] == 1  # the right arm starts first and wins
    assert ref["u_shape"]["labels"][2, 1] == 1
    d = ref["diagonal_corner"]["labels"]
    assert d[T - 1, T - 1] == d[T, T] != 0 and d[T - 1, 2 * T] == d[T, 2 * T - 1] != 0  # joined across the tile corners only
    areas = sorted(ref["sizes"]["stats"][0].tolist())
    assert areas.count(19) >= 3 and areas.count(20) >= 3 and areas.count(9) >= 2 and areas.count(10) >= 2
    assert ref["sizes"]["removed"].sum() == 20 * areas.count(20)
    kept = [a for a in R.region_sums(ref["sizes"]["rois"], ref["sizes"]["rois_n"])[0]]
    assert len(ref["sizes"]["points"]) == sum(a >= 10 for a in kept)
    e = f["edges"]
    assert e[0].any() and e[-1].any() and e[:, 0].any() and e[:, -1].any()
    assert not np.array_equal(ref["edges"]["closed"], R.erode(R.dilate(e), R.DISK2, 0))  # the erosion border matters


def test_asymmetric_footprint_conventions_match_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    fp = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0]], np.uint8)
    m = R.gaussian_noise(23, 31, 5)
    for border in (0, 1):
        assert np.array_equal(R.dilate(m, fp, border), ndi.binary_dilation(m, fp, border_value=border))
        assert np.array_equal(R.erode(m, fp, border), ndi.binary_erosion(m, fp, border_value=border))


def _bimodal_hist():
    rs = np.random.RandomState(3)
    v = np.concatenate([rs.normal(60, 12, 5000), rs.normal(170, 20, 3000)]).clip(7, 243).astype(np.uint8)
    return np.bincount(v, minlength=256)


def test_yen_level_is_the_brute_force_maximum():
    hist = _bimodal_hist()
    nz = np.nonzero(hist)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    pmf = (hist[lo:hi + 1] / hist.sum()).tolist()
    crit = [R.yen_criterion(pmf, t) for t in range(hi - lo)]
    best = lo + int(np.argmax(crit))
    assert 60 < best < 170
    margin = np.sort(crit)[-1] - np.sort(crit)[-2]
    assert margin > 1e-9  # the maximum is not a rounding tie between the two evaluations
    assert utils.skimage_yen_from_hist(hist) == best == R.yen_from_hist(hist)
    assert utils.skimage_yen_from_hist(torch.from_numpy(hist)) == best
    flat = np.zeros(256, np.int64)
    flat[93] = 4096
    assert utils.skimage_yen_from_hist(flat) == 93 == R.yen_from_hist(flat)
    with pytest.raises(ValueError):
        utils.skimage_yen_from_hist(np.zeros(256, np.int64))


def test_query_mean_reference_is_numpy_mean():
    rs = np.random.RandomState(11)
    rows = rs.standard_normal((2, 6, 5, 49)).astype(np.float32)
    sel = [[3, 0, 3, 4, 1, 1, 2, 0, 4, 3, 2], []]
    got = R.query_mean(rows, sel)
    maps = [np.mean(rows[0, :, q], axis=0) for q in sel[0]]
    assert maps[0].dtype == np.float32
    assert np.array_equal(got[0], np.mean(maps, axis=0)) and np.isnan(got[1]).all()


def test_entry_points_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ocm_vit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert "#define OCM_ABI_VERSION 20\n" in open(os.path.join(ROOT, "include", "ocm_vit.h")).read()
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION == 20
    assert lib.ocm_label8_tile() == T
    assert "kernels_morph.hip" in open(os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc", "Makefile")).read()


def test_workspace_sizes(lib):
    assert lib.ocm_label8_workspace_bytes(3, 37, 53) >= 3 * 37 * 53 * 4 + 3 * 2 * 4
    assert lib.ocm_label8_workspace_bytes(1, 4096, 4096) >= 4096 * 4096 * 4
    assert lib.ocm_remove_small_objects_workspace_bytes(2, 10, 10) >= 2 * 2 * 100 * 4
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 40000, 4), (1, 32768, 32768 + 1)]:
        assert lib.ocm_label8_workspace_bytes(*bad) == 0 and lib.ocm_remove_small_objects_workspace_bytes(*bad) == 0


def test_argument_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    p = C.c_void_p(4096)  # non-null, never touched
    E = _lib.OCM_EINVAL
    big = 1 << 40

    def refused(rc, word):
        assert rc == E, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    refused(lib.ocm_op_label8(None, p, p, 1, 4, 4, p, big, None), "null")
    refused(lib.ocm_op_label8(p, p, p, 0, 4, 4, p, big, None), "batch")
    refused(lib.ocm_op_label8(p, p, p, 70000, 4, 4, p, big, None), "batch")
    refused(lib.ocm_op_label8(p, p, p, 1, 0, 4, p, big, None), "image")
    refused(lib.ocm_op_label8(p, p, p, 1, 32768, 32769, p, big, None), "image")
    assert lib.ocm_op_label8(p, p, p, 1, 4, 4, p, 16, None) == _lib.OCM_ENOMEM
    assert lib.ocm_op_label8(p, p, p, 1, 4, 4, None, big, None) == _lib.OCM_ENOMEM
    refused(lib.ocm_op_remove_small_objects(p, None, 1, 4, 4, 20, p, big, None), "null")
    refused(lib.ocm_op_remove_small_objects(p, p, 1, 4, -4, 20, p, big, None), "image")
    refused(lib.ocm_op_remove_small_objects(p, p, 1, 4, 4, -1, p, big, None), "min_size")
    assert lib.ocm_op_remove_small_objects(p, p, 1, 4, 4, 20, p, 8, None) == _lib.OCM_ENOMEM
    refused(lib.ocm_op_region_stats(p, 1, 4, 4, 3, p, p, None, p, None), "null")
    refused(lib.ocm_op_region_stats(p, 1, 4, 4, 0, p, p, p, p, None), "max_regions")
    refused(lib.ocm_op_region_stats(p, 0, 4, 4, 3, p, p, p, p, None), "batch")
    q = C.c_void_p(8192)
    refused(lib.ocm_op_binary_morph(p, p, 1, 4, 4, 1, 1, 0, 0, None), "aliased")
    refused(lib.ocm_op_binary_morph(p, q, 1, 4, 4, 0x1FF, 4, 0, 0, None), "size")
    refused(lib.ocm_op_binary_morph(p, q, 1, 4, 4, 0x1FF, 9, 0, 0, None), "size")
    refused(lib.ocm_op_binary_morph(p, q, 1, 4, 4, 0x3FF, 3, 0, 0, None), "beyond")
    refused(lib.ocm_op_binary_morph(p, q, 1, 4, 4, 0, 3, 0, 0, None), "empty")
    refused(lib.ocm_op_binary_morph(p, q, 1, 4, 4, 0x1FF, 3, 2, 0, None), "op")
    refused(lib.ocm_op_binary_morph(p, q, 1, 4, 4, 0x1FF, 3, 1, 2, None), "border")
    refused(lib.ocm_op_mask_ge_u8(p, None, 16, 3, None), "null")
    refused(lib.ocm_op_mask_ge_u8(p, q, 0, 3, None), "count")
    refused(lib.ocm_op_query_mean(p, p, None, p, 1, 3, 1, 4, 1, None), "null")
    refused(lib.ocm_op_query_mean(p, None, p, p, 1, 3, 1, 4, 1, None), "null")
    refused(lib.ocm_op_query_mean(p, p, p, p, 1, 0, 1, 4, 1, None), "shape")
    refused(lib.ocm_op_query_mean(p, p, p, p, 1, 3, 1, 4, -1, None), "shape")


def test_python_surface_refusals():
    cpu_mask = torch.zeros(8, 8, dtype=torch.bool)
    for fn in (utils.yen_threshold, utils.morphology_cleaning):
        with pytest.raises(NotImplementedError):
            fn(cpu_mask, save=True)
    for fn in (utils.label_regions, utils.get_ROIs, utils.morphology_cleaning, utils.remove_small_objects,
               utils.binary_closing, utils.yen_threshold):
        with pytest.raises(RuntimeError):  # no host fall-back
            fn(cpu_mask)
    assert utils.footprint_bits(R.DISK2) == (5, sum(1 << i for i, v in enumerate(R.DISK2.ravel()) if v))
    assert utils.footprint_bits(utils.DISK2)[1] == utils.footprint_bits(R.DISK2)[1]
    for bad in (np.ones((2, 2)), np.ones((9, 9)), np.ones((3, 5)), np.ones(3)):
        with pytest.raises(ValueError):
            utils.footprint_bits(bad)
    from vit_ocm_wmsegmentation_amd import analyse_attention
    with pytest.raises(RuntimeError):
        analyse_attention.region_query_points(torch.zeros(1, 3, 16, 16), 8)
    with pytest.raises(ValueError):
        analyse_attention.region_queried_attention(None, torch.zeros(1, 3, 16, 16), median_filter=0)
