"""Host side of the Chan-Vese path (kernels_levelset.hip, utils.chan_vese_level_set / chan_vese, eval.chan_vese_segment): the
numpy restatement tests/chan_vese_ref.py on its own test images, the C ABI's declarations and argument refusals, and the
refusals of the Python surface. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import chan_vese_ref as R
from vit_ocm_wmsegmentation_amd import _lib, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ocm_chan_vese_tile", "ocm_chan_vese_workspace_bytes", "ocm_op_chan_vese"]
T = 32  # the kernels' tile side (ocm_chan_vese_tile(), asserted below)


@pytest.mark.parametrize("h,w,seed", [(9, 9, 6), (37, 53, 1), (96, 96, 0), (96, 96, 2)])
def test_restatement_converges_on_blobs(h, w, seed):
    img, phi0, r = R.cached("blobs", h, w, seed)
    assert 20 < r["iters"] < 200 and len(r["phis"]) == r["iters"] + 1 and len(r["phivars"]) == r["iters"]
    assert r["phivars"][-1] <= 1e-3 < min(r["phivars"][:-1])  # the first iteration at or below tol ends the loop
    assert np.array_equal(r["phis"][0], R.checkerboard(h, w)) and r["phis"][-1] is r["phi"]
    # the segmentation separates the bright blobs from the dark ground: the two class means lie far apart
    x = R.normalize(img)
    assert 0.05 < r["mask"].mean() < 0.95
    assert abs(x[r["mask"]].mean() - x[~r["mask"]].mean()) > 0.3


@pytest.mark.parametrize("h,w", [(9, 9), (37, 53), (48, 48)])
def test_restatement_puts_the_edge_at_the_step(h, w):
    img, _, r = R.cached("step", h, w, 0)
    assert r["iters"] == 200 and r["phivars"][-1] > 1e-3  # the sharp edge keeps moving phi: the cap ends the run
    want = np.zeros((h, w), bool)
    want[:, w // 2:] = True
    assert np.array_equal(r["mask"], want)


def test_restatement_pieces():
    assert np.array_equal(R.normalize(R.flat(5, 7)), np.zeros((5, 7)))  # max == 0: no division
    x = R.normalize(np.array([[10, 20], [30, 110]], np.uint8))
    assert x.min() == 0.0 and x.max() == 1.0 and x[0, 1] == 10.0 / 100.0
    cb = R.checkerboard(11, 13)
    assert cb.dtype == np.float64 and cb[0].max() == 0.0 and cb[2, 3] == np.sin(np.pi / 5 * 2) * np.sin(np.pi / 5 * 3)
    assert np.array_equal(utils.chan_vese_checkerboard(11, 13), cb)
    # max_num_iter = 0: nothing runs
    r = R.chan_vese(R.blobs(9, 9, 6), max_num_iter=0)
    assert r["iters"] == 0 and np.array_equal(r["phi"], R.checkerboard(9, 9))
    # a Jacobi step reads only old values: the step of a transposed problem is the transposed step
    img, phi = R.normalize(R.blobs(12, 17, 3)), R.random_start(12, 17, 4)
    a = R.step(img, phi, 0.25, 1.0, 1.0, 0.5)
    b = R.step(img.T.copy(), phi.T.copy(), 0.25, 1.0, 1.0, 0.5).T
    assert np.abs(a - b).max() <= 1e-14


def test_flat_image_stays_finite():
    _, _, r = R.cached("flat", 37, 53, 0)
    assert 0 < r["iters"] < 200 and np.isfinite(r["phi"]).all()


def test_entry_points_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ocm_vit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION == 20
    assert lib.ocm_chan_vese_tile() == T
    assert "kernels_levelset.hip" in open(os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc", "Makefile")).read()


def test_workspace_sizes(lib):
    assert lib.ocm_chan_vese_workspace_bytes(3, 37, 53) >= 3 * 37 * 53 * 8 + 2 * 3 * 4 * 32 + 3 * 4
    assert lib.ocm_chan_vese_workspace_bytes(16, 384, 384) >= 16 * 384 * 384 * 8
    assert lib.ocm_chan_vese_workspace_bytes(1, 32768, 32768) >= (1 << 30) * 8
    for bad in [(0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 40000, 4), (1, 32768, 32768 + 1)]:
        assert lib.ocm_chan_vese_workspace_bytes(*bad) == 0


def test_argument_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    p = C.c_void_p(4096)  # non-null, never touched
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def call(image=p, phi=p, mask=p, iters=p, batch=1, h=4, w=4, mu=0.25, l1=1.0, l2=1.0, tol=1e-3, it=200, dt=0.5, ws=p,
             nbytes=big):
        return lib.ocm_op_chan_vese(image, phi, mask, iters, batch, h, w, mu, l1, l2, tol, it, dt, ws, nbytes, None)

    def refused(rc, word):
        assert rc == _lib.OCM_EINVAL, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    for name in ("image", "phi", "mask", "iters"):
        refused(call(**{name: None}), "null")
    for batch in (0, -1, 65536):
        refused(call(batch=batch), "batch")
    for h, w in ((0, 4), (4, 0), (-4, 4), (32769, 4), (4, 32769), (32768, 32768 + 1)):
        refused(call(h=h, w=w), "image")
    for it in (-1, 10001):
        refused(call(it=it), "max_num_iter")
    for bad in (nan, inf, -inf, -1e-9):
        refused(call(mu=bad), "mu")
        refused(call(dt=bad), "dt")
        refused(call(tol=bad), "tol")
    refused(call(l1=nan), "lambda")
    refused(call(l2=inf), "lambda")
    assert call(nbytes=16) == _lib.OCM_ENOMEM
    assert call(ws=None) == _lib.OCM_ENOMEM
    assert call(nbytes=lib.ocm_chan_vese_workspace_bytes(1, 4, 4) - 1) == _lib.OCM_ENOMEM


def test_python_surface_refusals():
    from vit_ocm_wmsegmentation_amd import eval as E
    cpu = torch.zeros(8, 8, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        utils.chan_vese(cpu, torch.zeros(8, 8), save=True)
    with pytest.raises(RuntimeError):  # no host fall-back
        utils.chan_vese_level_set(cpu)
    with pytest.raises(RuntimeError):
        utils.chan_vese(cpu, torch.zeros(8, 8))
    with pytest.raises(ValueError):
        E.chan_vese_segment(None, torch.zeros(1, 3, 16, 16), method="otsu")
    with pytest.raises(ValueError):
        E.chan_vese_segment(None, torch.zeros(1, 3, 16, 16), method="chan-vese", median_filter=0)
    for method in E.CHAN_VESE:  # segment_images keeps refusing them, and now says where they run
        with pytest.raises(ValueError, match="chan_vese_segment"):
            E.segment_images(None, torch.zeros(1, 3, 16, 16), method=method)
    with pytest.raises(ValueError):
        E.segment_images(None, torch.zeros(1, 3, 16, 16), method="k-means")
