"""Host side of the pixel k-means path (kernels_kmeans_px.hip, utils.cv_rng_uniform / kmeans_pixels / kmeans,
eval.kmeans_pixels_segment): cv::RNG against Python big integers, the C ABI's declarations and argument refusals, the refusals of
the Python surface, and the numpy restatement tests/kmeans_px_ref.py on its own inputs and against live sklearn. No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import kmeans_px_ref as R
from vit_ocm_wmsegmentation_amd import _lib, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc")
NEW_SYMBOLS = ["ocm_cv_rng_uniform", "ocm_kmeans_px_workspace_bytes", "ocm_op_kmeans_px"]
T = 512  # the kernels' workgroup size, which the device tests choose their shapes by (asserted below)


# ---- cv::RNG ---------------------------------------------------------------------------------------------------------------------
def test_rng_matches_big_integer_arithmetic():
    want, state = R.rng_uniform(0xffffffff, 60)
    assert state == 0xe84cc2be49a1a3fb  # the check value of the arithmetic: 60 draws, one call of cv2.kmeans with 10 attempts
    got, got_state = utils.cv_rng_uniform(0xffffffff, 60)
    assert got.dtype == np.float32 and got_state == state and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert 0.0 <= got.min() and got.max() <= 1.0
    for seed in (1, 0x123456789abcdef0, (1 << 64) - 1, 0xffffffff00000000):
        w, ws = R.rng_uniform(seed, 37)
        g, gs = utils.cv_rng_uniform(seed, 37)
        assert gs == ws and np.array_equal(g.view(np.uint32), w.view(np.uint32)), hex(seed)


def test_rng_seed_zero_and_chaining():
    a, sa = utils.cv_rng_uniform(0, 24)
    b, sb = utils.cv_rng_uniform(0xffffffff, 24)
    assert sa == sb and np.array_equal(a, b)  # a seed of 0 stands for 0xffffffff
    first, mid = utils.cv_rng_uniform(0xffffffff, 10)
    second, end = utils.cv_rng_uniform(mid, 14)
    assert end == sb and np.array_equal(np.concatenate([first, second]), b)  # two calls chained equal one call
    none, same = utils.cv_rng_uniform(mid, 0)
    assert none.size == 0 and same == mid
    assert utils.CV_RNG_START == R.RNG_START == 0xffffffff


def test_rng_refusals(lib):
    st = C.c_uint64(1)
    out = np.empty(4, np.float32)
    assert lib.ocm_cv_rng_uniform(None, out.ctypes.data_as(C.c_void_p), 4) == _lib.OCM_EINVAL
    assert lib.ocm_cv_rng_uniform(C.byref(st), None, 4) == _lib.OCM_EINVAL
    assert lib.ocm_cv_rng_uniform(C.byref(st), out.ctypes.data_as(C.c_void_p), -1) == _lib.OCM_EINVAL
    assert st.value == 1


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ocm_vit.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert "kernels_kmeans_px.hip" in open(os.path.join(CSRC, "Makefile")).read()
    src = open(os.path.join(CSRC, "kernels_kmeans_px.hip")).read()
    assert f"constexpr int KP_THREADS = {T};" in src and "#pragma clang fp contract(off)" in src


def test_otsu_statements_are_shared(lib):
    """ocm_otsu_threshold and the finishing kernel take the level from one function (otsu.h); the host results are the ones the
    restated getThreshVal_Otsu_8u gives."""
    assert "ocm_otsu_level" in open(os.path.join(CSRC, "engine.hip")).read()
    assert "ocm_otsu_level" in open(os.path.join(CSRC, "kernels_kmeans_px.hip")).read()

    def level(hist):
        h = np.asarray(hist, np.uint64)
        return lib.ocm_otsu_threshold(h.ctypes.data_as(C.POINTER(C.c_uint64)), int(h.sum()))

    def otsu_numpy(hist):
        count = float(np.sum(hist))
        scale = 1.0 / count
        mu = 0.0
        for i in range(256):
            mu += i * float(hist[i])
        mu *= scale
        mu1 = q1 = max_sigma = 0.0
        max_val = 0
        for i in range(256):
            p_i = float(hist[i]) * scale
            mu1 *= q1
            q1 += p_i
            q2 = 1.0 - q1
            if min(q1, q2) < 1.1920928955078125e-07 or max(q1, q2) > 1.0 - 1.1920928955078125e-07:
                continue
            mu1 = (mu1 + i * p_i) / q1
            mu2 = (mu - q1 * mu1) / q2
            sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
            if sigma > max_sigma:
                max_sigma, max_val = sigma, i
        return max_val

    rs = np.random.RandomState(0)
    hists = [rs.randint(0, 1000, 256), np.bincount(R.painting(*_painted(R.plateaus(300, 1))), minlength=256)]
    one = np.zeros(256, np.int64)
    one[200] = 3087
    hists.append(one)  # a constant painting: no split, level 0
    for h in hists:
        assert level(h) == otsu_numpy(h)
    assert level(one) == 0
    assert lib.ocm_otsu_threshold(None, 5) < 0 and level(np.zeros(256, np.int64)) < 0


def _painted(pixels, attempts=3):
    r = R.kmeans(pixels, R.uniforms_for(1, attempts)[0][0])
    return r["labels"], r["centers"]


def test_workspace_sizes(lib):
    f = lib.ocm_kmeans_px_workspace_bytes
    assert f(1, 2, 1) >= 16 + 32
    assert f(3, 4 * T + 5, 10) >= 3 * 10 * (4 * T + 5)
    assert f(16, 384 * 384 // 3, 10) >= 16 * 10 * 49152
    assert f(65535, 1 << 24, 32) >= 65535 * 32 * (1 << 24)
    for bad in [(0, 4, 1), (65536, 4, 1), (1, 1, 1), (1, 0, 1), (1, -3, 1), (1, (1 << 24) + 1, 1), (1, 4, 0), (1, 4, 33)]:
        assert f(*bad) == 0, bad


def test_argument_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    p = C.c_void_p(4096)  # non-null, 16-byte aligned, never touched
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def call(pixels=p, problems=1, samples=4, uniforms=p, attempts=10, max_iter=10, eps=1.0, labels=p, centers=p, compactness=p,
             iters=p, best=p, mask=p, ws=p, nbytes=big):
        return lib.ocm_op_kmeans_px(pixels, problems, samples, uniforms, attempts, max_iter, eps, labels, centers, compactness,
                                    iters, best, mask, ws, nbytes, None)

    def refused(rc, word):
        assert rc == _lib.OCM_EINVAL, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    for name in ("pixels", "uniforms", "labels", "centers", "compactness", "iters", "best", "mask"):
        refused(call(**{name: None}), "null")
    for problems in (0, -1, 65536):
        refused(call(problems=problems), "problems")
    for samples in (1, 0, -6, (1 << 24) + 1, 1 << 40):
        refused(call(samples=samples), "samples")
    for attempts in (0, -1, 33):
        refused(call(attempts=attempts), "attempts")
    for it in (0, -1, 1001):
        refused(call(max_iter=it), "max_iter")
    for bad in (nan, inf, -inf, -1e-9):
        refused(call(eps=bad), "eps")
    refused(call(ws=C.c_void_p(4096 + 8)), "aligned")
    assert call(nbytes=16) == _lib.OCM_ENOMEM
    assert call(ws=None) == _lib.OCM_ENOMEM
    assert call(nbytes=lib.ocm_kmeans_px_workspace_bytes(1, 4, 10) - 1) == _lib.OCM_ENOMEM


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
class _Untouchable:
    """A model whose every use fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the model was used ({name}) before the pixel count was checked")


def test_pixel_counts_that_are_no_multiple_of_three_are_refused_first():
    from vit_ocm_wmsegmentation_amd import eval as E
    model = _Untouchable()
    for method in E.KMEANS_PIXELS:
        for shape in ((1, 3, 16, 16), (2, 3, 224, 224), (1, 4, 3, 8, 8)):  # 256, 50 176 and 256 pixels: not multiples of 3
            x = torch.zeros(shape)
            with pytest.raises(ValueError, match="triples"):
                E.kmeans_pixels_segment(model, x, method=method)
            side = shape[-1] * (2 if len(shape) == 5 else 1)
            with pytest.raises(ValueError, match="triples"):
                E.score_images(model, x, torch.zeros(shape[0], side, side), method=method)
            with pytest.raises(ValueError, match="triples"):
                E.validate(model, [(x, torch.zeros(shape[0], side, side))], method=method)
    with pytest.raises(ValueError, match="triples"):
        utils.kmeans_pixels(torch.zeros(16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="triples"):
        utils.kmeans(torch.zeros(16, 16, dtype=torch.uint8), torch.zeros(16, 16))


def test_python_surface_refusals():
    from vit_ocm_wmsegmentation_amd import eval as E
    cpu = torch.zeros(9, 9, dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        utils.kmeans(cpu, torch.zeros(9, 9), save=True)
    with pytest.raises(RuntimeError):  # no host fall-back
        utils.kmeans_pixels(cpu)
    with pytest.raises(RuntimeError):
        utils.kmeans(cpu, torch.zeros(9, 9))
    with pytest.raises(ValueError):
        E.kmeans_pixels_segment(None, torch.zeros(1, 3, 48, 48), method="otsu")
    with pytest.raises(ValueError):
        E.kmeans_pixels_segment(None, torch.zeros(1, 3, 48, 48), method="k-means", median_filter=0)
    for method in E.KMEANS_PIXELS:  # segment_images keeps refusing them, and says where they run
        with pytest.raises(ValueError, match="kmeans_pixels_segment"):
            E.segment_images(None, torch.zeros(1, 3, 48, 48), method=method)
    assert E.KMEANS_PIXELS == ("k-means", "k-means_ours")


# ---- the restatement on its own inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(2, 0), (65, 1), (341, 2), (1029, 3), (3072, 4)])
def test_restatement_separates_the_plateaus(n, seed):
    px = R.plateaus(n, seed)
    sides = R.plateau_sides(px)
    assert 0 < sides.sum() < n
    x = px.reshape(-1, 3).astype(int)
    assert x[sides == 1].min() - x[sides == 0].max() > 4 * (R.PLATEAU_NOISE - 1)  # the gap exceeds four times the noise range
    r = R.kmeans(px, R.uniforms_for(1, 10)[0][0])
    R.assert_best_is_decided(r)
    for a in r["attempts"]:  # every attempt reaches the one partition, in a few iterations
        assert R.same_partition(a["labels"], sides) and 2 <= a["iters"] <= 6, a["iters"]
    assert len(set(r["compactness"].tolist())) == 1 and r["best"] == 0  # equal compactness: the first attempt stays the best


@pytest.mark.parametrize("n,seed", [(341, 2), (1029, 3), (3072, 4)])
def test_restatement_agrees_with_sklearn_on_the_plateaus(n, seed):
    cluster = pytest.importorskip("sklearn.cluster")
    px = R.plateaus(n, seed)
    r = R.kmeans(px, R.uniforms_for(1, 10)[0][0])
    sk = cluster.KMeans(n_clusters=2, n_init=10, random_state=0).fit(px.reshape(-1, 3).astype(np.float64))
    assert R.same_partition(r["labels"], sk.labels_.astype(np.uint8))
    order = np.argsort(sk.cluster_centers_[:, 0]), np.argsort(r["centers"][:, 0])
    np.testing.assert_allclose(r["centers"][order[1]], sk.cluster_centers_[order[0]], rtol=1e-6)


def test_restatement_on_noise_and_constant_images():
    r = R.kmeans(R.noise(1029, 2), R.uniforms_for(1, 10)[0][0])
    assert r["iters"].max() == 10 and len(set(r["compactness"].tolist())) == 10  # the cap; ten different local optima
    R.assert_best_is_decided(r)
    assert r["compactness"][r["best"]] == r["compactness"].min()
    assert R.kmeans(R.noise(60, 2), R.uniforms_for(1, 2)[0][0], max_iter=1)["iters"].tolist() == [2, 2]  # max(max_iter, 2)
    for value, want in ((200, 255), (0, 0)):
        px = R.constant(1029, value)
        r = R.kmeans(px, R.uniforms_for(1, 10)[0][0])
        for a in r["attempts"]:  # both centres start equal, every label is 0, and the last sample moves to cluster 1
            assert a["relocations"] == [1] and a["iters"] == 2
            assert a["labels"].tolist() == [0] * 1028 + [1]
        assert np.array_equal(r["centers"], np.full((2, 3), value, np.float32))


def test_restatement_relocates_the_larger_index_on_a_tie():
    u = np.array([[0.32, 0.32, 0.32], [0.0, 0.0, 0.0]], np.float32)  # centre 1 starts outside the box: cluster 1 stays empty
    for n, lo_at, hi_at in ((4, 0, 3), (4, 3, 0), (1024, 5, 900), (1024, 900, 5)):
        for swap in (False, True):
            a = R.attempt(R.tie_case(n, lo_at, hi_at).reshape(-1, 3).astype(np.int64), u[::-1] if swap else u)
            assert a["relocations"] == [1]
            # the sample at the larger index left for the empty cluster, and the loop keeps it apart from then on
            assert np.flatnonzero(a["labels"] == (0 if swap else 1)).tolist() == [max(lo_at, hi_at)], (n, lo_at, hi_at, swap)
