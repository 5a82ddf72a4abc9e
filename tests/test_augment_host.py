"""Host side of DINO's augmentation path (kernels_augment.hip's ocm_gaussian_blur_table, utils.pil_color / pil_gaussian_blur,
dino/utils.py's GaussianBlur, Solarization, DataAugmentationDINO and dino_augment_params): the numpy restatement
tests/augment_ref.py against live Pillow, the C helper's integers against the restatement's, the C ABI's declarations and
refusals, and the order of the random draws. No GPU needed."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import augment_ref as A
from vit_ocm_wmsegmentation_amd import _lib, data, utils
from vit_ocm_wmsegmentation_amd.dino import utils as dino_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc")
NEW_SYMBOLS = ["ocm_color_u8_workspace_bytes", "ocm_op_color_u8", "ocm_gaussian_blur_table", "ocm_gaussian_blur_max_axis",
               "ocm_gaussian_blur_u8_workspace_bytes", "ocm_op_gaussian_blur_u8"]
SIDES = [1, 2, 3, 5, 31, 96]
RADII = [0.1, 0.3, 0.5773, 0.868, 1.0, 1.5, 2.0, 5.0]  # 0.5773: where l steps; 5.0: r = 4 above the small sides
FACTORS = [0.0, 0.6, 1.0, 1.4, 3.0]  # 3.0: the clip branch


def _drawn_radii():
    rng = random.Random(11)
    return [rng.uniform(0.1, 2.0) for _ in range(40)]


# ---- the restatement against live Pillow -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", SIDES)
def test_blur_equals_pillow(h):
    Image, ImageFilter = pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageFilter")
    for w in SIDES:
        img = A.noise(h, w, seed=100 * h + w)
        pil = Image.fromarray(img)
        for radius in RADII + _drawn_radii()[(h + w) % 4::4]:
            want = np.asarray(pil.filter(ImageFilter.GaussianBlur(radius)))
            assert np.array_equal(A.gaussian_blur(img, radius), want), (h, w, radius)
    assert np.array_equal(A.gaussian_blur(img, 0), img)  # radius 0: a copy, and the identity weights
    assert A.blur_table(0) == (0, 1 << 24, 0) and A.blur_table(5.0)[0] == 4 and A.blur_table(0.5773)[0] == 0


def test_blur_on_smooth_images_and_every_drawn_radius():
    Image, ImageFilter = pytest.importorskip("PIL.Image"), pytest.importorskip("PIL.ImageFilter")
    img = A.smooth(31, 96, seed=3)
    for radius in _drawn_radii():
        want = np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius)))
        assert np.array_equal(A.gaussian_blur(img, radius), want), radius


def _all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_hsv_round_trip_is_exhaustive():
    """All 2^24 colours each way, one 4096 x 4096 image per direction. The tie rule of hsv2rgb's round() cannot be told from
    the bytes: with halves to even the restatement gives the same 2^24 results, so no input reaches a tie. The code keeps C's
    round()."""
    Image = pytest.importorskip("PIL.Image")
    allc = _all_colours()
    want = np.asarray(Image.fromarray(allc).convert("HSV"))
    assert np.array_equal(A.rgb_to_hsv(allc), want)
    want = np.asarray(Image.fromarray(allc, "HSV").convert("RGB"))
    assert np.array_equal(A.hsv_to_rgb(allc), want)
    assert np.array_equal(A.hsv_to_rgb(allc[::16], np.rint), want[::16])


def _mean_straddling(k, above):
    """An image whose mean L sits just either side of k + 0.5: 16 x 20 grey pixels of k, 159 or 161 of the 320 one higher."""
    img = np.full((16, 20, 3), k, np.uint8)
    img.reshape(-1, 3)[: 160 + (1 if above else -1)] = k + 1
    return img


def test_enhancers_luma_and_solarize_equal_pillow():
    Image, ImageEnhance, ImageOps = (pytest.importorskip(m) for m in ("PIL.Image", "PIL.ImageEnhance", "PIL.ImageOps"))
    images = [A.noise(16, 20, seed=1), A.smooth(16, 20, seed=2), _mean_straddling(100, False), _mean_straddling(100, True)]
    assert A.contrast_mean(images[2]) == 100 and A.contrast_mean(images[3]) == 101
    rng = random.Random(5)
    for img in images:
        pil = Image.fromarray(img)
        for f in FACTORS + [rng.uniform(0.0, 2.0) for _ in range(20)]:
            for enh, fn in ((ImageEnhance.Brightness, A.brightness), (ImageEnhance.Contrast, A.contrast), (ImageEnhance.Color, A.saturation)):
                assert np.array_equal(fn(img, f), np.asarray(enh(pil).enhance(f))), (enh.__name__, f)
        assert np.array_equal(A.luma(img), np.asarray(pil.convert("L")))
        for thr in (128, 0, 255, 77):
            assert np.array_equal(A.solarize(img, thr), np.asarray(ImageOps.solarize(pil, thr)))


def _table(ops, factors, grey=False, radius=0.0, sol=False, crop=(0, 0, 20, 16), hflip=False):
    return dict(crops=np.array([crop]), hflip=np.array([hflip]), ops=np.array([ops], np.int32), factors=np.array([factors], np.float32),
                grey=np.array([grey]), radius=np.array([radius], np.float32), solarize=np.array([sol]))


def test_chain_in_all_24_slot_orders():
    pytest.importorskip("PIL.Image")
    img = A.smooth(16, 20, seed=4)
    factor = {A.OP_BRIGHTNESS: 1.3, A.OP_CONTRAST: 0.7, A.OP_SATURATION: 1.15, A.OP_HUE: 243.0}
    seen = set()
    for n, order in enumerate(itertools.permutations(factor)):
        view = _table(order, [factor[o] for o in order], grey=n % 5 == 0, radius=(0.0, 0.8, 1.7)[n % 3], sol=n % 4 == 1,
                      crop=(1, 2, 19, 15), hflip=bool(n % 2))
        got = A.view_chain(img, view, 0, 12)
        assert got.dtype == np.float32 and got.shape == (3, 12, 12)
        assert np.array_equal(got.view(np.int32), A.pil_view_chain(img, view, 0, 12).view(np.int32)), order
        seen.add(A.view_u8(img, _table(order, [factor[o] for o in order]), 0, 12).tobytes())
    assert len(seen) > 12  # the order matters: the contrast's mean and the clips depend on what ran before


# ---- ocm_gaussian_blur_table against the restatement, as integers ------------------------------------------------------------------
def test_blur_table_equals_the_restatement():
    radii = [0.0] + RADII + _drawn_radii() + [float(np.float32(r)) for r in np.linspace(0.01, 40, 500)]
    got = utils.gaussian_blur_table(radii)
    assert got.dtype == np.uint32 and got.shape == (len(radii), 3)
    for r, row in zip(radii, got):
        assert tuple(int(v) for v in row) == A.blur_table(r), r
    assert sorted(set(got[:, 0].tolist()))[:4] == [0, 1, 2, 3]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "ocm_vit.h")).read()
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    src = open(os.path.join(CSRC, "kernels_augment.hip")).read()
    assert "kernels_augment.hip" in open(os.path.join(CSRC, "Makefile")).read()
    assert "#pragma clang fp contract(off)" in src  # Image.blend is a product, then a sum
    for k, name in enumerate(("NONE", "BRIGHTNESS", "CONTRAST", "SATURATION", "HUE")):
        assert re.search(rf"#define OCM_COLOR_{name} {k}\b", text) and getattr(utils, f"COLOR_{name}") == k == getattr(A, f"OP_{name}")
    assert lib.ocm_gaussian_blur_max_axis() == A.BLUR_MAX_AXIS == 1024
    assert re.search(r"constexpr int AUG_MAX_AXIS = 1024;", src)


def test_operator_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    p, big = C.c_void_p(4096), 1 << 40

    def refused(rc, word):
        assert rc == _lib.OCM_EINVAL, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    table = (C.c_uint32 * 3)()
    assert lib.ocm_gaussian_blur_table(1.0, table) == _lib.OCM_OK and tuple(table) == A.blur_table(1.0)
    refused(lib.ocm_gaussian_blur_table(1.0, None), "null")
    for bad in (-0.5, float("nan"), float("inf"), 5000.0):
        refused(lib.ocm_gaussian_blur_table(bad, table), "radius")

    f = lib.ocm_color_u8_workspace_bytes
    assert f(1) >= 32 and f(65535) >= 65535 * 32 and f(0) == 0 and f(65536) == 0

    def color(src=p, out=p, batch=2, h=9, w=11, ops=p, fac=p, flags=p, ws=p, nbytes=big):
        return lib.ocm_op_color_u8(src, out, batch, h, w, ops, fac, flags, ws, nbytes, None)

    for name in ("src", "out", "ops", "fac", "flags"):
        refused(color(**{name: None}), "null")
    for batch in (0, -1, 65536):
        refused(color(batch=batch), "batch")
    for hw in ((0, 11), (9, 0), (1 << 14, (1 << 12) + 1)):
        refused(color(h=hw[0], w=hw[1]), "image size")
    refused(color(ws=C.c_void_p(4096 + 4)), "aligned")
    assert color(ws=None) == _lib.OCM_ENOMEM and color(nbytes=f(2) - 1) == _lib.OCM_ENOMEM and color(nbytes=0) == _lib.OCM_ENOMEM

    g = lib.ocm_gaussian_blur_u8_workspace_bytes
    assert g(3, 37, 53) >= 3 * 37 * 53 * 3 and g(1, 1024, 1024) >= 3 << 20
    for bad in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1025, 8), (1, 8, 1025)):
        assert g(*bad) == 0, bad
    three = (C.c_float * 3)(0.5, 0.5, 0.5)

    def blur(src=p, batch=2, h=9, w=11, table=p, sol=None, u8=p, f32=p, mean=None, std=None, ws=p, nbytes=big):
        return lib.ocm_op_gaussian_blur_u8(src, batch, h, w, table, sol, u8, f32, mean, std, ws, nbytes, None)

    refused(blur(src=None), "null")
    refused(blur(table=None), "null")
    refused(blur(u8=None, f32=None), "null outputs")
    refused(blur(mean=C.cast(three, C.c_void_p)), "mean and std")
    refused(blur(std=C.cast(three, C.c_void_p)), "mean and std")
    for batch in (0, -1, 65536):
        refused(blur(batch=batch), "batch")
    for hw in ((0, 11), (9, 0)):
        refused(blur(h=hw[0], w=hw[1]), "image size")
    for hw in ((1025, 11), (9, 1025)):  # an axis over the cap
        refused(blur(h=hw[0], w=hw[1]), "up to 1024")
    assert blur(ws=None) == _lib.OCM_ENOMEM and blur(nbytes=g(2, 9, 11) - 1) == _lib.OCM_ENOMEM


def test_python_surface_refusals():
    img = torch.zeros(2, 9, 11, 3, dtype=torch.uint8)
    for call in (lambda: utils.pil_color(img, utils.COLOR_NONE, 0.0), lambda: utils.pil_gaussian_blur(img, 1.0),
                 lambda: dino_utils.GaussianBlur(1.0)(img), lambda: dino_utils.Solarization(1.0)(img),
                 lambda: dino_utils.DataAugmentationDINO(local_crops_number=1)(img)):
        with pytest.raises(RuntimeError):  # no host fall-back
            call()
    with pytest.raises(ValueError):
        utils.pil_color(img.float(), utils.COLOR_NONE, 0.0)
    with pytest.raises(ValueError):
        utils.pil_gaussian_blur(img[..., :2], 1.0)
    with pytest.raises(ValueError):
        dino_utils.DataAugmentationDINO()(img[0])
    with pytest.raises(ValueError):
        utils.gaussian_blur_table([-1.0])


# ---- the draws ---------------------------------------------------------------------------------------------------------------------
def _params(seed, batch=5, n=2):
    return dino_utils.dino_augment_params(batch, 40, 52, (0.4, 1.0), (0.05, 0.4), n, torch.Generator().manual_seed(seed),
                                          random.Random(seed + 1))


def test_params_are_deterministic_per_seed():
    a, b, c = _params(3), _params(3), _params(4)
    assert len(a) == 4
    for va, vb in zip(a, b):
        assert va.keys() == vb.keys() and all(np.array_equal(va[k], vb[k]) and va[k].dtype == vb[k].dtype for k in va)
    assert any(not np.array_equal(va["crops"], vc["crops"]) for va, vc in zip(a, c))
    for v, view in enumerate(a):
        assert view["crops"].shape == (5, 4) and view["ops"].dtype == np.int32 and view["factors"].dtype == np.float32
        assert (view["crops"][:, :2] >= 0).all() and (view["crops"][:, 2] <= 52).all() and (view["crops"][:, 3] <= 40).all()
        assert (view["radius"] > 0).all() if v == 0 else True  # global 1 always blurs
        assert not view["solarize"].any() if v != 1 else True  # only global 2 solarizes


def test_draw_order_matches_draws_made_by_hand():
    """The same generators, drawn from here in torchvision's call order and the reference classes' order."""
    B, n, seed = 6, 2, 9
    views = _params(seed, B, n)
    g, rng = torch.Generator().manual_seed(seed), random.Random(seed + 1)
    jittered = skipped = 0
    for b in range(B):
        for v in range(2 + n):
            i, j, h, w = data.random_resized_crop_params(40, 52, (0.4, 1.0) if v < 2 else (0.05, 0.4), generator=g)
            assert tuple(views[v]["crops"][b]) == (j, i, j + w, i + h)
            assert views[v]["hflip"][b] == bool(torch.rand(1, generator=g).item() < 0.5)
            if 0.8 < torch.rand(1, generator=g).item():  # RandomApply fails: no jitter draws are consumed
                assert not views[v]["ops"][b].any() and not views[v]["factors"][b].any()
                skipped += 1
            else:
                order = torch.randperm(4, generator=g).tolist()
                bf, cf, sf = (float(torch.empty(1).uniform_(lo, hi, generator=g)) for lo, hi in ((0.6, 1.4), (0.6, 1.4), (0.8, 1.2)))
                hf = float(torch.empty(1).uniform_(-0.1, 0.1, generator=g))
                value = {0: np.float32(bf), 1: np.float32(cf), 2: np.float32(sf), 3: np.float32(A.hue_shift(hf))}
                assert views[v]["ops"][b].tolist() == [fn + 1 for fn in order]
                assert views[v]["factors"][b].tolist() == [value[fn] for fn in order]
                jittered += 1
            assert views[v]["grey"][b] == bool(torch.rand(1, generator=g).item() < 0.2)
            p = (1.0, 0.1, 0.5)[min(v, 2)]
            radius = rng.uniform(0.1, 2.0) if rng.random() <= p else 0.0
            assert views[v]["radius"][b] == np.float32(radius)
            if v == 1:
                assert views[v]["solarize"][b] == (rng.random() < 0.2)
    assert jittered > skipped > 0  # both branches of RandomApply were taken, and the streams stayed in step after a skip


def test_hue_shift_truncates_and_wraps():
    assert [A.hue_shift(f) for f in (0.0, 0.05, 0.1, -0.05, -0.1, 0.0039, -0.0039)] == [0, 12, 25, 244, 231, 0, 0]
    g = torch.Generator().manual_seed(0)
    for _ in range(20):
        slots = dict(dino_utils._color_jitter_params(g))
        assert set(slots) == {1, 2, 3, 4} and 0.6 <= slots[1] <= 1.4 and 0.6 <= slots[2] <= 1.4 and 0.8 <= slots[3] <= 1.2
        assert slots[4] == int(slots[4]) and (0 <= slots[4] <= 25 or 231 <= slots[4] <= 255)


def test_reference_classes_draw_as_the_reference_does():
    rng, twin = random.Random(2), random.Random(2)
    blur, sol = dino_utils.GaussianBlur(0.5, 0.1, 2.0, rng=rng), dino_utils.Solarization(0.2, rng=rng)
    assert (blur.prob, blur.radius_min, blur.radius_max, sol.p) == (0.5, 0.1, 2.0, 0.2)
    for _ in range(50):
        want = twin.uniform(0.1, 2.0) if twin.random() <= 0.5 else 0.0
        assert blur.draw() == want
        assert sol.draw() == (twin.random() < 0.2)
