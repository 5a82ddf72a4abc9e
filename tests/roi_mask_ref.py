"""Pure-numpy restatement of the ROI step of the reference's SimMIMTransform.__call__ (data.py:211-233, mim.py --roi_masking) as
scikit-image 0.19.3 computes it, the reference of tests/test_roi_mask_gpu.py and tests/test_roi_mask_memcheck_gpu.py, itself held
against live scipy, Pillow, torch and numpy by tests/test_roi_mask_host.py — and the image families the device tests run on.
Closing and labelling come from tests/morph_ref.py."""
import functools
import math

import numpy as np

from tests import morph_ref as M


# ---- steps 1-6 ------------------------------------------------------------------------------------------------------------------
def gray_u8(img):
    """ToPILImage()(img).convert('L') of a float32 (C,h,w) image, C in (1, 3): each channel byte(img * 255) — an fp32 multiply,
    truncated —, then L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; one channel is its own grey image."""
    u = (np.asarray(img, np.float32) * np.float32(255.0)).astype(np.int32).astype(np.uint8).astype(np.uint32)
    if u.shape[0] == 1:
        return u[0].astype(np.uint8)
    return ((19595 * u[0] + 38470 * u[1] + 7471 * u[2] + 0x8000) >> 16).astype(np.uint8)


def remove_small_labels(ar, min_size):
    """skimage.morphology.remove_small_objects of an INTEGER array: the array is its own label image, so a value goes as a
    whole when fewer than min_size pixels hold it, whatever their components."""
    sizes = np.bincount(ar.ravel())
    out = ar.copy()
    out[(sizes < min_size)[ar]] = 0
    return out


def sample_index(in_size, out_size):
    """scipy.ndimage.zoom(order=0, mode='mirror', grid_mode=True) along one axis, which skimage's resize(order=0,
    anti_aliasing=False) calls: the coordinate (i + 0.5) * z - 0.5 with z = in / out in double, then order 0's floor(c + 0.5),
    clamped to the axis."""
    z = float(in_size) / float(out_size)
    return np.array([min(max(math.floor(((i + 0.5) * z - 0.5) + 0.5), 0), in_size - 1) for i in range(out_size)], np.int32)


def short_sample_index(in_size, out_size):
    """The one-step formula that must NOT be used: it differs from scipy on some pairs."""
    return np.array([min(math.floor((i + 0.5) * in_size / out_size), in_size - 1) for i in range(out_size)], np.int32)


def wrap_nonzero(labels):
    """rois.astype(np.uint8) != 0 of a float64 label image: numpy's cast wraps modulo 256 on x86-64."""
    return (np.asarray(labels).astype(np.int64) & 255) != 0


def rois_on_grid(img, gh, gw, level=10, min_size=20):
    """Steps 1-5: the bool (gh, gw) array `rois` of data.py:229 for one image."""
    g = gray_u8(img)
    binary = np.where(g > level, 255, 0).astype(np.uint8)
    cleaned = remove_small_labels(binary, min_size)
    labels, _ = M.label8(M.closing(cleaned != 0))
    h, w = labels.shape
    sampled = labels.astype(np.float64)[np.ix_(sample_index(h, gh), sample_index(w, gw))]
    return wrap_nonzero(sampled)


def roi_mask(img, mask, level=10, min_size=20):
    """(new mask as 0 / 1 in mask's dtype, used) for one float32 (C,h,w) image and one (gh, gw) mask."""
    mask = np.asarray(mask)
    set_ = mask != 0
    new = set_ & rois_on_grid(img, mask.shape[0], mask.shape[1], level, min_size)
    used = bool(new.sum() != 0)
    return (new if used else set_).astype(mask.dtype), used


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
L10, L11 = (33, 0, 3), (36, 0, 3)  # colour triples whose L is 10 and 11


def from_u8(u8):
    """A float32 (3,h,w) image whose channel bytes are exactly u8 ((3,h,w) or (h,w) replicated): (k + 0.5) / 255."""
    u8 = np.asarray(u8)
    if u8.ndim == 2:
        u8 = np.stack([u8] * 3)
    return ((u8.astype(np.float64) + 0.5) / 255.0).astype(np.float32)


def below_eleven():
    """The largest float32 v with fl(v * 255) < 11: its byte is 10."""
    v = np.float32(11.0 / 255.0)
    while np.float32(v * np.float32(255.0)) < 11:
        v = np.nextafter(v, np.float32(1.0))
    while np.float32(v * np.float32(255.0)) >= 11:
        v = np.nextafter(v, np.float32(0.0))
    return v


def spaced_points(h, w, gh, gw, gap=9):
    """Sample points (y, x, i, j), chosen in raster order, pairwise at least `gap` apart (Chebyshev): no closing joins them."""
    ri, ci = sample_index(h, gh), sample_index(w, gw)
    pts = []
    for i, y in enumerate(ri):
        for j, x in enumerate(ci):
            if all(max(abs(y - p[0]), abs(x - p[1])) >= gap for p in pts):
                pts.append((int(y), int(x), i, j))
    return pts


def _ballast(u, y, x):
    """A bright 5 x 5 block around (y, x), moved inside the image where it has room: more than 20 pixels."""
    h, w = u.shape
    y, x = max(min(y, h - 3), 2), max(min(x, w - 3), 2)
    u[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = 200


@functools.lru_cache(maxsize=None)
def families(h, w, gh, gw):
    """name -> (float32 (3,h,w) image, int64 (gh,gw) mask): the image families of the device tests."""
    rs = np.random.RandomState(1000 * h + 10 * w + gh)
    ri, ci = sample_index(h, gh), sample_index(w, gw)
    ones = np.ones((gh, gw), np.int64)
    f = {}
    # bright blobs on black; the mask has cells on and off them
    u = np.zeros((h, w), np.uint8)
    u[:(h + 1) // 2, :(w + 1) // 2] = 180
    _ballast(u, h - 3, w // 4)
    m = (rs.uniform(size=(gh, gw)) < 0.6).astype(np.int64)
    m[0, 0] = m[-1, -1] = 1
    f["mixed"] = (from_u8(u), m)
    f["dark"] = (from_u8(rs.randint(0, 11, size=(h, w)).astype(np.uint8)), m.copy())
    # 19 and 20 isolated white pixels on a pitch-3 lattice through the first sample point: every component is one pixel
    lat = [(y, x) for y in range(ri[0] % 3, h, 3) for x in range(ci[0] % 3, w, 3)]
    lat.sort(key=lambda p: (max(abs(p[0] - ri[0]), abs(p[1] - ci[0])), p))
    for n in (19, 20):
        u = np.zeros((h, w), np.uint8)
        for y, x in lat[:n]:
            u[y, x] = 255
        f[f"count{n}"] = (from_u8(u), ones.copy())
    # an ROI, but the only masked cell samples off it
    u = np.zeros((h, w), np.uint8)
    u[:(h + 1) // 2, :(w + 1) // 2] = 90
    m = np.zeros((gh, gw), np.int64)
    m[-1, -1] = 1
    f["disjoint"] = (from_u8(u), m)
    # grey levels at sample points far enough apart that the closing leaves them alone; a block elsewhere carries the count
    pts = spaced_points(h, w, gh, gw)
    if len(pts) >= 4:
        u = np.zeros((3, h, w), np.uint8)
        u[:, pts[0][0], pts[0][1]] = 10
        u[:, pts[1][0], pts[1][1]] = 11
        u[:, pts[2][0], pts[2][1]] = np.array(L10, np.uint8)
        _ballast(u[0], pts[3][0], pts[3][1])
        u[1] = np.where(u[0] == 200, 200, u[1])
        u[2] = np.where(u[0] == 200, 200, u[2])
        f["grey_a"] = (from_u8(u), ones.copy())
        u = np.zeros((3, h, w), np.uint8)
        u[:, pts[0][0], pts[0][1]] = np.array(L11, np.uint8)
        _ballast(u[0], pts[3][0], pts[3][1])
        u[1] = np.where(u[0] == 200, 200, u[1])
        u[2] = np.where(u[0] == 200, 200, u[2])
        img = from_u8(u)
        img[:, pts[1][0], pts[1][1]] = below_eleven()                       # byte 10: background
        img[:, pts[2][0], pts[2][1]] = np.nextafter(below_eleven(), np.float32(1.0))  # byte 11: ROI
        f["grey_b"] = (img, ones.copy())
    # two strokes with a 2-pixel gap around the sample point nearest the centre: ROI there only after the closing
    y, x = min(((int(a), int(b)) for a in ri for b in ci), key=lambda p: (abs(p[0] - h // 2) + abs(p[1] - w // 2), p))
    if x >= 1 and x + 2 < w:
        u = np.zeros((h, w), np.uint8)
        u[max(y - 5, 0):y + 6, x - 1] = 255
        u[max(y - 5, 0):y + 6, x + 2] = 255
        f["gap"] = (from_u8(u), ones.copy())
    # a stroke two pixels from the left edge: the dilation grows it against the edge and the erosion (border 1) keeps that
    if w >= 8 and h >= 26:
        u = np.zeros((h, w), np.uint8)
        u[3:h - 3, 2] = 255
        f["edge"] = (from_u8(u), ones.copy())
    for img, m in f.values():
        img.setflags(write=False)
        m.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(h, w, gh, gw):
    """name -> (new mask int64, used) for families(h, w, gh, gw)."""
    return {k: roi_mask(img, m) for k, (img, m) in families(h, w, gh, gw).items()}


def geometries(T):
    """(h, w, gh, gw) of the device tests for a labelling tile side T."""
    return [(32, 32, 4, 4), (48, 48, 12, 12), (37, 37, 5, 5), (2 * T + 3, 2 * T + 3, 7, 7), (64, 64, 64, 64), (33, 33, 2, 2),
            (40, 56, 5, 8)]


@functools.lru_cache(maxsize=None)
def wrap_case():
    """S = 128, G = 16: 256 single bright pixels at (8a + 4, 8b + 4) and an all-ones mask. The closing leaves the lattice as it
    is, so sample (i, j) reads label 16 i + j + 1 and cell (15, 15) reads 256, which the uint8 cast turns into 0."""
    u = np.zeros((128, 128), np.uint8)
    u[4::8, 4::8] = 255
    img, m = from_u8(u), np.ones((16, 16), np.int64)
    img.setflags(write=False)
    return img, m, roi_mask(img, m)


def batch(fams, names):
    """(images (B,3,h,w) float32, masks (B,gh,gw) int64) of the named families, in order."""
    return np.stack([fams[n][0] for n in names]), np.stack([fams[n][1] for n in names])
