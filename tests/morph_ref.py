"""Pure-numpy restatement of the query-point chain of analyse_attention.py --region_query (skimage 0.19.3 / scipy.ndimage
semantics), the reference of tests/test_morph_gpu.py and tests/test_region_query_gpu.py, itself pinned against live
scipy.ndimage by tests/test_morph_host.py: 8-connected labelling in raster order, remove_small_objects, binary dilation /
erosion with a border value, binary_closing, region sums, the Yen level of a histogram, the query mean — and the input
families and sizes the device kernels are tested on."""
import functools

import numpy as np

DISK2 = np.array([[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]], np.uint8)
NEIGHBOURS8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def label8(mask):
    """(labels int32, n): flood fill from every unlabelled foreground pixel met in raster order — components are numbered
    by their first pixel, as skimage.measure.label(connectivity=2) / scipy.ndimage.label(structure=ones((3,3))) do."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    labels = np.zeros((h, w), np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(m)):  # np.nonzero walks in raster order
        if labels[y0, x0]:
            continue
        n += 1
        labels[y0, x0] = n
        stack = [(int(y0), int(x0))]
        while stack:
            y, x = stack.pop()
            for dy, dx in NEIGHBOURS8:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and m[yy, xx] and not labels[yy, xx]:
                    labels[yy, xx] = n
                    stack.append((yy, xx))
    return labels, n


def remove_small_objects(mask, min_size=20):
    """skimage.morphology.remove_small_objects of a bool mask with connectivity=2."""
    labels, n = label8(mask)
    sizes = np.bincount(labels.ravel(), minlength=n + 1)
    small = sizes < min_size
    small[0] = True
    return ~small[labels]


def _shifted(mask, footprint, border, mirror):
    fp = np.asarray(footprint) != 0
    r = fp.shape[0] // 2
    m = np.asarray(mask) != 0
    h, w = m.shape
    pad = np.full((h + 2 * r, w + 2 * r), bool(border))
    pad[r:r + h, r:r + w] = m
    for dy in range(fp.shape[0]):
        for dx in range(fp.shape[1]):
            if fp[dy, dx]:
                oy, ox = (-(dy - r), -(dx - r)) if mirror else (dy - r, dx - r)
                yield pad[r + oy:r + oy + h, r + ox:r + ox + w]


def dilate(mask, footprint=DISK2, border=0):
    """scipy.ndimage.binary_dilation(mask, footprint, border_value=border): OR over the mirrored footprint."""
    return np.logical_or.reduce(list(_shifted(mask, footprint, border, True)))


def erode(mask, footprint=DISK2, border=0):
    """scipy.ndimage.binary_erosion(mask, footprint, border_value=border): AND over the footprint."""
    return np.logical_and.reduce(list(_shifted(mask, footprint, border, False)))


def closing(mask, footprint=DISK2):
    """skimage.morphology.binary_closing (0.19.3): dilation with border 0, erosion with border_value=True."""
    return erode(dilate(mask, footprint, 0), footprint, 1)


def region_sums(labels, n):
    """area, sum_row, sum_col (int64 (n,)) and bbox (int32 (n,4): min_row, min_col, max_row + 1, max_col + 1; (h, w, 0, 0)
    for an absent label) of the labels 1..n; labels outside are ignored."""
    labels = np.asarray(labels)
    h, w = labels.shape
    area, sr, sc = (np.zeros(n, np.int64) for _ in range(3))
    bbox = np.tile(np.array([h, w, 0, 0], np.int32), (n, 1))
    ys, xs = np.nonzero((labels >= 1) & (labels <= n))
    l = labels[ys, xs] - 1
    np.add.at(area, l, 1)
    np.add.at(sr, l, ys)
    np.add.at(sc, l, xs)
    np.minimum.at(bbox[:, 0], l, ys)
    np.minimum.at(bbox[:, 1], l, xs)
    np.maximum.at(bbox[:, 2], l, ys + 1)
    np.maximum.at(bbox[:, 3], l, xs + 1)
    return area, sr, sc, bbox


def get_rois(mask):
    """utils.py:250-254 for a bool mask: the label image and its count."""
    return label8(closing(remove_small_objects(mask, 20)))


def cleaning_points(mask):
    """utils.py:256-281: (x0, y0) = (centroid column, centroid row) of the regions with area >= 10, in label order."""
    labels, n = get_rois(mask)
    area, sr, sc, _ = region_sums(labels, n)
    return [(float(sc[i] / np.float64(area[i])), float(sr[i] / np.float64(area[i]))) for i in range(n) if area[i] >= 10]


def yen_criterion(pmf, t):
    """The Yen criterion of splitting a pmf after bin t, written out term by term (the brute-force check of yen_from_hist)."""
    p1 = float(sum(pmf[:t + 1]))
    a = float(sum(v * v for v in pmf[:t + 1]))
    b = float(sum(v * v for v in pmf[t + 1:]))
    with np.errstate(divide="ignore"):
        return float(np.log(np.float64((p1 * (1.0 - p1)) ** 2) / np.float64(a * b)))


def yen_from_hist(hist):
    """skimage.filters.threshold_yen (0.19.3) of a uint8 image from its 256-bin histogram, in float64."""
    h = np.asarray(hist, np.float64)
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if lo == hi:
        return lo
    pmf = h[lo:hi + 1] / h[lo:hi + 1].sum()
    P1 = np.cumsum(pmf)
    P1_sq = np.cumsum(pmf ** 2)
    P2_sq = np.cumsum(pmf[::-1] ** 2)[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        crit = np.log(((P1_sq[:-1] * P2_sq[1:]) ** -1) * (P1[:-1] * (1.0 - P1[:-1])) ** 2)
    return lo + int(np.argmax(crit))


def gray_u8(img):
    """image_to_gray_u8 of a float32 (C,H,W) image: mul(255) truncated, PIL's integer RGB -> L weights."""
    u = (np.asarray(img, np.float32) * np.float32(255.0)).astype(np.int32).astype(np.uint8).astype(np.uint32)
    if u.shape[0] == 1:
        return u[0].astype(np.uint8)
    return ((19595 * u[0] + 38470 * u[1] + 7471 * u[2] + 0x8000) >> 16).astype(np.uint8)


def query_points(img, patch):
    """analyse_attention.py:184-193 for a float32 (C,S,S) image: (points, tokens)."""
    g = gray_u8(img)
    level = yen_from_hist(np.bincount(g.ravel(), minlength=256))
    points = cleaning_points(level <= g)
    wf = g.shape[-1] // patch
    return points, [int(x0 // patch * wf + y0 // patch) for x0, y0 in points]


def head_mean(rows):
    """np.mean over heads of (H, P) float32 rows as ocm_op_head_mean computes it: sequential float32 sum, / H."""
    s = rows[0].astype(np.float32).copy()
    for h in range(1, rows.shape[0]):
        s = s + rows[h]
    return s / np.float32(rows.shape[0])


def query_mean(rows, selections):
    """rows (T,H,R,P) float32; per tile the mean over its selected rows' head means, added in selection order in float32
    and divided by their number (np.mean(list_of_float32_maps, axis=0)); NaN for an empty selection."""
    T, H, R, P = rows.shape
    out = np.full((T, P), np.nan, np.float32)
    for t, sel in enumerate(selections):
        if not len(sel):
            continue
        acc = head_mean(rows[t, :, sel[0]])
        for q in sel[1:]:
            acc = acc + head_mean(rows[t, :, q])
        out[t] = acc / np.float32(len(sel))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def sizes(T):
    """The image sizes of the device tests for a labelling tile side T."""
    return [(1, 1), (1, T + 5), (T + 5, 1), (T - 1, T + 1), (T, T), (2 * T + 3, 3 * T + 1), (37, 53)]


def _put(m, y, x, block):
    """OR `block` into m at (y, x), clipped to the image."""
    h, w = m.shape
    y, x = max(y, 0), max(x, 0)
    b = np.asarray(block, bool)[:max(h - y, 0), :max(w - x, 0)]
    if y < h and x < w:
        m[y:y + b.shape[0], x:x + b.shape[1]] |= b


def serpentine(h, w):
    """Rows 0, 4, 8, ... full, joined alternately at the right and the left edge: one component, one long chain."""
    m = np.zeros((h, w), bool)
    m[0::4] = True
    for k, y in enumerate(range(0, h - 4, 4)):
        m[y:y + 5, (w - 1) if k % 2 == 0 else 0] = True
    return m


def gaussian_noise(h, w, seed, sigma=1.5, quantile=0.6):
    """Thresholded Gaussian-filtered noise (separable convolution, reflected edges)."""
    rs = np.random.RandomState(seed)
    r = 4
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = np.pad(rs.standard_normal((h, w)), r, mode="symmetric")
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, a)
    a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, a)
    return a > np.quantile(a, quantile)


@functools.lru_cache(maxsize=None)
def families(h, w, T):
    """name -> bool (h, w) mask: the input families of the device tests, clipped to the image."""
    f = {}
    f["empty"] = np.zeros((h, w), bool)
    f["full"] = np.ones((h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    f["checkerboard"] = (yy + xx) % 2 == 0          # one component under 8-connectivity
    f["isolated"] = (yy % 2 == 0) & (xx % 2 == 0)   # the maximum label count
    f["serpentine"] = serpentine(h, w)
    u = np.zeros((h, w), bool)                      # arms meet only in the last row; the right arm starts first
    u[2:, 1 % w] = True
    u[0:, w - 2 if w > 2 else w - 1] = True
    u[h - 1, (1 % w):] = True
    _put(u, h // 2, w // 2, np.ones((2, 2)))        # an island between the arms (joins them only on tiny images)
    f["u_shape"] = u
    d = np.zeros((h, w), bool)                      # blobs that touch only diagonally across tile corners
    _put(d, T - 3, T - 3, np.ones((3, 3)))
    _put(d, T, T, np.ones((3, 3)))
    _put(d, T - 3, 2 * T, np.ones((3, 3)))
    _put(d, T, 2 * T - 3, np.ones((3, 3)))
    _put(d, 2 * T - 2, T - 2, np.eye(4))
    _put(d, 0, 0, np.ones((2, 2)))
    f["diagonal_corner"] = d
    f["noise"] = gaussian_noise(h, w, 1000 + 7 * h + w)
    s = np.zeros((h, w), bool)                      # components of exactly 19 and 20 pixels, and 9 and 10
    _put(s, 1, 1, np.ones((1, 19)))
    _put(s, 3, 1, np.ones((1, 20)))
    blk = np.ones((4, 5))
    _put(s, 6, 1, blk)
    blk19 = blk.copy()
    blk19[3, 4] = 0
    _put(s, 6, 8, blk19)
    _put(s, 12, 1, np.ones((3, 3)))
    _put(s, 12, 6, np.ones((2, 5)))
    _put(s, 17, 2, np.eye(10))                      # a 10-pixel diagonal: one component only under 8-connectivity
    _put(s, 17, 16, np.eye(9)[::-1])
    _put(s, T - 2, 24, np.ones((5, 4)))             # 20 pixels across a tile border
    _put(s, T - 2, 30, blk19.T)
    f["sizes"] = s
    e = np.zeros((h, w), bool)                      # foreground on every image edge, with gaps closing can and cannot fill
    e[0, ::3] = e[h - 1, 1::4] = True
    e[::5, 0] = e[2::3, w - 1] = True
    _put(e, 0, 0, np.ones((6, 6)))
    _put(e, h - 5, w - 7, np.ones((5, 7)))
    _put(e, h // 2, 0, np.ones((3, 9)))
    f["edges"] = e
    for v in f.values():
        v.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(h, w, T):
    """name -> dict(labels, n, removed, dilated, eroded1, closed, rois, rois_n, stats, points) for families(h, w, T)."""
    out = {}
    for name, m in families(h, w, T).items():
        labels, n = label8(m)
        rois, rois_n = get_rois(m)
        out[name] = dict(labels=labels, n=n, removed=remove_small_objects(m, 20), dilated=dilate(m, DISK2, 0),
                         eroded1=erode(m, DISK2, 1), eroded0=erode(m, DISK2, 0), closed=closing(m), rois=rois, rois_n=rois_n,
                         stats=region_sums(labels, max(n, 1)), points=cleaning_points(m))
    return out
