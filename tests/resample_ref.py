"""Pillow's 8-bit Image.resize restated in numpy from its algorithm (libImaging Resample.c: precompute_coeffs,
normalize_coeffs_8bpc and the two 8bpc passes; Geometry.c: ImagingScaleAffine for NEAREST): the reference the resample tests
compare with, itself compared with the live library in tests/test_resample_host.py. Python floats are IEEE doubles and numpy
float32 is C's float, so every statement below is the C statement.

  table(filter, in_size, in0, in1, out_size, flip, ksize_padded) -> (bounds, coeffs, ksize) of one axis
  resize(img, size, filter, box, crop, hflip, vflip)            -> uint8 image, horizontal pass first
  to_tensor(u8)                                                 -> float32 CHW = u8 / 255.0f
"""
import math

import numpy as np

NEAREST, BILINEAR, BICUBIC = 0, 2, 3
PRECISION_BITS = 32 - 8 - 2


def bilinear_filter(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def bicubic_filter(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


FILTERS = {BILINEAR: (bilinear_filter, 1.0), BICUBIC: (bicubic_filter, 2.0)}


def _scale(in0, in1, out_size):
    """(in0, in1 as the floats Pillow holds, (double)(in1 - in0) / outSize with the difference a float)."""
    f0, f1 = np.float32(in0), np.float32(in1)
    return float(f0), float(f1), float(np.float32(f1 - f0)) / out_size


def ksize_of(filt, in0, in1, out_size):
    if filt == NEAREST:
        return 1
    _, _, scale = _scale(in0, in1, out_size)
    return int(math.ceil(FILTERS[filt][1] * max(scale, 1.0))) * 2 + 1


def table(filt, in_size, in0, in1, out_size, flip=False, ksize_padded=None):
    ksize = ksize_of(filt, in0, in1, out_size)
    kp = ksize if ksize_padded is None else ksize_padded
    assert kp >= ksize
    in0, in1, scale = _scale(in0, in1, out_size)
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, kp), np.int32)
    if filt == NEAREST:
        xo = in0 + scale * 0.5
        for xx in range(out_size):
            xin = -1 if xo < 0.0 else int(xo)
            if 0 <= xin < in_size:
                bounds[xx] = (xin, 1)
                coeffs[xx, 0] = 1 << PRECISION_BITS
            xo += scale
    else:
        fn, fsupport = FILTERS[filt]
        filterscale = max(scale, 1.0)
        support = fsupport * filterscale
        ss = 1.0 / filterscale
        for xx in range(out_size):
            center = in0 + (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)
            xmax = min(int(center + support + 0.5), in_size) - xmin
            k, ww = [], 0.0
            for x in range(xmax):
                w = fn((x + xmin - center + 0.5) * ss)
                k.append(w)
                ww += w
            for x in range(xmax):
                w = k[x] / ww if ww != 0.0 else k[x]
                coeffs[xx, x] = int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS))
            bounds[xx] = (xmin, max(xmax, 0))
    if flip:
        bounds, coeffs = bounds[::-1].copy(), coeffs[::-1].copy()
    return bounds, coeffs, ksize


def pass_sums(lines, bounds, coeffs):
    """acc = 2^21 + sum pixel * coeff along axis 1 of `lines` (n, in_size, C), before the shift and the clip: (n, out, C) int64,
    which must fit an int32."""
    out = np.empty((lines.shape[0], bounds.shape[0], lines.shape[2]), np.int64)
    src = lines.astype(np.int64)
    for xx, (first, count) in enumerate(bounds):
        k = coeffs[xx, :count].astype(np.int64)
        out[:, xx] = (1 << (PRECISION_BITS - 1)) + np.einsum("nkc,k->nc", src[:, first:first + count], k)
    assert out.min() >= -(1 << 31) and out.max() < (1 << 31)
    return out


def clip8(sums):
    return np.clip(sums >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(img, size, filt=BICUBIC, box=None, crop=None, hflip=False, vflip=False, return_sums=False):
    """img: (H,W) or (H,W,C) uint8; size (width, height); box (x0, y0, x1, y1) floats with taps outside it; crop (x0, y0, x1,
    y1) integers, a sub-image cut out first; the flips mirror the resized image."""
    squeeze = img.ndim == 2
    a = img[:, :, None] if squeeze else img
    if crop is not None:
        a = a[crop[1]:crop[3], crop[0]:crop[2]]
    H, W = a.shape[:2]
    bx = (0.0, 0.0, float(W), float(H)) if box is None else box
    xb, xc, _ = table(filt, W, bx[0], bx[2], size[0], hflip)
    yb, yc, _ = table(filt, H, bx[1], bx[3], size[1], vflip)
    hsums = pass_sums(a, xb, xc)                              # rows are the lines: (H, out_w, C)
    tmp = clip8(hsums)
    vsums = pass_sums(tmp.transpose(1, 0, 2), yb, yc)         # columns are the lines: (out_w, out_h, C)
    out = clip8(vsums).transpose(1, 0, 2)
    out = np.ascontiguousarray(out[:, :, 0] if squeeze else out)
    return (out, hsums, vsums) if return_sums else out


def to_tensor(u8):
    """torchvision's ToTensor of an (h,w) / (h,w,C) uint8 image: float32 (C,h,w), the IEEE quotient by 255."""
    a = u8[:, :, None] if u8.ndim == 2 else u8
    return np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def noise(h, w, c, seed):
    shape = (h, w) if c == 0 else (h, w, c)
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def blocks(h, w, c, seed=0, side=3):
    """0 / 255 in blocks of `side` pixels: bicubic overshoots both ways at every edge."""
    rs = np.random.RandomState(seed)
    cells = rs.randint(0, 2, (-(-h // side), -(-w // side), max(c, 1))).astype(np.uint8) * 255
    img = cells.repeat(side, 0).repeat(side, 1)[:h, :w]
    return np.ascontiguousarray(img[:, :, 0] if c == 0 else img)


# ---- the cases the host and the device tests share --------------------------------------------------------------------------------
# the kernels' tile constants (kernels_resample.hip), which the device tests choose their shapes by; test_resample_host.py asserts
# them against the source
TILE = dict(RS_THREADS=256, RS_HTILE_W=64, RS_HTILE_ROWS=16, RS_HSPAN=256, RS_VPACK=4)
VTILE = TILE["RS_THREADS"] * TILE["RS_VPACK"]  # bytes of an output row per workgroup of the vertical pass

# ((H, W) -> (h, w)): down, one axis the identity, up, mixed, the identity, 117 taps, a large upscale
SHAPES = [((37, 53), (24, 24)), ((64, 64), (64, 48)), ((50, 70), (128, 96)), ((97, 33), (16, 40)), ((40, 40), (40, 40)),
          ((200, 180), (7, 5)), ((9, 11), (64, 80))]


def tile_edge_shapes():
    """Sizes one below, at and one above every tile constant: output columns per workgroup and source rows per workgroup of the
    horizontal pass, the pixels it stages at a time (one, exactly one and two stagings, and a 481-tap row over three), and
    the bytes of an output row per workgroup of the vertical pass (for one channel and for three)."""
    out = []
    for d in (-1, 0, 1):
        out.append(((20, 90), (10, TILE["RS_HTILE_W"] + d)))
        out.append(((20, 90), (TILE["RS_HTILE_W"] + d, 10)))
        out.append(((TILE["RS_HTILE_ROWS"] + d, 30), (12, 20)))
        out.append(((9, 11), (TILE["RS_HTILE_ROWS"] + d, TILE["RS_HTILE_ROWS"] + d)))
        out.append(((6, TILE["RS_HSPAN"] + d), (6, 8)))
        out.append(((TILE["RS_HSPAN"] + d, 6), (8, 6)))
        out.append(((5, 7), (6, VTILE + d)))
    out.append(((6, 600), (6, 5)))
    return out
