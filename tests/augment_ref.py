"""DINO's per-pixel augmentations restated in numpy from Pillow's algorithms (libImaging BoxBlur.c, Blend.c, Convert.c; ImageOps
.solarize, ImageEnhance): the reference the augmentation tests compare with, itself compared with the live library in
tests/test_augment_host.py. numpy float32 is C's float and Python floats / numpy float64 are C's double, so every statement
below is the C statement.

  blur_table(radius)                 -> (r, ww, fw): the box radius and the two 8.24 weights of one Gaussian radius
  gaussian_blur(img, radius)         -> Image.filter(ImageFilter.GaussianBlur(radius)): three box passes per axis, rows first
  solarize(img, threshold)           -> ImageOps.solarize
  luma(img)                          -> convert('L')
  brightness / contrast / saturation -> ImageEnhance.{Brightness, Contrast, Color}(img).enhance(f)
  rgb_to_hsv / hsv_to_rgb / hue      -> convert('HSV'), convert('RGB'), torchvision's adjust_hue on a byte shift
  normalize(u8, mean, std)           -> ToTensor + Normalize, float32 (3,h,w)
  color(img, ops, factors, grey, solarize_on, threshold) -> the point operations of one view in its own order
  view_chain(img, params, v, b, size) -> one view of one image from a parameter table (dino_augment_params)
"""
import numpy as np

from tests import resample_ref as R

F32 = np.float32
OP_NONE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3, 4
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BLUR_MAX_AXIS = 1024  # kernels_augment.hip's AUG_MAX_AXIS


# ---- Gaussian blur (BoxBlur.c: _gaussian_blur_radius, ImagingLineBoxBlur8 / 32) -------------------------------------------------
def box_radius(radius, passes=3):
    """_gaussian_blur_radius: float variables, the constants 12.0, 1.0 and 2.0 doubles."""
    radius = F32(radius)
    s2 = F32(F32(radius * radius) / F32(passes))
    L = F32(np.sqrt(12.0 * float(s2) + 1.0))
    l = F32(np.floor((float(L) - 1.0) / 2.0))
    a = F32(F32(F32(2) * l + F32(1)) * F32(F32(l * F32(l + F32(1))) - F32(F32(3) * s2)))
    a = F32(a / F32(F32(6) * F32(s2 - F32(F32(l + F32(1)) * F32(l + F32(1))))))
    return F32(l + a)


def blur_table(radius):
    fr = box_radius(radius)
    r = int(fr)
    ww = int(np.uint32(F32(1 << 24) / F32(F32(fr * F32(2)) + F32(1))))
    fw = (((1 << 24) - (2 * r + 1) * ww) & 0xFFFFFFFF) // 2
    return r, ww, fw


def box_pass(a, r, ww, fw):
    """One pass along axis 0 of a uint8 array: direct tap sums, the clamp to the line's ends on this pass's own input."""
    n = a.shape[0]
    x = np.arange(n)
    v = a.astype(np.uint64)
    acc = np.zeros_like(v)
    for i in range(-r, r + 1):
        acc += v[np.clip(x + i, 0, n - 1)]
    far = v[np.clip(x - r - 1, 0, n - 1)] + v[np.clip(x + r + 1, 0, n - 1)]
    bulk = (acc * np.uint64(ww) + far * np.uint64(fw) + np.uint64(1 << 23)) & np.uint64(0xFFFFFFFF)  # UINT32 arithmetic
    return (bulk >> np.uint64(24)).astype(np.uint8)


def gaussian_blur(img, radius):
    if F32(radius) == 0:
        return img.copy()
    r, ww, fw = blur_table(radius)
    a = img.transpose(1, 0, 2) if img.ndim == 3 else img.T  # rows are the lines first
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    a = a.transpose(1, 0, 2) if img.ndim == 3 else a.T
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    return np.ascontiguousarray(a)


# ---- point operations -------------------------------------------------------------------------------------------------------------
def solarize(img, threshold=128):
    return np.where(img < threshold, img, 255 - img).astype(np.uint8)


def luma(img):
    a = img.astype(np.uint32)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def grey(img):
    return np.repeat(luma(img)[..., None], 3, -1)


def blend(d, x, f):
    """Image.blend(degenerate, image, f): a float product, then a float sum (no fused multiply-add)."""
    f = F32(f)
    df, xf = np.broadcast_to(d, x.shape).astype(F32), x.astype(F32)
    t = df + f * (xf - df)  # numpy rounds the product before the sum
    if 0.0 <= f <= 1.0:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def contrast_mean(img):
    """int(ImageStat.Stat(convert('L')).mean[0] + 0.5): an exact sum, a double quotient."""
    L = luma(img)
    return int(float(int(L.astype(np.int64).sum())) / float(L.size) + 0.5)


def brightness(img, f):
    return blend(np.uint8(0), img, f)


def contrast(img, f):
    return blend(np.uint8(contrast_mean(img)), img, f)


def saturation(img, f):
    return blend(grey(img), img, f)


def rgb_to_hsv(img):
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = cr / np.where(flat, 1, mx).astype(F32)
        rc, gc, bc = ((mx - c).astype(F32) / cr for c in (r, g, b))
    hr = bc - gc                                                                   # float
    hg = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(F32)         # double, stored to a float
    hb = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(F32)
    h = np.where(r == mx, hr, np.where(g == mx, hg, hb))
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
    H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(flat, 0, H), np.where(flat, 0, S), mx], -1)
    return out.astype(np.uint8)


def _c_round(x):
    """C's round(): halves away from zero (the operands here are >= 0)."""
    return np.floor(x + 0.5)


def hsv_to_rgb(hsv, rnd=_c_round):
    H, S, V = (hsv[..., c] for c in range(3))
    h6 = H.astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6)
    f = (h6 - i).astype(F32).astype(np.float64)
    fs = (S.astype(F32).astype(np.float64) / 255.0).astype(F32).astype(np.float64)
    v = V.astype(np.float64)
    p = np.clip(rnd(v * (1.0 - fs)), 0, 255).astype(np.uint8)
    q = np.clip(rnd(v * (1.0 - fs * f)), 0, 255).astype(np.uint8)
    t = np.clip(rnd(v * (1.0 - fs * (1.0 - f))), 0, 255).astype(np.uint8)
    k = i.astype(np.int64) % 6
    r = np.choose(k, [V, q, p, p, t, V])
    g = np.choose(k, [t, V, V, q, p, p])
    b = np.choose(k, [p, p, t, V, V, q])
    zero = S == 0
    return np.stack([np.where(zero, V, r), np.where(zero, V, g), np.where(zero, V, b)], -1).astype(np.uint8)


def hue(img, shift):
    """torchvision's adjust_hue on a PIL image with np.uint8(hue_factor * 255) = shift: the H plane wraps modulo 256."""
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + int(shift)) % 256
    return hsv_to_rgb(hsv)


def hue_shift(hue_factor):
    """int(hue_factor * 255) truncated, modulo 256: what the cast to uint8 gives on x86."""
    return int(float(hue_factor) * 255) % 256


def color(img, ops, factors, grey_on=False, solarize_on=False, threshold=128):
    out = img
    for op, f in zip(ops, factors):
        if op == OP_BRIGHTNESS:
            out = brightness(out, f)
        elif op == OP_CONTRAST:
            out = contrast(out, f)
        elif op == OP_SATURATION:
            out = saturation(out, f)
        elif op == OP_HUE:
            out = hue(out, int(f))
        else:
            assert op == OP_NONE, op
    if grey_on:
        out = grey(out)
    if solarize_on:
        out = solarize(out, threshold)
    return np.ascontiguousarray(out)


def normalize(u8, mean=None, std=None):
    """ToTensor, then Normalize's sub_().div_(): float32 (3,h,w), every operation rounded on its own."""
    t = np.ascontiguousarray(u8.transpose(2, 0, 1)).astype(F32) / F32(255)
    if mean is not None:
        t = (t - np.asarray(mean, F32)[:, None, None]) / np.asarray(std, F32)[:, None, None]
    return t


def view_u8(img, view, b, size):
    """The uint8 image of view table `view` (one entry of dino_augment_params' list) for image b: crop + BICUBIC resize + flip,
    the jitter slots and grey, the blur, then solarize."""
    out = R.resize(img, (size, size), R.BICUBIC, crop=tuple(int(c) for c in view["crops"][b]), hflip=bool(view["hflip"][b]))
    out = color(out, view["ops"][b], view["factors"][b], bool(view["grey"][b]))
    out = gaussian_blur(out, view["radius"][b])
    if view["solarize"][b]:
        out = solarize(out)
    return out


def view_chain(img, view, b, size, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    return normalize(view_u8(img, view, b, size), mean, std)


def pil_view_chain(img, view, b, size, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The same view through live Pillow (the caller has checked that it is installed): what upstream's Compose runs, with
    torchvision's thin wrappers written out."""
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
    x0, y0, x1, y1 = (int(c) for c in view["crops"][b])
    im = Image.fromarray(img).crop((x0, y0, x1, y1)).resize((size, size), Image.BICUBIC)
    if view["hflip"][b]:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    for op, f in zip(view["ops"][b], view["factors"][b]):
        if op == OP_BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(float(f))
        elif op == OP_CONTRAST:
            im = ImageEnhance.Contrast(im).enhance(float(f))
        elif op == OP_SATURATION:
            im = ImageEnhance.Color(im).enhance(float(f))
        elif op == OP_HUE:
            h, s, v = im.convert("HSV").split()
            nh = (np.asarray(h).astype(np.int64) + int(f)) % 256
            im = Image.merge("HSV", (Image.fromarray(nh.astype(np.uint8), "L"), s, v)).convert("RGB")
    if view["grey"][b]:
        im = Image.merge("RGB", [im.convert("L")] * 3)
    if F32(view["radius"][b]) != 0:
        im = im.filter(ImageFilter.GaussianBlur(radius=float(view["radius"][b])))
    if view["solarize"][b]:
        im = ImageOps.solarize(im)
    return normalize(np.asarray(im), mean, std)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def smooth(h, w, seed):
    """Low-frequency colour with some noise: jitter, blur and HSV act on plausible pixels, not only on white noise."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = [127 + 120 * np.sin(yy / (3.0 + c) + rs.rand() * 6) * np.cos(xx / (4.0 + 2 * c) + rs.rand() * 6) for c in range(3)]
    return np.clip(np.stack(base, -1) + rs.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
