"""Float64 numpy restatement of skimage.segmentation.chan_vese (0.19.x) as the reference's utils.py:199-225 calls it, written
from the loop include/ocm_vit.h states for ocm_op_chan_vese (scikit-image is not installed: this file is the arbiter of the
device tests, like the Yen and Otsu restatements). `evolve` also returns every iteration's phi and phivar. Below it: generators
of small uint8 test images and a cache, so that every test of a session shares one evaluation per case."""
import functools

import numpy as np

DEFAULTS = dict(mu=0.25, lambda1=1.0, lambda2=1.0, tol=1e-3, max_num_iter=200, dt=0.5)


def normalize(img_u8):
    """skimage: image = image - min(image); if max(image) != 0: image = image / max(image) — in float64."""
    img = np.asarray(img_u8).astype(np.float64)
    img = img - np.min(img)
    if np.max(img) != 0:
        img = img / np.max(img)
    return img


def checkerboard(h, w, square_size=5):
    """skimage's _cv_checkerboard."""
    yv = np.arange(h, dtype=np.float64).reshape(h, 1)
    xv = np.arange(w, dtype=np.float64)
    sf = np.pi / square_size
    xv *= sf
    yv *= sf
    return np.sin(yv) * np.sin(xv)


def step(image, phi, mu, lambda1, lambda2, dt):
    """One Jacobi sweep: every term reads the old phi."""
    eta = 1e-16
    P = np.pad(phi, 1, mode="edge")
    c = P[1:-1, 1:-1]
    e, w, s, n = P[1:-1, 2:], P[1:-1, :-2], P[2:, 1:-1], P[:-2, 1:-1]
    xp, xn, x0 = e - c, c - w, (e - w) / 2.0
    yp, yn, y0 = s - c, c - n, (s - n) / 2.0
    C1 = 1.0 / np.sqrt(eta + xp ** 2 + y0 ** 2)
    C2 = 1.0 / np.sqrt(eta + xn ** 2 + y0 ** 2)
    C3 = 1.0 / np.sqrt(eta + x0 ** 2 + yp ** 2)
    C4 = 1.0 / np.sqrt(eta + x0 ** 2 + yn ** 2)
    K = e * C1 + w * C2 + s * C3 + n * C4
    H = 1.0 * (phi > 0)  # the sharp Heaviside
    Hinv = 1.0 - H
    Hsum, Hinvsum = np.sum(H), np.sum(Hinv)
    c1, c2 = np.sum(image * H), np.sum(image * Hinv)
    if Hsum != 0:
        c1 = c1 / Hsum
    if Hinvsum != 0:
        c2 = c2 / Hinvsum
    D = -lambda1 * (image - c1) ** 2 + lambda2 * (image - c2) ** 2
    delta = 1.0 / (1.0 + phi ** 2)
    new = phi + (dt * delta) * (mu * K + D)
    return new / (1.0 + mu * dt * delta * (C1 + C2 + C3 + C4))


def evolve(image, phi0, mu=0.25, lambda1=1.0, lambda2=1.0, tol=1e-3, max_num_iter=200, dt=0.5):
    """image: normalised float64 (h, w); phi0: the start. Returns dict(phi, mask, iters, phis = [phi_0 .. phi_iters],
    phivars = [phivar_1 .. phivar_iters])."""
    phi = np.array(phi0, dtype=np.float64)
    phis, phivars = [phi], []
    i, phivar = 0, np.finfo(np.float64).max
    while phivar > tol and i < max_num_iter:
        new = step(image, phi, mu, lambda1, lambda2, dt)
        phivar = float(np.sqrt(((new - phi) ** 2).mean()))
        phi = new
        i += 1
        phis.append(phi)
        phivars.append(phivar)
    return dict(phi=phi, mask=phi > 0, iters=i, phis=phis, phivars=phivars)


def chan_vese(img_u8, init=None, **kw):
    """skimage.segmentation.chan_vese(img_u8, ..., init_level_set="checkerboard" or the array `init`), with the history."""
    img_u8 = np.asarray(img_u8)
    phi0 = checkerboard(*img_u8.shape) if init is None else init
    return evolve(normalize(img_u8), phi0, **{**DEFAULTS, **kw})


# ---- test images (uint8) ---------------------------------------------------------------------------------------------------------
def blobs(h, w, seed):
    """A few bright ellipses on a dark ground, smooth edges, plus uniform noise: what the classical baseline is run on."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), 40.0)
    for _ in range(2 + seed % 3):
        cy, cx = rs.uniform(0.15, 0.85) * h, rs.uniform(0.15, 0.85) * w
        ry, rx = rs.uniform(0.12, 0.3) * h + 1, rs.uniform(0.12, 0.3) * w + 1
        d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
        img += rs.uniform(90, 150) / (1.0 + np.exp(np.clip((d - 1.0) * 6.0, -50, 50)))
    img += rs.uniform(-12, 12, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def flat(h, w, value=93):
    """A constant image: normalises to all zero through the `max == 0` branch."""
    return np.full((h, w), value, np.uint8)


def step_image(h, w, lo=50, hi=200):
    """Two levels, the edge between columns w // 2 - 1 and w // 2."""
    img = np.full((h, w), lo, np.uint8)
    img[:, w // 2:] = hi
    return img


def random_start(h, w, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (h, w))


@functools.lru_cache(maxsize=None)
def cached(kind, h, w, seed, max_num_iter=200, tol=1e-3, start=None):
    """One evaluation per (image kind, size, seed, max_num_iter, tol, start seed or None for the checkerboard), shared by the
    tests of a session. The arrays it returns are not to be modified. Returns (img_u8, phi0, result of evolve)."""
    img = {"blobs": lambda: blobs(h, w, seed), "noise": lambda: noise(h, w, seed), "flat": lambda: flat(h, w),
           "step": lambda: step_image(h, w)}[kind]()
    phi0 = checkerboard(h, w) if start is None else random_start(h, w, start)
    return img, phi0, evolve(normalize(img), phi0, **{**DEFAULTS, "max_num_iter": max_num_iter, "tol": tol})
