"""numpy restatement of the reference's utils.kmeans (utils.py:118-169): cv2.kmeans(Z, 2, None, (EPS + MAX_ITER, max_iter, eps),
attempts, KMEANS_RANDOM_CENTERS) on the pixel triples of a uint8 image as OpenCV 4.x modules/core/src/kmeans.cpp runs it for
K = 2, dims = 3, then np.uint8(centres)[labels] and its Otsu mask. include/ocm_vit.h states the loop; this file is the arbiter
of the device tests (OpenCV is not installable here: parity with a live cv2 is unpinned).

Arithmetic: float32 elementwise (numpy rounds every operation on its own), exact integer sums rounded to float32 once, the
centre shift and the compactness in float64. The compactness is summed in two orders (numpy's pairwise sum and a sequential
cumsum): their spread is what a third fixed order — the device's — may differ by."""
import ctypes as C

import numpy as np

F = np.float32
RNG_START = 0xffffffff
RNG_A = 4164903690
MASK64 = (1 << 64) - 1


# ---- cv::RNG ---------------------------------------------------------------------------------------------------------------------
def rng_uniform(state, n):
    """n draws in Python big integers: state = (state & 0xffffffff) * 4164903690 + (state >> 32) mod 2^64, a draw is
    (float)(uint32)state * 2.3283064365386963e-10f. A state of 0 stands for 0xffffffff. Returns (float32 (n,), new state)."""
    s = int(state) or RNG_START
    out = np.empty(n, F)
    for i in range(n):
        s = ((s & 0xffffffff) * RNG_A + (s >> 32)) & MASK64
        out[i] = F(s & 0xffffffff) * F(2.3283064365386963e-10)
    return out, s


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def dist(x, c):
    """((t0 t0 + t1 t1) + t2 t2), t = x - c, in float32. x (N,3) float32, c (3,) float32 or (N,3)."""
    t = x - c
    return (t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]


def start_centres(u, lo, hi):
    """c[k][j] = (u (1 + 2 margin) - margin) (hi[j] - lo[j]) + lo[j], margin = 1.f / 3. u (2,3) float32."""
    margin = F(1) / F(3)
    return ((u.astype(F) * (F(1) + margin * F(2)) - margin) * (hi - lo) + lo).astype(F)


def attempt(xi, u, max_iter=10, eps=1.0):
    """One attempt on the integer samples xi (N,3) int64 from the uniforms u (2,3). Returns a dict: labels (N,) uint8, centers
    (2,3) float32, compactness / compactness_seq (the two summation orders), iters, relocations (the iterations that moved a
    sample into an empty cluster)."""
    x = xi.astype(F)
    n = x.shape[0]
    lo, hi = x.min(0), x.max(0)
    c = start_centres(np.asarray(u, F).reshape(2, 3), lo, hi)
    assert c.dtype == F
    labels = np.zeros(n, np.int64)
    it, cap, relocations = 0, max(int(max_iter), 2), []
    while True:
        shift = np.inf
        if it > 0:
            old = c.copy()
            count = np.array([np.sum(labels == 0), np.sum(labels == 1)], np.int64)
            sums = np.stack([xi[labels == k].sum(0) for k in (0, 1)]).astype(np.int64)
            for k in (0, 1):
                if count[k]:
                    continue
                m = int(np.argmax(count))  # the first maximum, as OpenCV's scan keeps it
                b = sums[m].astype(F) * (F(1) / F(count[m]))
                d = dist(x, b)
                d[labels != m] = -1.0
                far = n - 1 - int(np.argmax(d[::-1]))  # the largest distance, the largest index on a tie
                labels[far] = k
                count[m] -= 1
                count[k] += 1
                sums[m] -= xi[far]
                sums[k] += xi[far]
                relocations.append(it)
            c = np.stack([sums[k].astype(F) * (F(1) / F(count[k])) for k in (0, 1)])
            assert c.dtype == F
            shift = 0.0
            for k in (0, 1):
                t = (c[k] - old[k]).astype(np.float64)
                shift = max(shift, float((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))
        it += 1
        if it == cap or shift <= float(eps) * float(eps):
            d = dist(x, c[labels]).astype(np.float64)
            return dict(labels=labels.astype(np.uint8), centers=c, compactness=float(d.sum()),
                        compactness_seq=float(np.cumsum(d)[-1]), iters=it, relocations=relocations)
        labels = (dist(x, c[1]) < dist(x, c[0])).astype(np.int64)  # a tie goes to 0


def kmeans(pixels, uniforms, max_iter=10, eps=1.0):
    """Every attempt of one problem. pixels: uint8, 3 N of them in raster order; uniforms (attempts, 2, 3). Returns a dict:
    attempts (the list of attempt() results), best (the first attempt with the smallest compactness), and that attempt's
    labels and centers."""
    xi = np.asarray(pixels, np.uint8).reshape(-1, 3).astype(np.int64)
    runs = [attempt(xi, u, max_iter, eps) for u in np.asarray(uniforms, F).reshape(-1, 2, 3)]
    best = 0
    for a, r in enumerate(runs):
        if r["compactness"] < runs[best]["compactness"]:
            best = a
    return dict(attempts=runs, best=best, labels=runs[best]["labels"], centers=runs[best]["centers"],
                compactness=np.array([r["compactness"] for r in runs]), iters=np.array([r["iters"] for r in runs], np.int32))


def same_partition(a, b):
    return np.array_equal(a, b) or np.array_equal(a, 1 - b)


def assert_best_is_decided(r, rel=1e-9):
    """The choice of the best attempt does not hang on the summation order: any two attempts with different partitions differ
    in compactness by more than `rel`, relatively."""
    runs = r["attempts"]
    for i in range(len(runs)):
        for j in range(i + 1, len(runs)):
            if same_partition(runs[i]["labels"], runs[j]["labels"]):
                continue
            ci, cj = runs[i]["compactness"], runs[j]["compactness"]
            assert abs(ci - cj) > rel * max(ci, cj), (i, j, ci, cj)


def compactness_rtol(run, base=1e-12):
    """The tolerance rule of tests/test_cluster_shapes_gpu.py for a device fp64 sum: `base` while the reference's two summation
    orders agree to a quarter of it, else 4 x their spread."""
    a, b = run["compactness"], run["compactness_seq"]
    spread = abs(a - b) / abs(a) if a else 0.0
    return base if spread < base / 4 else 4 * spread


# ---- res and its Otsu mask -------------------------------------------------------------------------------------------------------
def painting(labels, centers):
    """np.uint8(centres)[labels].reshape(-1): truncation; up to six distinct values."""
    return centers.astype(np.uint8)[labels.astype(np.int64)].reshape(-1)


def otsu_mask(res, lib):
    """cv2.threshold(res, 0, 255, THRESH_BINARY + THRESH_OTSU)[1]: ocm_otsu_threshold on the histogram, res > level ? 255 : 0."""
    hist = np.bincount(res, minlength=256).astype(np.uint64)
    level = int(lib.ocm_otsu_threshold(hist.ctypes.data_as(C.POINTER(C.c_uint64)), int(res.size)))
    assert level >= 0
    return np.where(res > level, 255, 0).astype(np.uint8), level


def segment(pixels, uniforms, lib, max_iter=10, eps=1.0):
    """kmeans() plus mask and level."""
    r = kmeans(pixels, uniforms, max_iter, eps)
    r["mask"], r["level"] = otsu_mask(painting(r["labels"], r["centers"]), lib)
    return r


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
PLATEAU_LOW, PLATEAU_HIGH, PLATEAU_NOISE = 40, 190, 21  # noise values 0..20: the gap of 130 exceeds four times their range


def plateaus(n_samples, seed):
    """3 n pixels: every sample lies on one of two plateaus (runs of random length), plus noise narrower than the gap."""
    rs = np.random.RandomState(seed)
    side = np.zeros(n_samples, np.int64)
    i, s = 0, int(rs.randint(2))
    while i < n_samples:
        run = int(rs.randint(1, max(2, n_samples // 6 + 2)))
        side[i:i + run] = s
        i, s = i + run, 1 - s
    if n_samples >= 2 and side.min() == side.max():
        side[n_samples // 2:] = 1 - side[0]  # both plateaus are present
    base = np.where(side == 1, PLATEAU_HIGH, PLATEAU_LOW)[:, None]
    return (base + rs.randint(0, PLATEAU_NOISE, size=(n_samples, 3))).astype(np.uint8).reshape(-1)


def plateau_sides(pixels):
    """The plateau of every sample of plateaus(): 0 / 1."""
    return (np.asarray(pixels).reshape(-1, 3)[:, 0] >= (PLATEAU_LOW + PLATEAU_HIGH + PLATEAU_NOISE) // 2).astype(np.uint8)


def noise(n_samples, seed):
    return np.random.RandomState(seed).randint(0, 256, size=3 * n_samples).astype(np.uint8)


def constant(n_samples, value):
    return np.full(3 * n_samples, value, np.uint8)


def bright(n_samples, seed):
    """Near-saturated: 250..255 with a sprinkle of darker runs, so that the column sums pass 2^24 early."""
    rs = np.random.RandomState(seed)
    x = rs.randint(250, 256, size=3 * n_samples)
    dark = rs.rand(n_samples) < 0.04
    x.reshape(-1, 3)[dark] -= 60
    return x.astype(np.uint8)


def tie_case(n_samples, low_at, high_at):
    """Non-constant data whose mean is exact (n a power of two) and has two farthest samples at one distance: (10,10,10)
    everywhere, (0,0,0) at `low_at` and (20,20,20) at `high_at`. With every sample in one cluster, the relocation must take
    the larger of the two indices."""
    assert n_samples & (n_samples - 1) == 0 and low_at != high_at
    x = np.full((n_samples, 3), 10, np.uint8)
    x[low_at], x[high_at] = 0, 20
    return x.reshape(-1)


def uniforms_for(problems, attempts, state=RNG_START):
    """The stream as the operator consumes it: (problems, attempts, 2, 3) float32 and the state after it."""
    u, state = rng_uniform(state, problems * attempts * 6)
    return u.reshape(problems, attempts, 2, 3), state
