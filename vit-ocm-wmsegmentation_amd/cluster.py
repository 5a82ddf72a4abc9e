"""k-means feature clustering of eval.py's `k-means_feature_clustering` method (reference eval.py:185-202,
utils.py:171-197) with the row-wise work on the device.

The reference clusters the z-scored key features of the last block, upsampled to the image size, with
`sklearn.cluster.KMeans(n_clusters=2, n_init=10, random_state=0).fit`. `fit_two_means` replays that call of sklearn 1.7.2
step by step (sklearn is never imported here):

  _tolerance          tol = mean(var(X, axis=0)) * 1e-4, from the column statistics of the z-score pass
  centring            X -= X.mean(axis=0) (fp32), the mean added back to the centres at the end
  _kmeans_plusplus    one RandomState(0) shared in order by the ten initialisations; first centre
                      choice(n, p=ones / n); 2 + int(log(2)) = 2 local trials drawn with uniform(size=2) * pot
                      and searchsorted on the fp64 cumulative sum of the fp32 closest distances
  _kmeans_single_lloyd  max_iter 300, strict convergence when no label changed, else stop once the summed squared
                      centre shift is <= tol; a final assignment against the last centres for labels and inertia
  best run            kept when inertia < best_inertia and the labelling is not the same clustering as the best one

The driver talks to a narrow backend: `zscore`, `dist`, `lloyd` and the host copies they need. `DeviceBackend` runs
the HIP kernels of kernels_cluster.hip on an [S*S][D] fp32 matrix on the device; `NumpyBackend` is the same
arithmetic in float64 numpy (tests use it to hold the driver against sklearn without a GPU). Distances and cluster sums
are fp64 on both; sklearn's are fp32 GEMMs, so a pixel within rounding of the decision boundary can land on the other
side (measured in DESIGN.md 3.17).
"""
import numpy as np

N_CLUSTERS = 2
N_INIT = 10
MAX_ITER = 300
TOL = 1e-4


class EmptyClusterError(RuntimeError):
    """A Lloyd step left a cluster without rows (sklearn relocates such a cluster; with two clusters seeded by k-means++
    it does not happen, and this path refuses rather than diverge from sklearn silently)."""


# ---- backends ------------------------------------------------------------------------------------------------------------
class NumpyBackend:
    """float64 numpy arithmetic over an fp32 [n][D] matrix: the reference the device kernels are tested against.
    Distances use the fp64 expansion ||x||^2 - 2 x.c + ||c||^2 (a BLAS GEMM, for speed); its rounding is ~1e-13 of the
    distance, far below the fp32 rounding the comparison with sklearn allows for."""

    def __init__(self, features):
        self.X = np.array(features, dtype=np.float32).reshape(-1, np.shape(features)[-1])
        self.n, self.dim = self.X.shape
        self._x64 = None

    def zscore(self):
        x64 = self.X.astype(np.float64)
        mean = x64.mean(axis=0)
        std = np.sqrt(((x64 - mean) ** 2).sum(axis=0) / (self.n - 1))
        z = (self.X - mean.astype(np.float32)) / std.astype(np.float32)
        cmean = z.astype(np.float64).mean(axis=0).astype(np.float32)
        self.X = z - cmean
        self._x64 = self.X.astype(np.float64)
        self._xx = (self._x64 ** 2).sum(axis=1)
        return np.stack([mean, std, cmean.astype(np.float64), self._x64.var(axis=0)])

    def row(self, i):
        return self.X[int(i)].copy()

    def _sq_dist(self, centers):
        if self._x64 is None:
            self._x64 = self.X.astype(np.float64)
            self._xx = (self._x64 ** 2).sum(axis=1)
        c = np.atleast_2d(np.asarray(centers, dtype=np.float64))
        return np.maximum(self._xx[None, :] - 2.0 * (c @ self._x64.T) + (c ** 2).sum(axis=1)[:, None], 0.0)

    def dist(self, cand, closest=None):
        d = self._sq_dist(cand)
        return d if closest is None else np.minimum(closest[None, :], d)

    def to_host(self, a):
        return np.asarray(a)

    def lloyd(self, centers, labels_old=None, assign_only=False):
        d = self._sq_dist(centers)
        labels = (d[1] < d[0]).astype(np.int32)
        info = np.zeros(7)
        info[0] = np.where(labels == 1, d[1], d[0]).sum()
        info[2] = labels.sum()
        info[1] = self.n - info[2]
        info[5] = 1.0 if labels_old is None or np.any(labels != labels_old) else 0.0
        info[6] = float((info[1] == 0) + (info[2] == 0))
        if assign_only:
            return labels, None, info
        sums = np.stack([self._x64[labels == j].sum(axis=0) for j in range(2)])
        cnt = info[1:3]
        new = np.where(cnt[:, None] > 0, sums / np.maximum(cnt, 1)[:, None], 0.0).astype(np.float32)
        info[3:5] = ((new.astype(np.float64) - np.asarray(centers, np.float64)) ** 2).sum(axis=1)
        return labels, new, info


class DeviceBackend:
    """The HIP kernels over X, a contiguous fp32 (n, D) tensor on the device that this backend standardises in place."""

    def __init__(self, X):
        import torch

        from . import _lib
        from .engine import _require_hip
        _require_hip(X, "X")
        if X.dtype != torch.float32 or X.dim() != 2 or not X.is_contiguous():
            raise ValueError(f"X must be a contiguous float32 (n, D) tensor, got {X.dtype} {tuple(X.shape)}")
        self.n, self.dim = X.shape
        S = int(round(self.n ** 0.5))
        if S * S != self.n:
            raise ValueError(f"X has {self.n} rows: not a square S x S pixel grid")
        self.S, self.X, self.torch, self._lib = S, X, torch, _lib
        self.lib = _lib.load()
        self.dev = X.device
        ws = max(self.lib.ocm_kmeans_zscore_workspace_bytes(S, self.dim),
                 self.lib.ocm_kmeans_lloyd_workspace_bytes(S, self.dim))
        self.ws = torch.empty(max(ws, 8), dtype=torch.uint8, device=self.dev)

    def _call(self, name, *args):
        from .engine import _stream
        with self.torch.cuda.device(self.dev):
            self._lib.check(getattr(self.lib, name)(*args, _stream()))

    def _up(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)

    def zscore(self):
        from .engine import _p
        stats = self.torch.empty((4, self.dim), dtype=self.torch.float64, device=self.dev)
        self._call("ocm_op_kmeans_zscore", _p(self.X), self.S, self.dim, _p(stats), _p(self.ws), self.ws.numel())
        return stats.cpu().numpy()

    def row(self, i):
        return self.X[int(i)].cpu().numpy()

    def dist(self, cand, closest=None):
        from .engine import _p
        c = self._up(np.atleast_2d(cand), np.float32)
        out = self.torch.empty((c.shape[0], self.n), dtype=self.torch.float64, device=self.dev)
        self._call("ocm_op_kmeans_dist", _p(self.X), self.S, self.dim, _p(c), c.shape[0], _p(closest), _p(out))
        return out

    def to_host(self, a):
        return a.cpu().numpy()

    def lloyd(self, centers, labels_old=None, assign_only=False):
        from .engine import _p
        t = self.torch
        c = self._up(centers, np.float32)
        labels = t.empty(self.n, dtype=t.int32, device=self.dev)
        new = None if assign_only else t.empty((2, self.dim), dtype=t.float32, device=self.dev)
        info = t.empty(7, dtype=t.float64, device=self.dev)
        self._call("ocm_op_kmeans_lloyd", _p(self.X), self.S, self.dim, _p(c), _p(labels_old), _p(labels), _p(new),
                   _p(None), _p(info), int(bool(assign_only)), _p(self.ws), self.ws.numel())
        return labels, (None if new is None else new.cpu().numpy()), info.cpu().numpy()


# ---- sklearn 1.7.2's KMeans(n_clusters=2, n_init=10, random_state=0).fit, replayed ------------------------------------------
def kmeans_plusplus(backend, random_state):
    """_kmeans_plusplus for two clusters (unit sample weights). Returns the (2, D) fp32 initial centres."""
    n = backend.n
    sw = np.ones(n, dtype=np.float32)
    n_local_trials = 2 + int(np.log(N_CLUSTERS))
    center_id = random_state.choice(n, p=sw / sw.sum())
    centers = np.empty((N_CLUSTERS, backend.dim), dtype=np.float32)
    centers[0] = backend.row(center_id)
    closest_dev = backend.dist(centers[0][None])[0]
    closest = backend.to_host(closest_dev).astype(np.float32)  # sklearn's distances are fp32
    current_pot = closest[None, :] @ sw
    for c in range(1, N_CLUSTERS):
        rand_vals = random_state.uniform(size=n_local_trials) * current_pot
        candidate_ids = np.searchsorted(np.cumsum(sw * closest, dtype=np.float64), rand_vals)
        np.clip(candidate_ids, None, n - 1, out=candidate_ids)
        cand = np.stack([backend.row(i) for i in candidate_ids])
        d_dev = backend.dist(cand, closest_dev)
        d = backend.to_host(d_dev).astype(np.float32)
        candidates_pot = d @ sw.reshape(-1, 1)
        best = int(np.argmin(candidates_pot))
        current_pot = candidates_pot[best]
        closest_dev, closest = d_dev[best], d[best]
        centers[c] = cand[best]
    return centers


def lloyd_single(backend, centers, tol, max_iter=MAX_ITER):
    """_kmeans_single_lloyd: (labels backend array, inertia, centres (2, D) fp32, n_iter)."""
    labels_old = None
    for i in range(max_iter):
        labels, new, info = backend.lloyd(centers, labels_old)
        if info[6]:
            raise EmptyClusterError(f"Lloyd iteration {i} left {int(info[6])} cluster(s) empty")
        centers = new
        if labels_old is not None and info[5] == 0:
            break  # strict convergence
        if info[3] + info[4] <= tol:
            break
        labels_old = labels
    # labels and inertia against the final centres: sklearn's closing E-step when convergence was not strict; after a
    # strict convergence the centres did not move and the assignment repeats the last labels
    labels, _, info = backend.lloyd(centers, None, assign_only=True)
    return labels, float(info[0]), centers, i + 1


def is_same_clustering(labels1, labels2):
    """sklearn's _is_same_clustering: every label of labels1 maps to one label of labels2."""
    for a in range(N_CLUSTERS):
        vals = labels2[labels1 == a]
        if vals.size and np.any(vals != vals[0]):
            return False
    return True


def fit_two_means(backend, n_init=N_INIT, random_state=0, record=None):
    """KMeans(n_clusters=2, n_init=n_init, random_state=random_state).fit on the backend's matrix (standardised first, as
    kmeans_feature does). Returns dict(labels=host int32 (n,), inertia, centers (2, D) fp32 in the z-scored frame,
    n_iter, stats). `record`, when a list, receives each initialisation's (inertia, n_iter)."""
    stats = backend.zscore()
    tol = float(np.mean(stats[3])) * TOL
    rs = np.random.RandomState(random_state)
    best = None
    for _ in range(n_init):
        centers = kmeans_plusplus(backend, rs)
        labels, inertia, centers, n_iter = lloyd_single(backend, centers, tol)
        if record is not None:
            record.append((inertia, n_iter))
        if best is None:
            best = (backend.to_host(labels), inertia, centers, n_iter)
        elif inertia < best[1]:
            host = backend.to_host(labels)
            if not is_same_clustering(host, best[0]):
                best = (host, inertia, centers, n_iter)
    labels, inertia, centers, n_iter = best
    return dict(labels=labels.astype(np.int32), inertia=inertia, centers=centers + stats[2].astype(np.float32),
                n_iter=n_iter, stats=stats)


# ---- device feature map ------------------------------------------------------------------------------------------------
def key_features(qkv, image, size, out=None):
    """X (size*size, D) fp32 on the device: the keys of the patch tokens of `image` in the last block's qkv
    (3, B, H, N, hd) in channel order (head, hd), bilinearly upsampled (align_corners=False) from the square token grid to
    size x size — eval.py:189-199 without the host round trip. `out` is reused when given."""
    import torch

    from . import _lib
    from .engine import _p, _require_hip, _stream
    _require_hip(qkv, "qkv")
    if qkv.dim() != 5 or qkv.shape[0] != 3 or qkv.dtype != torch.float32:
        raise ValueError(f"expected a float32 (3, B, H, N, hd) qkv tensor, got {qkv.dtype} {tuple(qkv.shape)}")
    qkv = qkv.contiguous()
    _, B, H, N, hd = qkv.shape
    g = int(round((N - 1) ** 0.5))
    if g * g != N - 1:
        raise ValueError(f"{N - 1} patch tokens do not form a square token grid")
    D = H * hd
    if out is None:
        out = torch.empty((size * size, D), dtype=torch.float32, device=qkv.device)
    elif tuple(out.shape) != (size * size, D) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 ({size * size}, {D}) tensor")
    with torch.cuda.device(qkv.device):
        _lib.check(_lib.load().ocm_op_kmeans_features(_p(qkv), B, H, N, hd, int(image), g, int(size), _p(out),
                                                      _stream()))
    return out
