"""Writes tests/golden/kmeans_feature.npz: what the reference's k-means feature clustering (utils.py:171-197) returns on
the seeded token grids of synth.KMEANS_CASES. The recipe is the reference's: torch CPU F.interpolate (bilinear,
align_corners=False), torch.mean / torch.std z-score, sklearn KMeans(n_clusters=2, n_init=10, random_state=0).fit.
Run it where sklearn 1.7.2 is importable; the inputs are regenerated from their seeds, the fixture holds only results:
labels_ as packed bits, inertia_, cluster_centers_ and n_iter_ per case."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vit_ocm_wmsegmentation_amd import synth  # noqa: E402


def reference_fit(features):
    """utils.py:172-187 verbatim in effect: (1, S, S, D) -> fitted sklearn KMeans."""
    from sklearn.cluster import KMeans
    f = torch.reshape(features, (-1, features.shape[-1]))
    f = (f - torch.mean(f, axis=0)) / torch.std(f, axis=0)
    return KMeans(n_init=10, n_clusters=2, random_state=0).fit(f)


def main():
    import sklearn
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name, (seed, g, D, S, two) in synth.KMEANS_CASES.items():
        km = reference_fit(synth.upsample_token_grid(synth.synth_token_grid(seed, g, D, two), S))
        out[f"{name}/labels_bits"] = np.packbits(km.labels_.astype(np.uint8))
        out[f"{name}/inertia"] = np.float64(km.inertia_)
        out[f"{name}/centers"] = km.cluster_centers_.astype(np.float32)
        out[f"{name}/n_iter"] = np.int64(km.n_iter_)
        print(f"{name}: inertia {km.inertia_:.6e}, n_iter {km.n_iter_}, cluster 1 holds {km.labels_.mean():.4f}")
    path = os.path.join(ROOT, "tests", "golden", "kmeans_feature.npz")
    np.savez_compressed(path, **out)
    print(f"-> {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes, sklearn {sklearn.__version__})")


if __name__ == "__main__":
    main()
