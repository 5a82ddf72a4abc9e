"""k-means feature clustering (eval.py --method k-means_feature_clustering, utils.py:171-197), host side: the driver of
vit_ocm_wmsegmentation_amd.cluster (sklearn 1.7.2's KMeans(n_clusters=2, n_init=10, random_state=0).fit replayed) on
its float64 numpy backend, against sklearn's recorded results (tests/golden/kmeans_feature.npz, written by
tools/make_golden_kmeans.py) and, where sklearn is importable, against sklearn live. No GPU needed."""
import numpy as np
import pytest
import torch

from tests.helpers import KMEANS_WIDE_FITS, load_golden
from vit_ocm_wmsegmentation_amd import cluster, synth


def _fit(seed, g, D, S, two):
    return cluster.fit_two_means(cluster.NumpyBackend(
        synth.upsample_token_grid(synth.synth_token_grid(seed, g, D, two), S).numpy()))


@pytest.mark.parametrize("name", list(synth.KMEANS_CASES))
def test_driver_reproduces_recorded_sklearn_fit(name):
    gold = load_golden("kmeans_feature")
    seed, g, D, S, two = synth.KMEANS_CASES[name]
    r = _fit(seed, g, D, S, two)
    want = np.unpackbits(gold[f"{name}/labels_bits"])[: S * S]
    assert np.array_equal(r["labels"], want)
    assert abs(r["inertia"] / float(gold[f"{name}/inertia"]) - 1) <= 1e-6
    assert r["n_iter"] == int(gold[f"{name}/n_iter"])
    np.testing.assert_allclose(r["centers"], gold[f"{name}/centers"], rtol=0, atol=1e-5)


# (g, D, S) cycled over the seeds; every third seed a two-region grid
LIVE_SHAPES = [(8, 32, 32), (6, 16, 48), (10, 48, 40), (12, 64, 48)]


@pytest.mark.parametrize("seed", range(200, 224))
def test_driver_matches_live_sklearn(seed):
    pytest.importorskip("sklearn")
    from sklearn.cluster import KMeans
    g, D, S = LIVE_SHAPES[seed % len(LIVE_SHAPES)]
    two = seed % 3 == 0
    kt = synth.upsample_token_grid(synth.synth_token_grid(seed, g, D, two), S)
    f = torch.reshape(kt, (-1, kt.shape[-1]))  # utils.py:173-181 as the reference writes it
    f = (f - torch.mean(f, axis=0)) / torch.std(f, axis=0)
    km = KMeans(n_init=10, n_clusters=2, random_state=0).fit(f)
    r = _fit(seed, g, D, S, two)
    assert np.array_equal(r["labels"], km.labels_)
    assert abs(r["inertia"] / km.inertia_ - 1) <= 1e-6
    assert r["n_iter"] == km.n_iter_


@pytest.mark.parametrize("name", list(KMEANS_WIDE_FITS))
def test_driver_matches_live_sklearn_at_model_widths(name):
    """The two-region grids at the ViT-T and ViT-B widths that tests/test_cluster_shapes_gpu.py fits on the device."""
    pytest.importorskip("sklearn")
    from sklearn.cluster import KMeans
    seed, g, D, S = KMEANS_WIDE_FITS[name]
    kt = synth.upsample_token_grid(synth.synth_token_grid(seed, g, D, True), S)
    f = torch.reshape(kt, (-1, kt.shape[-1]))
    f = (f - torch.mean(f, axis=0)) / torch.std(f, axis=0)
    for n_init in (10, 3):  # sklearn's default call, and the three initialisations the device test runs
        km = KMeans(n_init=n_init, n_clusters=2, random_state=0).fit(f)
        r = cluster.fit_two_means(cluster.NumpyBackend(kt.numpy()), n_init=n_init)
        assert np.array_equal(r["labels"], km.labels_)
        assert abs(r["inertia"] / km.inertia_ - 1) <= 1e-6
        assert r["n_iter"] == km.n_iter_


def test_same_clustering_rule():
    a = np.array([0, 0, 1, 1], np.int32)
    assert cluster.is_same_clustering(a, a)
    assert cluster.is_same_clustering(a, 1 - a)
    assert not cluster.is_same_clustering(a, np.array([0, 1, 1, 1], np.int32))


def test_empty_cluster_is_an_error():
    class Stuck(cluster.NumpyBackend):
        def lloyd(self, centers, labels_old=None, assign_only=False):
            labels, new, info = super().lloyd(centers, labels_old, assign_only)
            info[6] = 1.0
            return labels, new, info
    b = Stuck(np.random.RandomState(0).standard_normal((16, 8)).astype(np.float32))
    with pytest.raises(cluster.EmptyClusterError):
        cluster.fit_two_means(b, n_init=1)


def test_argument_checks():
    from vit_ocm_wmsegmentation_amd.eval import segment_images
    from vit_ocm_wmsegmentation_amd.utils import kmeans_feature
    with pytest.raises(NotImplementedError):
        kmeans_feature(None, torch.zeros(1, 4, 4, 8), save=True)
    with pytest.raises(ValueError):  # crops (5-D input): refused before any device work
        segment_images(None, torch.zeros(1, 4, 3, 16, 16), method="k-means_feature_clustering")
    with pytest.raises(ValueError):  # non-square images, hence a non-square token grid
        segment_images(None, torch.zeros(1, 3, 16, 32), method="k-means_feature_clustering")
    with pytest.raises(ValueError):  # rows that are not an S x S pixel grid
        kmeans_feature(None, torch.zeros(1, 3, 5, 8))
    with pytest.raises(ValueError):  # the other host methods of eval.py stay refused
        segment_images(None, torch.zeros(1, 3, 16, 16), method="chan-vese")
