"""k-means feature clustering on the device (kernels_cluster.hip, cluster.py, utils.kmeans_feature, eval.segment_images
with method "k-means_feature_clustering"): each operator against float64 numpy, run-to-run bit equality, the recorded
sklearn 1.7.2 fits of tests/golden/kmeans_feature.npz, and the whole eval.py chain on ViT-S/8 at 384^2 against the CPU
chain (oracle keys -> torch interpolate -> live sklearn)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import (CASES, build_module, case_state_dict, check_key_features, check_kmeans_dist, check_kmeans_lloyd,
                           kmeans_matrix, load_golden, sq_dist64)
from vit_ocm_wmsegmentation_amd import _lib, cluster, synth
from vit_ocm_wmsegmentation_amd.engine import _p

pytestmark = pytest.mark.gpu


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand_qkv(dev, B=2, H=3, g=12, hd=16, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((3, B, H, g * g + 1, hd), generator=gen).to(dev)


@pytest.mark.parametrize("g,S", [(12, 96), (7, 40), (5, 5), (4, 3)])
def test_features_match_torch_interpolate(dev, lib, g, S):
    qkv = _rand_qkv(dev, g=g)
    for image in range(qkv.shape[1]):
        check_key_features(qkv, image, S)


def test_features_reject_bad_arguments(dev, lib):
    qkv = _rand_qkv(dev)
    X = torch.empty((16, 48), device=dev)
    assert lib.ocm_op_kmeans_features(_p(qkv), 2, 3, 145, 16, 2, 12, 4, _p(X), _s()) == _lib.OCM_EINVAL  # image
    assert lib.ocm_op_kmeans_features(_p(qkv), 2, 3, 146, 16, 0, 12, 4, _p(X), _s()) == _lib.OCM_EINVAL  # grid
    assert lib.ocm_op_kmeans_features(_p(qkv), 2, 3, 145, 16, 0, 12, 0, _p(X), _s()) == _lib.OCM_EINVAL  # S
    assert lib.ocm_op_kmeans_features(None, 2, 3, 145, 16, 0, 12, 4, _p(X), _s()) == _lib.OCM_EINVAL
    d = torch.empty(64, dtype=torch.float64, device=dev)
    assert lib.ocm_op_kmeans_dist(_p(X), 4, 46, _p(X), 1, None, _p(d), _s()) == _lib.OCM_EINVAL  # D % 4
    assert lib.ocm_op_kmeans_dist(_p(X), 0, 48, _p(X), 1, None, _p(d), _s()) == _lib.OCM_EINVAL
    assert lib.ocm_op_kmeans_lloyd(_p(X), 4, 48, None, None, _p(d), _p(X), None, _p(d), 0, _p(d), 512,
                                   _s()) == _lib.OCM_EINVAL


def _matrix(dev, S, D, seed):
    x = kmeans_matrix(S, D, seed)
    return x, torch.from_numpy(x).to(dev)


@pytest.mark.parametrize("S,D", [(48, 64), (37, 384), (9, 4), (20, 1024)])
def test_zscore_against_float64(dev, S, D):
    x, X = _matrix(dev, S, D, 1)
    b = cluster.DeviceBackend(X)
    stats = b.zscore()
    ref = cluster.NumpyBackend(x)
    want = ref.zscore()
    np.testing.assert_allclose(stats[:2], want[:2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(stats[2], want[2], rtol=0, atol=1e-7)  # an fp32 mean of values that sum to ~0
    np.testing.assert_allclose(stats[3], want[3], rtol=1e-5)
    np.testing.assert_allclose(X.cpu().numpy(), ref.X, rtol=0, atol=2e-6)


@pytest.mark.parametrize("S,D", [(48, 64), (37, 384), (9, 4), (20, 1024), (13, 100)])
def test_dist_and_lloyd_against_float64(dev, S, D):
    x, X = _matrix(dev, S, D, 2)
    b = cluster.DeviceBackend(X)
    cand = x[[3, 17, 40]]
    check_kmeans_dist(b, cand, sq_dist64(x, cand))
    check_kmeans_lloyd(b, x, x[[5, 11]])


def test_lloyd_tie_goes_to_cluster_zero(dev):
    x = np.zeros((16, 8), np.float32)
    b = cluster.DeviceBackend(torch.from_numpy(x).to(dev))
    labels, _, info = b.lloyd(np.ones((2, 8), np.float32), assign_only=True)
    assert int(labels.sum()) == 0 and info[1] == 16 and info[2] == 0


def test_reruns_give_the_same_bits(dev):
    x, _ = _matrix(dev, 64, 384, 3)
    outs = []
    for _ in range(2):
        X = torch.from_numpy(x).to(dev)
        b = cluster.DeviceBackend(X)
        stats = b.zscore()
        d = b.to_host(b.dist(x[[1, 2]]))
        labels, new, info = b.lloyd(x[[7, 9]])
        r = cluster.fit_two_means(cluster.DeviceBackend(torch.from_numpy(x).to(dev)), n_init=3)
        outs.append((X.cpu().numpy(), stats, d, labels.cpu().numpy(), new, info, r["labels"], r["inertia"], r["centers"]))
    for a, bb in zip(*outs):
        assert np.array_equal(np.asarray(a), np.asarray(bb))


@pytest.mark.parametrize("name", list(synth.KMEANS_CASES))
def test_kmeans_feature_matches_recorded_sklearn(dev, name):
    from vit_ocm_wmsegmentation_amd.utils import kmeans_feature, kmeans_feature_labels
    gold = load_golden("kmeans_feature")
    seed, g, D, S, two = synth.KMEANS_CASES[name]
    feats = synth.upsample_token_grid(synth.synth_token_grid(seed, g, D, two), S)  # (1, S, S, D) on the host
    want = np.unpackbits(gold[f"{name}/labels_bits"])[: S * S].reshape(S, S).astype(np.int64) * 255
    mask = kmeans_feature(None, feats)
    assert mask.shape == (S, S)
    agree = np.mean(mask == want)
    assert agree >= (1.0 if two else 0.999), agree  # agreement counts polarity: an inverted mask agrees nowhere
    on_dev = feats.to(dev)
    assert np.array_equal(kmeans_feature(None, on_dev), mask)
    assert torch.equal(on_dev.cpu(), feats)  # the caller's features are not modified
    r = kmeans_feature_labels(feats.reshape(S * S, D).to(dev).contiguous())
    assert abs(r["inertia"] / float(gold[f"{name}/inertia"]) - 1) <= 1e-5


def _two_region_images(B, S, seed=11):
    """(B, 3, S, S) gray tiles: a bright disc (a different centre per image) on a darker ground, plus mild noise: a scene
    with one boundary, like the tissue / background split the method is meant for. Uniform-noise tiles give key
    features without cluster structure, where any arithmetic difference moves the k-means boundary."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = []
    for _ in range(B):
        cy, cx = rs.uniform(0.35, 0.65, 2) * S
        disc = ((yy - cy) ** 2 + (xx - cx) ** 2 < (0.25 * S) ** 2).astype(np.float32)
        out.append(0.05 + 0.2 * disc + 0.02 * rs.uniform(size=(S, S)).astype(np.float32))
    g = torch.from_numpy(np.stack(out))[:, None]
    return g.expand(-1, 3, -1, -1).contiguous()


_CPU_CHAIN = {}


def _cpu_chain_mask(case, x):
    """eval.py:185-202 on the CPU: oracle qkv of the last block -> keys -> torch interpolate -> utils.kmeans_feature
    with live sklearn. Computed once per image (precision-independent)."""
    key = float(x.sum())
    if key not in _CPU_CHAIN:
        from sklearn.cluster import KMeans

        from oracle import vit_oracle as O
        sd = case_state_dict(case)
        cfg = O.make_cfg(sd, case["patch"], 6)
        _, attns, qkvs = O.get_intermediate_feat(sd, cfg, x[None], 1)
        q = qkvs[0]
        nb, nh, nt = attns[0].shape[:3]
        k = q[1].transpose(1, 2).reshape(nb, nt, -1)[:, 1:]
        g = int(round((nt - 1) ** 0.5))
        S = x.shape[-1]
        kt = F.interpolate(k.reshape(1, g, g, -1).permute(0, 3, 1, 2), size=(S, S), mode="bilinear",
                           align_corners=False).permute(0, 2, 3, 1)
        f = torch.reshape(kt, (-1, kt.shape[-1]))
        f = (f - torch.mean(f, axis=0)) / torch.std(f, axis=0)
        labels = KMeans(n_init=10, n_clusters=2, random_state=0).fit(f).labels_
        _CPU_CHAIN[key] = labels.reshape(S, S) * 255
    return _CPU_CHAIN[key]


@pytest.mark.parametrize("precision", ["bf16x3", "fp32"])
def test_segment_images_kmeans_vs_cpu_chain(dev, precision):
    """Batch 2 against two calls at batch 1, and image 0 against the CPU chain with live sklearn."""
    from vit_ocm_wmsegmentation_amd.eval import segment_images
    pytest.importorskip("sklearn")
    case = CASES["vits8_384_sharp"]
    model = build_module(case, dev)
    model.set_precision(precision)
    x = _two_region_images(2, 384)
    masks, maps = segment_images(model, x.to(dev), method="k-means_feature_clustering", as_numpy=True)
    assert masks.shape == (2, 384, 384) and masks.dtype == np.uint8 and maps.shape == (2, 384, 384)
    assert set(np.unique(masks)) <= {0, 255}
    for b in range(2):
        one, _ = segment_images(model, x[b:b + 1].to(dev), method="k-means_feature_clustering", as_numpy=True)
        if precision == "fp32":  # fp32 forwards give each image the same bits at any batch size
            assert np.array_equal(one[0], masks[b])
        else:  # split-bf16 forwards do not: keys differ by roundings, a boundary pixel may flip
            assert np.mean(one[0] == masks[b]) >= 0.999
    want = _cpu_chain_mask(case, x[0])
    agree = np.mean(masks[0].astype(np.int64) == want)
    assert agree >= 0.995, agree
