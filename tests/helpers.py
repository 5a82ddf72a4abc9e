"""Shared test helpers: rebuild a golden case's weights / inputs / oracle config from its seeds."""
import os

import numpy as np

from tests.golden_cases import CASES
from vit_ocm_wmsegmentation_amd import synth

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case_dims(case):
    if "arch" in case:
        return synth.ARCHS[case["arch"]]
    return case["dim"], case["depth"], case["heads"]


def case_state_dict(case):
    D, L, _ = case_dims(case)
    return synth.synth_state_dict(D, L, case["patch"], seed=case["seed"], variant=case["variant"],
                                  img_size=case["img_size"])


def case_inputs(case):
    return [synth.synth_tiles(B, H, W, seed=s) for (B, H, W, s) in case["inputs"]]


def load_golden(name):
    return np.load(os.path.join(GOLD_DIR, name + ".npz"))


def build_module(case, device):
    """The product's nn.Module for a golden case, weights loaded through load_state_dict."""
    from functools import partial

    import torch.nn as nn

    import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
    D, L, H = case_dims(case)
    if "arch" in case:
        model = vits.__dict__[case["arch"]](patch_size=case["patch"], num_classes=0)
    else:
        model = vits.VisionTransformer(img_size=[case["img_size"]], patch_size=case["patch"], embed_dim=D, depth=L,
                                       num_heads=H, mlp_ratio=4, qkv_bias=True,
                                       norm_layer=partial(nn.LayerNorm, eps=1e-6), num_classes=0)
    msg = model.load_state_dict(case_state_dict(case), strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    for p in model.parameters():
        p.requires_grad = False
    return model.eval().to(device)


# ---- k-means operators against float64 numpy (tests/test_cluster_gpu.py, tests/test_cluster_shapes_gpu.py) -----------------
# two-region grids (seed, g, D, S) at the ViT-T and ViT-B widths: the float64 driver against live sklearn on the host, the
# device driver against the float64 driver on the GPU
KMEANS_WIDE_FITS = {"vitt_d192_s64": (311, 8, 192, 64), "vitb_d768_s48": (312, 6, 768, 48)}


def kmeans_matrix(S, D, seed):
    """(S*S, D) fp32 standard normal rows, every column with its own scale in [0.5, 3) and offset in [-5, 5)."""
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((S * S, D)) * rs.uniform(0.5, 3, D) + rs.uniform(-5, 5, D)).astype(np.float32)


def sq_dist64(x, c):
    """||x - c||^2 by direct float64 subtraction, (len(c), len(x)): one centre at a time, the arithmetic of
    ((x64[None] - c64[:, None]) ** 2).sum(-1) without its (k, n, D) temporary."""
    x64, out = np.asarray(x, np.float64), []
    for ck in np.atleast_2d(np.asarray(c, np.float64)):
        d = x64 - ck
        d *= d
        out.append(d.sum(-1))
    return np.stack(out)


def tie_margin(dd):
    """min over rows of |d1 - d0| / (d0 + d1) for the (2, n) float64 distances to two centres: exact label equality is
    only asked of inputs where this is far above fp64 rounding."""
    return float((np.abs(dd[1] - dd[0]) / (dd[0] + dd[1])).min())


def lloyd_reference(x, centers):
    """A Lloyd step in float64: dict(dd (2, n), labels, counts, sums (2, D), inertia_terms (n,))."""
    dd = sq_dist64(x, centers)
    labels = (dd[1] < dd[0]).astype(np.int32)
    x64 = np.asarray(x, np.float64)
    return dict(dd=dd, labels=labels, counts=np.array([(labels == 0).sum(), (labels == 1).sum()], np.float64),
                sums=np.stack([x64[labels == j].sum(0) for j in range(2)]), inertia_terms=np.where(labels == 1, dd[1], dd[0]))


def check_kmeans_dist(b, cand, want, k1_closest=False):
    """DeviceBackend.dist on the candidates `cand` against their float64 distances `want`: all of them without `closest`
    (pairs in the K = 2 kernel, an odd last one in the K = 1 kernel), then cand[1:] min'ed with the distances to cand[0];
    with `k1_closest` the last candidate alone as well (K = 1 with `closest`). Returns the device distances."""
    d = b.to_host(b.dist(cand))
    np.testing.assert_allclose(d, want, rtol=1e-12)
    closest = b.dist(cand[:1])[0]
    dmin = b.to_host(b.dist(cand[1:], closest))
    np.testing.assert_array_equal(dmin, np.minimum(d[0][None], d[1:]))  # the same fp64 sums, min'ed
    if k1_closest:
        np.testing.assert_array_equal(b.to_host(b.dist(cand[-1:], closest)), np.minimum(d[0], d[-1])[None])
    return d


def check_kmeans_lloyd(b, x, centers, ref=None, sum_rtol=None):
    """DeviceBackend.lloyd on x (fp32, or the same values as float64) in full mode (without labels_old, then through the C ABI for the fp64 sums with labels_old = its own
    labels) and in assign-only mode against the new centres, each against float64 numpy. `ref` is lloyd_reference(x, centers)
    when the caller has it. The sums over rows are held to rtol 1e-12 (inertia) and 1e-11 (column sums), the tolerances at a
    few thousand rows; `sum_rtol(terms, base)` may return another one for the terms of a longer reference sum. Returns
    (labels device tensor, new centres)."""
    import ctypes as C

    import torch

    from vit_ocm_wmsegmentation_amd import _lib
    from vit_ocm_wmsegmentation_amd.engine import _p
    ref = ref or lloyd_reference(x, centers)
    sum_rtol = sum_rtol or (lambda terms, base: base)
    dd, want_lab, cnt, sums = ref["dd"], ref["labels"], ref["counts"], ref["sums"]
    labels, new, info = b.lloyd(centers)
    np.testing.assert_array_equal(labels.cpu().numpy(), want_lab)
    np.testing.assert_array_equal(info[1:3], cnt)
    np.testing.assert_allclose(new, (sums / cnt[:, None]).astype(np.float32), rtol=2e-7, atol=1e-6)
    np.testing.assert_allclose(info[0], ref["inertia_terms"].sum(), rtol=sum_rtol(ref["inertia_terms"], 1e-12))
    np.testing.assert_allclose(info[3:5], ((new.astype(np.float64) - centers.astype(np.float64)) ** 2).sum(1), rtol=1e-12)
    assert info[5] == 1.0 and info[6] == 0.0
    # the fp64 sums themselves, through the C ABI
    lib = _lib.load()
    dev, D = b.dev, b.dim
    sums_dev = torch.empty((2, D), dtype=torch.float64, device=dev)
    new_dev = torch.empty((2, D), dtype=torch.float32, device=dev)
    info_dev = torch.empty(7, dtype=torch.float64, device=dev)
    c_dev = torch.tensor(centers, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ocm_op_kmeans_lloyd(_p(b.X), b.S, D, _p(c_dev), _p(labels), _p(labels.clone()), _p(new_dev), _p(sums_dev),
                                       _p(info_dev), 0, _p(b.ws), b.ws.numel(), stream))
    x64 = np.asarray(x, np.float64)
    for j in range(2):
        np.testing.assert_allclose(sums_dev[j].cpu().numpy(), sums[j], rtol=sum_rtol(x64[want_lab == j], 1e-11), atol=1e-9)
    assert float(info_dev[5]) == 0.0  # labels_old == the same assignment: nothing changed
    np.testing.assert_array_equal(new_dev.cpu().numpy(), new)
    np.testing.assert_array_equal(info_dev[:5].cpu().numpy(), info[:5])
    # assign-only: labels and inertia against the given centres
    labels2, none, info2 = b.lloyd(new, labels, assign_only=True)
    assert none is None
    dn = sq_dist64(x, new)
    assert tie_margin(dn) >= 1e-9  # of the inputs of this step: no row within fp64 rounding of the boundary
    lab2 = (dn[1] < dn[0]).astype(np.int32)
    np.testing.assert_array_equal(labels2.cpu().numpy(), lab2)
    np.testing.assert_array_equal(info2[1:3], [(lab2 == 0).sum(), (lab2 == 1).sum()])
    terms2 = np.where(lab2 == 1, dn[1], dn[0])
    np.testing.assert_allclose(info2[0], terms2.sum(), rtol=sum_rtol(terms2, 1e-12))
    assert info2[5] == float(np.any(lab2 != want_lab)) and info2[3] == 0.0 and info2[4] == 0.0
    return labels, new


def check_key_features(qkv, image, S, out=None):
    """cluster.key_features for one image of a (3, B, H, N, hd) device qkv against CPU F.interpolate (eval.py:188-198):
    within 2e-7 of the element plus 2e-7 of max|k|."""
    import torch
    import torch.nn.functional as F

    from vit_ocm_wmsegmentation_amd import cluster
    _, B, H, N, hd = qkv.shape
    g = int(round((N - 1) ** 0.5))
    X = cluster.key_features(qkv, image, S, out=out)
    torch.cuda.synchronize()
    k = qkv[1, image].cpu().transpose(0, 1).reshape(N, H * hd)[1:]  # eval.py:188-195
    kt = k.reshape(1, g, g, H * hd).permute(0, 3, 1, 2)
    want = F.interpolate(kt, size=(S, S), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).reshape(S * S, -1)
    err = (X.cpu() - want).abs()
    assert bool((err <= 2e-7 * want.abs() + 2e-7 * k.abs().max()).all()), float(err.max())
    return X


__all__ = ["CASES", "case_dims", "case_state_dict", "case_inputs", "load_golden", "build_module"]
