"""Times eval.py's k-means feature clustering at S = 384, D = 384 (ViT-S/8 keys on a 384^2 image):
  * the device phases of one image separately — feature prep (key upsample + z-score), k-means++ and Lloyd per
    initialisation (with its iteration count) — with device events around synchronised work;
  * eval.segment_images(..., "k-means_feature_clustering") per image for ViT-S/8 at 384^2 (synthetic weights);
  * sklearn's KMeans(n_clusters=2, n_init=10, random_state=0).fit on the same matrix on this machine's CPUs (threads capped
    by OMP_NUM_THREADS), when sklearn is importable.
Prints one JSON object; whatever could not run is reported as "not measured".
    python tools/bench_kmeans.py [--images 2] [--no-sklearn]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vit_ocm_wmsegmentation_amd import cluster, synth  # noqa: E402

S, G, H, HD = 384, 48, 6, 64


def _timed(fn):
    """(result, device ms) of fn() between two events, the device idle before and after."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def device_phases(dev):
    gen = torch.Generator().manual_seed(7)
    qkv = torch.randn((3, 1, H, G * G + 1, HD), generator=gen)
    qkv[1, :, :, 1:] += torch.randn((1, H, 1, HD), generator=gen) * torch.linspace(-1, 1, G * G)[None, None, :, None]
    qkv = qkv.to(dev)
    X = cluster.key_features(qkv, 0, S)
    _, t_feat = _timed(lambda: cluster.key_features(qkv, 0, S, out=X))
    b = cluster.DeviceBackend(X)
    stats, t_z = _timed(b.zscore)
    tol = float(np.mean(stats[3])) * cluster.TOL
    rs = np.random.RandomState(0)
    inits = []
    for _ in range(cluster.N_INIT):
        centers, t_pp = _timed(lambda: cluster.kmeans_plusplus(b, rs))
        (labels, inertia, _, n_iter), t_ll = _timed(lambda: cluster.lloyd_single(b, centers, tol))
        inits.append(dict(kmeanspp_ms=round(t_pp, 3), lloyd_ms=round(t_ll, 3), lloyd_iters=n_iter,
                          lloyd_ms_per_iter=round(t_ll / (n_iter + 1), 3), inertia=inertia))
    host = X.cpu().numpy()
    return host, dict(feature_upsample_ms=round(t_feat, 3), zscore_ms=round(t_z, 3),
                      kmeanspp_ms_total=round(sum(i["kmeanspp_ms"] for i in inits), 3),
                      lloyd_ms_total=round(sum(i["lloyd_ms"] for i in inits), 3),
                      lloyd_iters_total=sum(i["lloyd_iters"] for i in inits), per_init=inits,
                      x_bytes=S * S * H * HD * 4)


def segment_per_image(dev, images):
    import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
    from vit_ocm_wmsegmentation_amd.eval import segment_images
    model = vits.vit_small(patch_size=8, num_classes=0)
    model.load_state_dict(synth.synth_arch_state_dict("vit_small", 8, seed=0, variant="sharp", img_size=224), strict=True)
    model = model.eval().to(dev)
    x = synth.synth_tiles(images, S, seed=4321).to(dev)
    segment_images(model, x[:1], method="k-means_feature_clustering")  # warm-up
    _, ms = _timed(lambda: segment_images(model, x, method="k-means_feature_clustering"))
    return round(ms / images, 3)


def sklearn_fit(host):
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        return "not measured (sklearn not importable)"
    t = time.perf_counter()
    km = KMeans(n_init=10, n_clusters=2, random_state=0).fit(host)
    return dict(ms=round((time.perf_counter() - t) * 1e3, 1), n_iter=int(km.n_iter_), inertia=float(km.inertia_),
                threads=os.environ.get("OMP_NUM_THREADS", "default"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    out = dict(S=S, D=H * HD)
    if not torch.cuda.is_available():
        out.update(device="not measured (no HIP device)", segment_images_ms_per_image="not measured (no HIP device)",
                   sklearn_cpu="not measured (no device matrix)")
        print(json.dumps(out))
        return
    dev = torch.device("cuda:0")
    out["gpu"] = torch.cuda.get_device_name(0)
    host, out["device"] = device_phases(dev)
    out["segment_images_ms_per_image"] = segment_per_image(dev, a.images)
    # the same z-scored, centred matrix the device clustered (sklearn's own centring then subtracts ~0)
    out["sklearn_cpu"] = "not measured (--no-sklearn)" if a.no_sklearn else sklearn_fit(host)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
