"""Times utils.kmeans_pixels (kernels_kmeans_px.hip) with device events on what eval.kmeans_pixels_segment hands it at 384 x 384:
2 B problems of 49 152 pixel triples (each image and a dimmed copy standing in for its attention-weighted version), 10 attempts,
10 iterations at most, eps 1.0, for B = 1 and B = 8.
  * blobs: two-region images, where an attempt converges in a few iterations;
  * noise: uniform noise, where every attempt runs to the iteration cap — the most a call can cost;
  * score_images(method="k-means_ours") on ViT-S/8 at 384 x 384 for the same B (forward, maps, k-means, scores), next to
    method="otsu" as the cost of everything but the k-means;
  * a host yardstick. OpenCV is not installable here, so cv2.kmeans itself cannot be timed: sklearn.cluster.KMeans(2,
    init="random", n_init=10, max_iter=10) on the same triples of ONE image stands in for it (another implementation of the same
    ten Lloyd runs, not the reference's own call).
Every device figure is the median of `--repeat` calls after `--warmup` calls and includes the wrapper's draws, its copy of the
uniforms and its allocations. No threshold is set on any of them. Prints one JSON object.
    python tools/bench_kmeans_px.py [--repeat 20] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import chan_vese_ref as CV  # noqa: E402
from tests import kmeans_px_ref as R  # noqa: E402
from vit_ocm_wmsegmentation_amd import utils  # noqa: E402


def _time(fn, repeat, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def _pairs(imgs, S):
    """ours_0, image_0, ours_1, ...: the order eval.kmeans_pixels_segment interleaves them in."""
    dim = (imgs * np.linspace(0.3, 1.0, S, dtype=np.float32)[None, None, :]).astype(np.uint8)
    return np.stack([dim, imgs], axis=1).reshape((-1,) + imgs.shape[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=384)
    ap.add_argument("--no-model", action="store_true", help="skip the score_images timings")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans_px.py needs a HIP device: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    S = args.side
    res = {"device": torch.cuda.get_device_name(0), "repeat": args.repeat, "side": S, "samples": S * S // 3}
    for B in (1, 8):
        blobs = np.stack([CV.blobs(S, S, s) for s in range(B)])
        noise = np.stack([R.noise(S * S // 3, 100 + s).reshape(S, S) for s in range(B)])
        for name, imgs in (("blobs", blobs), ("noise", noise)):
            x = torch.from_numpy(_pairs(imgs, S)).to(dev)
            ms = _time(lambda: utils.kmeans_pixels(x), args.repeat, args.warmup)
            iters = utils.kmeans_pixels(x)["iters"].cpu().numpy()
            res[f"operator_B{B}_{name}"] = {"problems": int(x.shape[0]), "ms_per_call": round(ms, 3),
                                            "iters_min_mean_max": [int(iters.min()), round(float(iters.mean()), 2), int(iters.max())]}
    if not args.no_model:
        from tests.helpers import CASES, build_module
        from vit_ocm_wmsegmentation_amd import eval as E
        model = build_module(CASES["vits8_384_sharp"], dev)
        for B in (1, 8):
            g = np.stack([CV.blobs(S, S, s) for s in range(B)])
            x = torch.from_numpy(np.ascontiguousarray(np.repeat((g.astype(np.float32) / np.float32(255))[:, None], 3, axis=1))).to(dev)
            t = torch.from_numpy((g > 128).astype(np.float32)).to(dev)
            res[f"score_images_B{B}"] = {m: round(_time(lambda: E.score_images(model, x, t, method=m), args.repeat, args.warmup), 3)
                                         for m in ("k-means_ours", "otsu")}
    try:
        from sklearn.cluster import KMeans
        Z = CV.blobs(S, S, 0).reshape(-1, 3).astype(np.float32)
        KMeans(2, init="random", n_init=10, max_iter=10, random_state=0).fit(Z)
        t0 = time.perf_counter()
        for k in range(3):
            KMeans(2, init="random", n_init=10, max_iter=10, random_state=k).fit(Z)
        res["cpu_sklearn_stand_in_one_image_ms"] = round((time.perf_counter() - t0) * 1e3 / 3, 2)
    except ImportError:
        res["cpu_sklearn_stand_in_one_image_ms"] = None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
