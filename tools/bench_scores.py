"""Times utils.mask_scores (kernels_score.hip) with device events on what eval.score_images hands it for a batch of 64 masks of
384 x 384: uint8 masks in {0, 255} (blobs thresholded, so that the classes form regions as a segmentation's do) against float32
0/1 targets, both already on the device.
  * device: one call scores all 64 images — ms per call, us per image, and the bytes the pass reads (5 per pixel) over that time;
    the same for a float32 prediction (8 bytes per pixel);
  * host: the reference's path for the same masks — copy them to the host, then per image the classes > 0.5 as uint8 and
    sklearn's jaccard_score, f1_score, recall_score, precision_score and accuracy_score (utils.py:388-408) — ms for the copy,
    ms per image for the five calls, and roc_auc_score on top (PGT.py:247-275). Skipped (null) where sklearn is not installed;
  * the scores of both sides compared: the five must be equal bit for bit.
Every device figure is the median of `--repeat` calls after `--warmup` calls and includes the wrapper's allocations. The host
side is timed once over `--host-images` images. Prints one JSON object.
    python tools/bench_scores.py [--repeat 20] [--warmup 5] [--images 64] [--side 384] [--host-images 64]"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import chan_vese_ref as CV  # noqa: E402
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


def _device_side(x, t, bytes_per_pixel, repeat, warmup):
    ms = _time(lambda: utils.mask_scores(x, t), repeat, warmup)
    B, pixels = x.shape[0], x[0].numel()
    return {"ms_per_call": round(ms, 4), "us_per_image": round(ms * 1e3 / B, 3),
            "read_GB_per_s": round(B * pixels * bytes_per_pixel / (ms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--side", type=int, default=384)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--host-images", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scores.py needs a HIP device: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    S, B = args.side, args.images
    blobs = np.stack([CV.blobs(S, S, s) for s in range(B)])
    masks = ((blobs > 120) * np.uint8(255)).astype(np.uint8)
    targets = (np.roll(blobs, 3, axis=2) > 128).astype(np.float32)  # the same regions, shifted: imperfect predictions
    x, t = torch.from_numpy(masks).to(dev), torch.from_numpy(targets).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "repeat": args.repeat, "images": B, "side": S,
           "device_u8_mask": _device_side(x, t, 5, args.repeat, args.warmup),
           "device_f32_prediction": _device_side(x.to(torch.float32) / 255, t, 8, args.repeat, args.warmup)}
    scores = utils.mask_scores(x, t)[0].cpu().numpy()
    try:
        import sklearn.metrics as M
    except ImportError:
        res["host_sklearn"] = None
        print(json.dumps(res))
        return
    n = min(args.host_images, B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_masks, host_targets = (x / 255).cpu().numpy(), t.cpu().numpy()  # eval.py's output / 255, then .cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    five, auc_ms = [], 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        for b in range(n):
            y_true = (host_targets[b] > 0.5).astype(np.uint8).reshape(-1)
            y_pred = (host_masks[b] > 0.5).astype(np.uint8).reshape(-1)
            five.append([M.jaccard_score(y_true, y_pred), M.f1_score(y_true, y_pred), M.recall_score(y_true, y_pred),
                         M.precision_score(y_true, y_pred), M.accuracy_score(y_true, y_pred)])
        five_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        aucs = [M.roc_auc_score((host_targets[b] > 0.5).astype(np.uint8).reshape(-1),
                                (host_masks[b] > 0.5).astype(np.uint8).reshape(-1)) for b in range(n)]
        auc_ms = (time.perf_counter() - t0) * 1e3
    five = np.array(five, np.float64)
    res["host_sklearn"] = {"images": n, "copy_ms_all_images": round(copy_ms, 3), "five_scores_ms_per_image": round(five_ms / n, 2),
                           "roc_auc_ms_per_image": round(auc_ms / n, 2), "cpus": os.cpu_count(),
                           "five_scores_bit_equal": bool(np.array_equal(five.view(np.int64), scores[:n, :5].view(np.int64))),
                           "max_auc_difference": float(np.abs(np.array(aucs) - scores[:n, 5]).max())}
    res["images_per_second"] = {"device": round(B / (res["device_u8_mask"]["ms_per_call"] * 1e-3)),
                                "host": round(n / ((copy_ms * n / B + five_ms) * 1e-3), 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
