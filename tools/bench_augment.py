"""Times DINO's multi-crop augmentation (dino/utils.py DataAugmentationDINO: utils.pil_resize, kernels_augment.hip) for one
training step's input: 64 decoded tiles of 320 x 320 to two 224 x 224 and eight 96 x 96 views each.
  * host_pillow_*: the same chain through Pillow, image by image (tests/augment_ref.pil_view_chain: crop, BICUBIC resize, flip,
    ImageEnhance / HSV jitter, grey, GaussianBlur, solarize, ToTensor + Normalize), on `--workers` processes (16: what a GPU
    command may use), each taking whole images. Run first, before the device is opened; skipped without Pillow.
  * step_ms: DataAugmentationDINO on pre-drawn tables, device events around the whole call: the 2 + n resample calls (their
    coefficient tables are built on the host inside the call), the two concatenations, two colour calls and two blur calls.
  * step_fresh_draws_wall_ms: the call with its own draws, a host clock around it and a device synchronise.
  * resample_ms: the ten resample calls on prepared plans; color_call_ms / blur_call_ms: the two colour and the two blur calls
    through utils.pil_color / pil_gaussian_blur (their small tables are made and uploaded inside); color_ms / blur_ms: the same
    operators through the C ABI on tables and buffers made beforehand, which is their device time.
Every device figure is the median of `--repeat` runs after `--warmup` runs; the views are checked against the host chain on two
images. Prints one JSON object.
    python tools/bench_augment.py [--repeat 20] [--warmup 3] [--batch 64] [--workers 16]"""
import argparse
import ctypes as C
import json
import multiprocessing
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import augment_ref as A  # noqa: E402
from vit_ocm_wmsegmentation_amd import _lib, utils  # noqa: E402
from vit_ocm_wmsegmentation_amd.dino import utils as DU  # noqa: E402

SIDE, GLOBAL, LOCAL, NLOCAL = 320, 224, 96, 8
_HOST = {}


def _host_image(b):
    """Every view of image b through Pillow; returns a checksum so that nothing is optimised away."""
    tiles, params = _HOST["tiles"], _HOST["params"]
    return sum(float(A.pil_view_chain(tiles[b], view, b, GLOBAL if v < 2 else LOCAL).sum()) for v, view in enumerate(params))


def host_chain(tiles, params, workers):
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        return None
    _HOST.update(tiles=tiles, params=params)
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        pool.map(_host_image, range(min(workers, len(tiles))))  # the workers' imports and first calls
        t0 = time.perf_counter()
        pool.map(_host_image, range(len(tiles)), chunksize=1)
        dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    _host_image(0)
    one = time.perf_counter() - t0
    return {"workers": workers, "host_pillow_step_ms": round(dt * 1e3, 1), "host_pillow_one_image_one_process_ms": round(one * 1e3, 1)}


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
    return round(statistics.median(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()
    B = args.batch
    tiles = np.stack([A.smooth(SIDE, SIDE, seed=b) for b in range(B)])
    aug = DU.DataAugmentationDINO(local_crops_number=NLOCAL, global_size=GLOBAL, local_size=LOCAL,
                                  generator=torch.Generator().manual_seed(1), rng=random.Random(2))
    params = aug.params(B, SIDE, SIDE)
    res = {"batch": B, "tile": SIDE, "views": [GLOBAL] * 2 + [LOCAL] * NLOCAL, "repeat": args.repeat}
    res["launches_per_step"] = {"resample": 2 * (2 + NLOCAL), "concatenate": 2, "color": 2 * 5, "color_memset": 2, "blur": 2 * 2}
    host = host_chain(tiles, params, args.workers)  # before the device is opened: the workers are forked
    res.update(host or {"host_pillow_step_ms": None})
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs a HIP device: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    res["device"] = torch.cuda.get_device_name(0)
    x = torch.from_numpy(tiles).to(dev)

    views = aug(x, params)
    for b in (0, B - 1):  # what is timed is what the host chain computes
        for v in (0, 1, 2 + NLOCAL - 1):
            want = A.view_chain(tiles[b], params[v], b, GLOBAL if v < 2 else LOCAL)
            assert np.array_equal(views[v][b].cpu().numpy().view(np.int32), want.view(np.int32)), (b, v)
    res["step_ms"] = _time(lambda: aug(x, params), args.repeat, args.warmup)
    wall = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aug(x)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["step_fresh_draws_wall_ms"] = round(statistics.median(wall), 3)

    # the stages on their own
    sizes = [GLOBAL] * 2 + [LOCAL] * NLOCAL
    plans = [utils.ResamplePlan(x, (s, s), utils.BICUBIC, crop=v["crops"], hflip=v["hflip"]) for s, v in zip(sizes, params)]
    res["resample_ms"] = _time(lambda: [p.run(x) for p in plans], args.repeat, args.warmup)
    groups = []
    for lo, hi in ((0, 2), (2, 2 + NLOCAL)):
        crops = torch.cat([p.run(x) for p in plans[lo:hi]])
        groups.append((crops, {k: np.concatenate([v[k] for v in params[lo:hi]]) for k in ("ops", "factors", "grey", "radius", "solarize")}))
    res["color_call_ms"] = _time(lambda: [utils.pil_color(c, t["ops"], t["factors"], grey=t["grey"], out=c) for c, t in groups],
                                 args.repeat, args.warmup)
    res["blur_call_ms"] = _time(lambda: [utils.pil_gaussian_blur(c, t["radius"], solarize=np.where(t["solarize"], 128, 256),
                                                                 to_tensor=True, mean=DU.IMAGENET_MEAN, std=DU.IMAGENET_STD)
                                         for c, t in groups], args.repeat, args.warmup)

    # the two operators through the C ABI on tables and buffers made beforehand: device time without the wrappers' host work
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    mean, std = ((C.c_float * 3)(*m) for m in (DU.IMAGENET_MEAN, DU.IMAGENET_STD))
    prepared = []
    for crops, t in groups:
        n, side = crops.shape[0], crops.shape[1]
        flags = np.stack([t["grey"].astype(np.int32), np.zeros(n, np.int32), np.full(n, 128, np.int32)], 1)
        dev_t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (
            t["ops"].astype(np.int32), t["factors"].astype(np.float32), flags, utils.gaussian_blur_table(t["radius"]).view(np.int32),
            np.where(t["solarize"], 128, 256).astype(np.int32))]
        cws = torch.empty(lib.ocm_color_u8_workspace_bytes(n), dtype=torch.uint8, device=dev)
        bws = torch.empty(lib.ocm_gaussian_blur_u8_workspace_bytes(n, side, side), dtype=torch.uint8, device=dev)
        out = torch.empty((n, 3, side, side), dtype=torch.float32, device=dev)
        prepared.append((crops, n, side, dev_t, cws, bws, out))

    def color():
        for crops, n, side, t, cws, _, _ in prepared:
            _lib.check(lib.ocm_op_color_u8(p(crops), p(crops), n, side, side, p(t[0]), p(t[1]), p(t[2]), p(cws), cws.numel(), s()))

    def blur():
        for crops, n, side, t, _, bws, out in prepared:
            _lib.check(lib.ocm_op_gaussian_blur_u8(p(crops), n, side, side, p(t[3]), p(t[4]), None, p(out), C.cast(mean, C.c_void_p),
                                                   C.cast(std, C.c_void_p), p(bws), bws.numel(), s()))

    res["color_ms"] = _time(color, args.repeat, args.warmup)
    res["blur_ms"] = _time(blur, args.repeat, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
