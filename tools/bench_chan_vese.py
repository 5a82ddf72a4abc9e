"""Times utils.chan_vese_level_set (kernels_levelset.hip) with device events on what eval.chan_vese_segment hands it for a batch
of 8 images of 384 x 384: 2 x 8 level sets (blobs plus noise, each image and a dimmed copy standing in for its
attention-weighted version), checkerboard start, the reference's parameters.
  * forced: tol = 0, so that all 16 level sets run the full 200 iterations — ms per call and us per iteration (= per launch);
  * default: tol = 1e-3, every level set stopping on its own — ms per call, the iteration counts, and us per launch over the
    200 launches the call always issues (a stopped image's workgroups return at once);
  * floor: the same 16 level sets cut down to 32 x 32 (one workgroup each), tol = 0 — what 200 dependent launches cost when
    the work in them is next to nothing;
  * the numpy restatement tests/chan_vese_ref.py on the CPU for ONE of these images at the default tol, as a yardstick
    (what a host run of skimage's loop costs per level set).
Every device figure is the median of `--repeat` calls after `--warmup` calls and includes the wrapper's normalisation and
allocations. Prints one JSON object.
    python tools/bench_chan_vese.py [--repeat 10] [--warmup 3]"""
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
from tests import chan_vese_ref as R  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=384)
    ap.add_argument("--images", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chan_vese.py needs a HIP device: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    S, B = args.side, args.images
    imgs = np.stack([R.blobs(S, S, s) for s in range(B)])
    both = np.concatenate([(imgs * np.linspace(0.3, 1.0, S, dtype=np.float32)[None, None, :]).astype(np.uint8), imgs])
    x = torch.from_numpy(both).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "repeat": args.repeat, "level_sets": int(x.shape[0]), "side": S}
    ms = _time(lambda: utils.chan_vese_level_set(x, tol=0.0), args.repeat, args.warmup)
    iters = utils.chan_vese_level_set(x, tol=0.0)[1].cpu().tolist()
    res["forced_200"] = {"ms_per_call": round(ms, 3), "us_per_iteration": round(ms * 1e3 / 200, 2), "iters": iters}
    ms = _time(lambda: utils.chan_vese_level_set(x), args.repeat, args.warmup)
    iters = utils.chan_vese_level_set(x)[1].cpu().tolist()
    res["default_tol"] = {"ms_per_call": round(ms, 3), "us_per_launch": round(ms * 1e3 / 200, 2), "iters": iters}
    small = x[:, :32, :32].contiguous()
    ms = _time(lambda: utils.chan_vese_level_set(small, tol=0.0), args.repeat, args.warmup)
    res["floor_32x32_forced_200"] = {"ms_per_call": round(ms, 3), "us_per_launch": round(ms * 1e3 / 200, 2)}
    t = time.perf_counter()
    ref = R.chan_vese(both[B])
    cpu_ms = (time.perf_counter() - t) * 1e3
    res["cpu_numpy_one_image"] = {"ms": round(cpu_ms, 1), "iters": ref["iters"], "device_iters_same_image": iters[B],
                                  "ms_per_iteration": round(cpu_ms / max(ref["iters"], 1), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
