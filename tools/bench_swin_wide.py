#!/usr/bin/env python3
"""Swin-B / window 12 / 384^2 inference (the swin-base-patch4-window12-384 geometry: embed_dim 128, depths 2 / 2 / 18 / 2, heads
4 / 8 / 16 / 32, synthetic weights) on one MI355X. Development tool, GPU box only.

    python tools/bench_swin_wide.py [--batch 8] [--steps 5] [--precisions bf16x3,bf16,fp32] [--eager-batch 2]

Per precision: ms per forward and images/s (wall clock around `steps` forwards), then the per-class device time of
ocm_prof_begin / ocm_prof_end (HIP events around every launch of the engine, a separate pass) and the window-attention share
of it. Last, the same forward through the fp32 oracle functions (oracle/swin_oracle.py: torch operators) on the same GPU: the
eager yardstick. One human line per row and one JSON line at the end. Reported, not gated."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from oracle import swin_oracle as SO  # noqa: E402
from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402
from vit_ocm_wmsegmentation_amd import swin as SW  # noqa: E402
from vit_ocm_wmsegmentation_amd import synth  # noqa: E402

SWIN_B_W12 = dict(synth.SWIN_TINY, image_size=384, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)


def timed(fn, steps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--precisions", default="bf16x3,bf16,fp32")
    ap.add_argument("--eager-batch", type=int, default=2, help="batch of the oracle's forward (its (nB, heads, 144, 144) scores are fp32)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = SWIN_B_W12
    sd = synth.synth_swin_state_dict(cfg, seed=1)
    hf = SW.SwinConfig(image_size=cfg["image_size"], embed_dim=cfg["embed_dim"], depths=cfg["depths"], num_heads=cfg["num_heads"],
                       window_size=cfg["window_size"], num_labels=cfg["num_labels"])
    x = synth.synth_tiles(a.batch, cfg["image_size"], seed=3).to(dev)
    lib = _lib.load()
    ncls = len(_lib.KERNEL_CLASSES)
    rows = {}
    for precision in a.precisions.split(","):
        model = SW.SwinForImageClassification(hf)
        model.load_state_dict(sd)
        model = model.to(dev).eval().set_precision(precision)
        dt = timed(lambda: model(pixel_values=x), a.steps)
        ms, cnt = (C.c_double * ncls)(), (C.c_int64 * ncls)()
        reps = 2
        _lib.check(lib.ocm_prof_begin(0xFFFFFFFF, reps * 1024))
        for _ in range(reps):
            model(pixel_values=x)
        torch.cuda.synchronize()
        _lib.check(lib.ocm_prof_end(ms, cnt))
        breakdown = {name: {"launches_per_fwd": cnt[i] // reps, "ms_per_fwd": round(ms[i] / reps, 3)}
                     for i, name in enumerate(_lib.KERNEL_CLASSES) if cnt[i]}
        total = sum(v["ms_per_fwd"] for v in breakdown.values())
        share = breakdown.get("attention", {"ms_per_fwd": 0.0})["ms_per_fwd"] / total if total else 0.0
        rows[precision] = {"ms_per_fwd": round(dt * 1e3, 3), "images_per_s": round(a.batch / dt, 1), "device_ms_per_fwd": round(total, 3),
                           "window_attention_share": round(share, 4), "kernel_breakdown": breakdown}
        print(f"swin-b/w12/384 batch {a.batch} {precision}: {dt * 1e3:.2f} ms/forward = {a.batch / dt:.1f} images/s; device "
              f"{total:.2f} ms, window attention {100 * share:.1f} %: "
              + ", ".join(f"{k} {v['ms_per_fwd']:.2f}" for k, v in breakdown.items()))
        del model
    sdd = {k: v.to(dev) for k, v in sd.items()}
    xe = x[:a.eager_batch]
    with torch.device(dev):  # the oracle builds its index and mask tensors with factory calls: on the GPU inside this context
        dte = timed(lambda: SO.swin_forward(sdd, cfg, xe), max(2, a.steps // 2))
    print(f"fp32 oracle (torch operators) on the same GPU, batch {a.eager_batch}: {dte * 1e3:.2f} ms/forward = "
          f"{a.eager_batch / dte:.1f} images/s")
    print(json.dumps({"metric": "Swin-B/window12/384 images/s", "config": {"batch": a.batch, "steps": a.steps}, "rows": rows,
                      "eager_fp32": {"batch": a.eager_batch, "ms_per_fwd": round(dte * 1e3, 3),
                                     "images_per_s": round(a.eager_batch / dte, 1)},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
