#!/usr/bin/env python3
"""What the Swin backbone outputs cost (Swin-T 224^2, batch 256, split-bf16, one MI355X). Development tool, GPU box only.

    python tools/bench_swin_outputs.py [--batch 256] [--steps 10] [--precision bf16x3]

Times, with HIP events around `steps` forwards after a warm-up (output buffers are allocated per call by swin.py, as a user's
call would: the caching allocator serves them after the first call):
  plain        model(pixel_values)
  hidden       ... output_hidden_states=True              (5 token-major copies + 5 (B, C, H, W) transposes)
  last_blocks  ... output_attentions=[1, 3, 9, 11]        (transformers 5.x's per-stage maps; layers 0 .. 3 leave their fused
                                                           attention kernels)
  all_layers   ... output_attentions=True                 (12 maps, 8.8 MB per image)
and ocm_op_swin_window_probs alone on stage-0 rows (B * 64 windows, 3 heads): its achieved write bandwidth.
Prints one human line per measurement and one JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402
from vit_ocm_wmsegmentation_amd import swin as SW  # noqa: E402
from vit_ocm_wmsegmentation_amd import synth  # noqa: E402
from vit_ocm_wmsegmentation_amd.engine import to_operand  # noqa: E402


def timed(fn, steps, warmup=3):
    """Median and spread of the per-call device time in ms (one HIP event pair per call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--precision", default="bf16x3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = SW.SwinForImageClassification(SW.SwinConfig(num_labels=5))
    model.load_state_dict(synth.synth_swin_state_dict(synth.SWIN_TINY, seed=1))
    model = model.to(dev).eval().set_precision(a.precision)
    x = synth.synth_tiles(a.batch, 224, seed=3).to(dev)
    depths = synth.SWIN_TINY["depths"]
    last_blocks = [sum(depths[:i + 1]) - 1 for i in range(len(depths))]
    runs = {
        "plain": lambda: model(pixel_values=x),
        "hidden": lambda: model(pixel_values=x, output_hidden_states=True),
        "last_blocks": lambda: model(pixel_values=x, output_attentions=last_blocks),
        "all_layers": lambda: model(pixel_values=x, output_attentions=True),
    }
    res = {}
    for name, fn in runs.items():
        med, lo, hi = timed(fn, a.steps)
        res[name] = {"ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3)}
        print(f"swin-tiny 224^2 batch {a.batch} {a.precision} {name}: {med:.2f} ms (min {lo:.2f}, max {hi:.2f}) = "
              f"{a.batch / med * 1e3:.0f} images/s")
        torch.cuda.empty_cache()
    for name in ("hidden", "last_blocks", "all_layers"):
        res[name]["over_plain"] = round(res[name]["ms"] / res["plain"]["ms"], 3)

    # the probabilities kernel alone, stage-0 shape: B x 56 x 56 tokens, 3 heads, window 7
    lib, pc = _lib.load(), _lib.PRECISIONS[a.precision]
    B, H, ws, heads = a.batch, 56, 7, 3
    qkv = to_operand(torch.randn(B * H * H, 3 * 32 * heads, device=dev), pc)
    table = torch.randn((2 * ws - 1) ** 2, heads, device=dev)
    scratch = torch.empty(heads * (4096 + ws ** 4), device=dev)
    out = torch.empty((B * (H // ws) ** 2, heads, ws * ws, ws * ws), device=dev)
    med, lo, hi = timed(lambda: _lib.check(lib.ocm_op_swin_window_probs(pc, qkv.data_ptr(), 3 * 32 * heads, out.data_ptr(),
                                                                        table.data_ptr(), scratch.data_ptr(), B, H, H, ws, 3,
                                                                        heads, torch.cuda.current_stream().cuda_stream)), a.steps)
    nbytes = out.numel() * 4
    res["window_probs_stage0"] = {"ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                                  "write_bytes": nbytes, "write_gbs": round(nbytes / med / 1e6, 1)}
    print(f"ocm_op_swin_window_probs stage 0 (batch {B}, shift 3, {a.precision}): {med:.3f} ms, {nbytes / 1e6:.0f} MB written = "
          f"{nbytes / med / 1e6:.0f} GB/s")
    print(json.dumps({"metric": "Swin-T backbone outputs, ms per forward", "batch": a.batch, "dtype": a.precision, "unit": "ms",
                      "last_blocks": last_blocks, "results": res}))


if __name__ == "__main__":
    main()
