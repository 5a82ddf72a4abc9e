"""Time stochastic depth on the ViT training path (kernels_drop_path.hip) on one MI355X. Two steps, each run under its own time
limit:

  timeout -k 10 240 python tools/bench_drop_path.py ops  [--batch 64] [--tokens 197] [--dim 384] [--iters 40] [--rounds 7]
  timeout -k 10 400 python tools/bench_drop_path.py step [--batch 64] [--steps 6] [--warmup 2] [--rounds 3] [--precision bf16x3]

ops   the two operators at batch x tokens rows of dim (12 608 x 384: ViT-S/16, B = 64) in the three output kinds, beside the chain
      of existing operators they replace: forward ocm_op_swin_drop_path -> ocm_op_layernorm (two launches, five passes over the
      rows: x, branch in, sum out, sum in, y out, where the fused kernel makes four), backward ocm_op_swin_drop_path_backward ->
      ocm_op_cast_bf16 / ocm_op_cast_split (four passes where the fused kernel makes three; fp32 needs no cast: one launch each).
      Every candidate walks `--sets` buffer sets (together larger than the 256 MB Infinity Cache) so that rows come from HBM; a
      timing is `--iters` launches between two device events; candidates alternate within a round; the figure is the median
      over `--rounds` and the spread is max - min of the rounds. GB/s counts the bytes the algorithm needs.
step  the training forward + backward of tools/bench_dino.py's backbone (vit_small(16), enable_training(); 2 x 224^2 + 8 x 96^2
      crops of `--batch` images in two resolution groups) at drop_path_rate 0 and 0.1 on the same build, the two models
      alternating within a round, and the share of the 0.1 step spent in draw_drop_path_scales (2 (depth - 1) torch.rand tables
      per group), timed on its own with the same events.

Nothing here is a gate. One JSON line per step."""
import argparse
import json
import os
import socket
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_ocm_wmsegmentation_amd  # noqa: E402,F401
from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as VT  # noqa: E402

KINDS = {"f32": (_lib.OCM_LN_F32, torch.float32, 4), "bf16": (_lib.OCM_LN_BF16, torch.bfloat16, 2),
         "split": (_lib.OCM_LN_SPLIT, torch.int32, 4)}
PRECS = {"fp32": (None, 0), "bf16": (torch.bfloat16, 2), "bf16x3": (torch.int32, 4)}
EPS = 1e-6


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def _alternate(cands, iters, rounds):
    """{name: (median us, spread us)}: every round times each candidate once, in turn."""
    for fn in cands.values():  # warm-up: code objects, every buffer set touched
        _time(fn, iters)
    times = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            times[k].append(_time(fn, iters))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in times.items()}


def ops(args):
    lib, dev = _lib.load(), torch.device("cuda:0")
    B, N, D = args.batch, args.tokens, args.dim
    rows, S = B * N, args.sets
    p = lambda t: t.data_ptr()  # noqa: E731
    x = [torch.randn(rows, D, device=dev) + 1.0 for _ in range(S)]
    br = [torch.randn(rows, D, device=dev) for _ in range(S)]
    out = [torch.empty(rows, D, device=dev) for _ in range(S)]
    scale = (torch.rand(B, device=dev) < 0.9).float() / 0.9
    gamma, beta = torch.randn(D, device=dev), torch.randn(D, device=dev)
    row_bytes = rows * D
    result = dict(step="ops", box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), rows=rows, dim=D, sets=S,
                  set_mb=round(4 * row_bytes * 4 / 2 ** 20, 1), iters=args.iters, rounds=args.rounds, forward={}, backward={})
    for name, (kind, dtype, width) in KINDS.items():
        y = [torch.empty(rows, D, dtype=dtype, device=dev) for _ in range(S)]

        def fused(i, kind=kind, y=y):
            j = i % S
            _lib.check(lib.ocm_op_drop_path_layernorm(p(x[j]), p(br[j]), p(scale), p(gamma), p(beta), p(out[j]), p(y[j]), kind, B, N,
                                                      D, EPS, None))

        def chain(i, kind=kind, y=y):
            j = i % S
            _lib.check(lib.ocm_op_swin_drop_path(p(x[j]), p(br[j]), p(scale), p(out[j]), B, N, D, None))
            _lib.check(lib.ocm_op_layernorm(p(out[j]), p(gamma), p(beta), p(y[j]), kind, rows, D, EPS, None))

        t = _alternate({"fused": fused, "chain": chain}, args.iters, args.rounds)
        need = row_bytes * (3 * 4 + width)  # x, branch in; x_out, y out
        result["forward"][name] = dict(fused_us=round(t["fused"][0], 2), fused_spread_us=round(t["fused"][1], 2),
                                       chain_us=round(t["chain"][0], 2), chain_spread_us=round(t["chain"][1], 2),
                                       fused_gbs=round(need / t["fused"][0] / 1e3, 1), fused_bytes=need,
                                       chain_bytes=need + row_bytes * 4)
        del y
    for name, (dtype, width) in PRECS.items():
        pc = _lib.PRECISIONS[name]
        d_op = [torch.empty(rows, D, dtype=dtype, device=dev) for _ in range(S)] if dtype is not None else None
        cast = lib.ocm_op_cast_bf16 if name == "bf16" else lib.ocm_op_cast_split

        def fused(i, pc=pc, d_op=d_op):
            j = i % S
            _lib.check(lib.ocm_op_drop_path_backward(pc, p(x[j]), p(scale), p(out[j]), p(d_op[j]) if d_op else None, B, N, D, None))

        def chain(i, d_op=d_op, cast=cast):
            j = i % S
            _lib.check(lib.ocm_op_swin_drop_path_backward(p(x[j]), p(scale), p(out[j]), B, N, D, None))
            if d_op:
                _lib.check(cast(p(out[j]), p(d_op[j]), rows * D, None))

        t = _alternate({"fused": fused, "chain": chain}, args.iters, args.rounds)
        need = row_bytes * (2 * 4 + width)
        result["backward"][name] = dict(fused_us=round(t["fused"][0], 2), fused_spread_us=round(t["fused"][1], 2),
                                        chain_us=round(t["chain"][0], 2), chain_spread_us=round(t["chain"][1], 2),
                                        fused_gbs=round(need / t["fused"][0] / 1e3, 1), fused_bytes=need,
                                        chain_bytes=need + (row_bytes * 4 if width else 0))
        del d_op
    print(json.dumps(result), flush=True)


def step(args):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    groups = [torch.rand(2 * args.batch, 3, 224, 224, device=dev, generator=gen) * 0.3,
              torch.rand(8 * args.batch, 3, 96, 96, device=dev, generator=gen) * 0.3]
    base = VT.vit_small(16)
    models = {}
    for rate in (0.0, 0.1):
        bb = VT.vit_small(16, drop_path_rate=rate).set_precision(args.precision)
        bb.load_state_dict(base.state_dict())
        models[rate] = bb.enable_training().to(dev).train()

    def run(rate):
        bb = models[rate]
        feats = torch.cat([bb(g) for g in groups])
        feats.backward(torch.ones_like(feats))
        bb.zero_grad(set_to_none=True)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def draw():
        for g in groups:
            VT.draw_drop_path_scales(models[0.1], g.shape[0], dev)

    cands = {"rate_0": lambda: run(0.0), "rate_0.1": lambda: run(0.1), "draw_0.1": draw}
    medians = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            medians[k].append(statistics.median(timed(fn) for _ in range(args.steps)))
    ms = {k: round(statistics.median(v), 4) for k, v in medians.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in medians.items()}
    depth = len(models[0.1].blocks)
    print(json.dumps(dict(step="step", box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), batch=args.batch,
                          precision=args.precision, rows=[g.shape[0] * ((g.shape[-1] // 16) ** 2 + 1) for g in groups], ms=ms,
                          spread_ms=spread, slowdown=round(ms["rate_0.1"] / ms["rate_0"], 4),
                          draw_share=round(ms["draw_0.1"] / ms["rate_0.1"], 5), tables_per_group=2 * (depth - 1),
                          steps=args.steps, warmup=args.warmup, rounds=args.rounds)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ops", "step"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=197)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--precision", default="bf16x3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_drop_path.py needs a HIP device: nothing is measured without one")
    if args.rounds is None:
        args.rounds = 7 if args.what == "ops" else 3
    (ops if args.what == "ops" else step)(args)


if __name__ == "__main__":
    main()
