"""Time dropout on the ViT training path (kernels_dropout.hip) on one MI355X. Two steps, each run under its own time limit:

  timeout -k 10 300 python tools/bench_dropout.py ops  [--batch 64] [--tokens 197] [--dim 384] [--hidden 1536] [--iters 40] [--rounds 7]
  timeout -k 10 400 python tools/bench_dropout.py step [--batch 64] [--steps 6] [--warmup 2] [--rounds 3] [--precision bf16x3]

ops   every fused operator beside the composition of operators it replaces, at batch x tokens rows (12 608: ViT-S/16, B = 64):
        forward   ocm_op_dropout_layernorm      against ocm_op_dropout -> ocm_op_drop_path_layernorm, rows of `dim`; without a
                                                scale table the composition gives that operator a table of ones
        backward  ocm_op_dropout_backward       against ocm_op_dropout -> ocm_op_drop_path_backward, or -> the cast without a
                                                scale table, rows of `dim`
        gelu      ocm_op_gelu_dropout           against ocm_op_gelu (fp32 out) -> ocm_op_dropout -> the cast, rows of `hidden`
        gelu_bwd  ocm_op_gelu_dropout_backward  against ocm_op_dropout -> ocm_op_gelu_backward, rows of `hidden`
      in the three precisions, and the unfused operators alone (ocm_op_drop_path_layernorm, ocm_op_gelu) to show what the ten
      Philox rounds per four elements cost. Every candidate walks several buffer sets (together larger than the 256 MB
      Infinity Cache) so that rows come from HBM; a timing is `--iters` launches between two device events; candidates alternate
      within a round; the figure is the median over `--rounds` and the spread is max - min of the rounds.
step  the training forward + backward of tools/bench_dino.py's backbone (vit_small(16), enable_training(); 2 x 224^2 + 8 x 96^2
      crops of `--batch` images in two resolution groups) at drop_rate 0 and 0.1 (enable_dropout()) on the same build, the two
      models alternating within a round.

Nothing here is a gate. One JSON line per step."""
import argparse
import ctypes as C
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

PRECS = {"fp32": (_lib.OCM_LN_F32, torch.float32, 4), "bf16": (_lib.OCM_LN_BF16, torch.bfloat16, 2),
         "bf16x3": (_lib.OCM_LN_SPLIT, torch.int32, 4)}
EPS = 1e-6
RATE = 0.1


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
    return {k: dict(us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2)) for k, v in times.items()}


def _sets(bytes_per_set):
    return max(2, -(-512 * 2 ** 20 // bytes_per_set))  # at least twice the Infinity Cache in flight


def ops(args):
    lib, dev = _lib.load(), torch.device("cuda:0")
    B, N, D, Mh = args.batch, args.tokens, args.dim, args.hidden
    rows = B * N
    p = lambda t: t.data_ptr()  # noqa: E731
    th, ik = C.c_uint32(), C.c_float()
    _lib.check(lib.ocm_dropout_threshold(RATE, C.byref(th), C.byref(ik)))
    th, ik = th.value, ik.value
    seeds = torch.randint(0, 2 ** 62, (4,), dtype=torch.int64, device=dev)
    scale = (torch.rand(B, device=dev) < 0.9).float() / 0.9
    ones = torch.ones(B, device=dev)
    gamma, beta = torch.randn(D, device=dev), torch.randn(D, device=dev)
    result = dict(step="ops", box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), rows=rows, dim=D, hidden=Mh,
                  rate=RATE, iters=args.iters, rounds=args.rounds, forward={}, backward={}, gelu={}, gelu_backward={})
    # ---- rows of dim: the two row operators
    S = _sets(rows * D * 4 * 4)
    x = [torch.randn(rows, D, device=dev) + 1.0 for _ in range(S)]
    br = [torch.randn(rows, D, device=dev) for _ in range(S)]
    tmp = [torch.empty(rows, D, device=dev) for _ in range(S)]
    out = [torch.empty(rows, D, device=dev) for _ in range(S)]
    for name, (kind, dtype, width) in PRECS.items():
        pc = _lib.PRECISIONS[name]
        y = [torch.empty(rows, D, dtype=dtype, device=dev) for _ in range(S)]
        cands = {}
        for tag, sc, sc_chain in (("scale", scale, scale), ("noscale", None, ones)):
            def fused(i, sc=sc):
                j = i % S
                _lib.check(lib.ocm_op_dropout_layernorm(p(x[j]), p(br[j]), p(seeds), 1, th, ik, p(sc) if sc is not None else None,
                                                        p(gamma), p(beta), p(out[j]), p(y[j]), kind, B, N, D, EPS, None))

            def chain(i, sc=sc_chain):
                j = i % S
                _lib.check(lib.ocm_op_dropout(p(br[j]), p(seeds), 1, th, ik, p(tmp[j]), rows * D, None))
                _lib.check(lib.ocm_op_drop_path_layernorm(p(x[j]), p(tmp[j]), p(sc), p(gamma), p(beta), p(out[j]), p(y[j]), kind, B,
                                                          N, D, EPS, None))

            cands[f"fused_{tag}"], cands[f"chain_{tag}"] = fused, chain

        def plain(i):  # no dropout at all: what the Philox rounds add to a four-pass row kernel
            j = i % S
            _lib.check(lib.ocm_op_drop_path_layernorm(p(x[j]), p(br[j]), p(scale), p(gamma), p(beta), p(out[j]), p(y[j]), kind, B, N,
                                                      D, EPS, None))

        cands["drop_path_layernorm_alone"] = plain
        result["forward"][name] = _alternate(cands, args.iters, args.rounds)
        result["forward"][name]["fused_bytes"] = rows * D * (3 * 4 + width)
        d_op = y if name != "fp32" else None
        cands = {}
        for tag, sc, sc_chain in (("scale", scale, scale), ("noscale", None, None)):
            def fused(i, sc=sc):
                j = i % S
                _lib.check(lib.ocm_op_dropout_backward(pc, p(x[j]), p(seeds), 1, th, ik, p(sc) if sc is not None else None, p(out[j]),
                                                       p(d_op[j]) if d_op else None, B, N, D, None))

            def chain(i, sc=sc_chain):
                j = i % S
                _lib.check(lib.ocm_op_dropout(p(x[j]), p(seeds), 1, th, ik, p(tmp[j]), rows * D, None))
                if sc is not None:
                    _lib.check(lib.ocm_op_drop_path_backward(pc, p(tmp[j]), p(sc), p(out[j]), p(d_op[j]) if d_op else None, B, N, D,
                                                             None))
                elif d_op:
                    cast = lib.ocm_op_cast_bf16 if name == "bf16" else lib.ocm_op_cast_split
                    _lib.check(cast(p(tmp[j]), p(d_op[j]), rows * D, None))

            cands[f"fused_{tag}"], cands[f"chain_{tag}"] = fused, chain
        result["backward"][name] = _alternate(cands, args.iters, args.rounds)
        result["backward"][name]["fused_bytes"] = rows * D * (2 * 4 + (width if d_op else 0))
        del y, d_op
    del x, br, tmp, out
    # ---- rows of hidden: the GELU pair
    n = rows * Mh
    S = _sets(n * 4 * 3)
    h = [torch.randn(rows, Mh, device=dev) for _ in range(S)]
    g32 = [torch.empty(rows, Mh, device=dev) for _ in range(S)]
    dg = [torch.randn(rows, Mh, device=dev) for _ in range(S)]
    for name, (kind, dtype, width) in PRECS.items():
        pc = _lib.PRECISIONS[name]
        o = [torch.empty(rows, Mh, dtype=dtype, device=dev) for _ in range(S)]

        def fused(i):
            j = i % S
            _lib.check(lib.ocm_op_gelu_dropout(pc, p(h[j]), p(seeds), 2, th, ik, p(o[j]), None, n, None))

        def chain(i):
            j = i % S
            if name == "fp32":
                _lib.check(lib.ocm_op_gelu(pc, p(h[j]), p(o[j]), None, n, None))
                _lib.check(lib.ocm_op_dropout(p(o[j]), p(seeds), 2, th, ik, p(o[j]), n, None))
                return
            _lib.check(lib.ocm_op_gelu(_lib.OCM_PREC_FP32, p(h[j]), p(g32[j]), None, n, None))
            _lib.check(lib.ocm_op_dropout(p(g32[j]), p(seeds), 2, th, ik, p(g32[j]), n, None))
            cast = lib.ocm_op_cast_bf16 if name == "bf16" else lib.ocm_op_cast_split
            _lib.check(cast(p(g32[j]), p(o[j]), n, None))

        def plain(i):
            j = i % S
            _lib.check(lib.ocm_op_gelu(pc, p(h[j]), p(o[j]), None, n, None))

        result["gelu"][name] = _alternate({"fused": fused, "chain": chain, "gelu_alone": plain}, args.iters, args.rounds)
        result["gelu"][name]["fused_bytes"] = n * (4 + width)
        del o

    def fused_b(i):
        j = i % S
        _lib.check(lib.ocm_op_gelu_dropout_backward(p(dg[j]), p(h[j]), p(seeds), 2, th, ik, p(dg[j]), p(g32[j]), n, None))

    def chain_b(i):
        j = i % S
        _lib.check(lib.ocm_op_dropout(p(dg[j]), p(seeds), 2, th, ik, p(dg[j]), n, None))
        _lib.check(lib.ocm_op_gelu_backward(p(dg[j]), p(h[j]), p(dg[j]), p(g32[j]), n, None))

    def plain_b(i):
        j = i % S
        _lib.check(lib.ocm_op_gelu_backward(p(dg[j]), p(h[j]), p(dg[j]), p(g32[j]), n, None))

    result["gelu_backward"] = _alternate({"fused": fused_b, "chain": chain_b, "gelu_backward_alone": plain_b}, args.iters,
                                         args.rounds)
    result["gelu_backward"]["fused_bytes"] = n * 16
    print(json.dumps(result), flush=True)


def step(args):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    groups = [torch.rand(2 * args.batch, 3, 224, 224, device=dev, generator=gen) * 0.3,
              torch.rand(8 * args.batch, 3, 96, 96, device=dev, generator=gen) * 0.3]
    base = VT.vit_small(16)
    models = {}
    for rate in (0.0, RATE):
        bb = VT.vit_small(16, drop_rate=rate).set_precision(args.precision)
        bb.load_state_dict(base.state_dict())
        models[rate] = bb.enable_training().enable_dropout().to(dev).train()

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

    cands = {"rate_0": lambda: run(0.0), f"rate_{RATE}": lambda: run(RATE)}
    medians = {k: [] for k in cands}
    for _ in range(args.rounds):
        for k, fn in cands.items():
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            medians[k].append(statistics.median(timed(fn) for _ in range(args.steps)))
    ms = {k: round(statistics.median(v), 4) for k, v in medians.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in medians.items()}
    print(json.dumps(dict(step="step", box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), batch=args.batch,
                          precision=args.precision, rows=[g.shape[0] * ((g.shape[-1] // 16) ** 2 + 1) for g in groups], ms=ms,
                          spread_ms=spread, slowdown=round(ms[f"rate_{RATE}"] / ms["rate_0"], 4),
                          sites=1 + 3 * len(models[RATE].blocks), steps=args.steps, warmup=args.warmup, rounds=args.rounds)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["ops", "step"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=197)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--hidden", type=int, default=1536)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--precision", default="bf16x3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dropout.py needs a HIP device: nothing is measured without one")
    if args.rounds is None:
        args.rounds = 7 if args.what == "ops" else 3
    (ops if args.what == "ops" else step)(args)


if __name__ == "__main__":
    main()
