"""Time one training step of build_unet on the HIP path (PGT.py's step: sigmoid Dice loss, backward, Adam) at 384^2, batch 8, in
the three precisions, next to a plain-PyTorch fp32 eager twin of the same network on the same GPU, timed in alternation. Per
precision: the forward, the backward and its split (data gradients = the 3x3 convolutions with the flipped kernel and the
up-convolutions' GEMM; weight gradients = im2col + ocm_op_weight_grad; the rest = BatchNorm + ReLU, pool, gather and classifier
backwards), the optimizer step, and torch.cuda.max_memory_allocated of a step. The split comes from device events around the
parts of _UNetTrain.backward (model._phase); the saved-activation footprint is the allocator's growth over a forward.

  python tools/bench_unet_train.py [--batch 8] [--img 384] [--reps 3] [--precisions fp32,bf16x3,bf16]
"""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.unet_twin import UNetTwin  # noqa: E402  (the eager twin: F.conv2d, F.batch_norm, F.max_pool2d, F.conv_transpose2d)
from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402
from vit_ocm_wmsegmentation_amd import model as M  # noqa: E402
from vit_ocm_wmsegmentation_amd import optimizer as OPT  # noqa: E402


def dice_loss(pred, target, smooth=1.0):
    p, t = torch.sigmoid(pred).reshape(-1), target.reshape(-1)
    return 1 - (2.0 * (p * t).sum() + smooth) / (p.sum() + t.sum() + smooth)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def _step(net, opt, x, y, log=None):
    opt.zero_grad(set_to_none=True)
    tf, loss = _timed(lambda: dice_loss(net(x), y))
    if log is not None:
        log.clear()
    tb, _ = _timed(loss.backward)
    to, _ = _timed(opt.step)
    parts = {"data": 0.0, "weight": 0.0}
    for name, a, b in log or ():
        parts[name] += a.elapsed_time(b)
    return {"fwd": tf, "bwd": tb, "bwd_data": parts["data"], "bwd_weight": parts["weight"],
            "bwd_rest": tb - parts["data"] - parts["weight"], "opt": to, "step": tf + tb + to}


def _median(rows):
    return {k: round(sorted(r[k] for r in rows)[len(rows) // 2], 3) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img", type=int, default=384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--precisions", default="fp32,bf16x3,bf16")
    ap.add_argument("--optimizer", default="torch", choices=["torch", "hip"],
                    help="the HIP step's optimizer: torch.optim (default) or optimizer.py's multi-tensor kernels")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.rand(args.batch, 3, args.img, args.img, device=dev)
    y = (x[:, :1] > 0.5).float()
    twin = UNetTwin().to(dev).train()
    opt_t = torch.optim.Adam(twin.parameters(), lr=1e-4)
    res = dict(box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), batch=args.batch, img=args.img, reps=args.reps)
    for precision in args.precisions.split(","):
        net = M.build_unet().to(dev).train().enable_training()
        net.precision = precision
        opt = (OPT.Adam if args.optimizer == "hip" else torch.optim.Adam)(net.parameters(), lr=1e-4)
        log = net.__dict__["_phase_log"] = []
        for _ in range(2):  # warm-up: operand copies, LDS opt-in, allocator
            _step(net, opt, x, y, log)
            _step(twin, opt_t, x, y)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        out = net(x)
        torch.cuda.synchronize()
        saved = torch.cuda.memory_allocated() - base  # what the graph keeps alive (and the logits)
        del out
        torch.cuda.reset_peak_memory_stats()
        hip, eager = [], []
        for _ in range(args.reps):
            hip.append(_step(net, opt, x, y, log))
            eager.append(_step(twin, opt_t, x, y))
        peak = torch.cuda.max_memory_allocated()
        h, e = _median(hip), _median(eager)
        res[precision] = dict(ms=h, eager_ms={k: e[k] for k in ("fwd", "bwd", "opt", "step")},
                              speedup_vs_eager=round(e["step"] / h["step"], 2), saved_gb=round(saved / 1e9, 2),
                              max_memory_allocated_gb=round(peak / 1e9, 2))
        del net, opt, log
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
