#!/usr/bin/env python3
"""One linear-probing training step at finetune.py's shape (--finetune False): a frozen ViT-S/8 encoder (12 blocks,
img_size [384]) at 384 x 384, LinearProbing(layer_num=2), sigmoid Dice loss, Adam on the decoder. Batch 1 (the reference's
default) and batch 8. Events around each phase: encoder forward, decoder forward (+ loss), decoder backward, Adam.
FLOP / byte counts from the shapes. Then the conv1 weight-gradient kernel alone against the forward conv1 ocm_op_linear of
the same FLOP count, with its share of the MFMA peak of the precision. Prints one JSON line per batch and one for the
kernel comparison."""
import argparse
import json
import os
import sys
from functools import partial

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vit_ocm_wmsegmentation_amd import _lib, model as M, synth  # noqa: E402
from vit_ocm_wmsegmentation_amd.engine import _p, _stream, to_operand  # noqa: E402

# dense MFMA peaks (MI355X spec): bf16 2.5 PF; split-bf16 runs three bf16 products per useful one; fp32 157.3 TF
PEAK = {"bf16": 2.5e15, "bf16x3": 2.5e15 / 3, "fp32": 157.3e12}


def build(precision, dev, depth):
    enc = M.VisionTransformerForFinetune(patch_size=8, embed_dim=384, depth=depth, num_heads=6, mlp_ratio=4,
                                         img_size=[384], qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                                         interpolate_encoding=True)
    enc.load_state_dict(synth.synth_state_dict(384, depth, 8, seed=5, img_size=224), strict=True)
    for p in enc.parameters():
        p.requires_grad_(False)
    enc = enc.to(dev).set_precision(precision)
    lp = M.LinearProbing(enc, 8, layer_num=2).to(dev).train()
    return lp


def dice_loss(pred, target, smooth=1.0):
    p = torch.sigmoid(pred).reshape(-1)
    t = target.reshape(-1)
    return 1 - (2.0 * (p * t).sum() + smooth) / (p.sum() + t.sum() + smooth)


def step_phases(lp, opt, x, y):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    ev[0].record()
    with torch.no_grad():
        tokens = lp.encoder._encode(x, tokens=True)
    ev[1].record()
    opt.zero_grad(set_to_none=True)
    loss = dice_loss(M._train_forward(lp, tokens), y)
    ev[2].record()
    loss.backward()
    ev[3].record()
    opt.step()
    ev[4].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]


def time_call(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default=_lib.DEFAULT_PRECISION, choices=sorted(_lib.PRECISIONS))
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=12)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lp = build(args.precision, dev, args.depth)
    opt = torch.optim.Adam(lp.two_layer_decoder.parameters(), lr=1e-3)
    D, s, mid, oc = 384, 8, 256, 64
    for B in (int(b) for b in args.batches.split(",")):
        x = synth.synth_tiles(B, 384, seed=1).to(dev)
        y = (torch.nn.functional.avg_pool2d(x[:, :1], 8) > 0.15).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
        for _ in range(args.warmup):
            step_phases(lp, opt, x, y)
        runs = [step_phases(lp, opt, x, y) for _ in range(args.steps)]
        med = [sorted(r[i] for r in runs)[len(runs) // 2] for i in range(4)]
        Mr, T = B * 48 * 48, 48 * 48 + 1
        fwd = 2 * Mr * (mid * 9 * D + oc * 9 * mid)
        bwd = 2 * Mr * (oc * 9 * mid + mid * 9 * oc + mid * 9 * D)
        enc = B * args.depth * (2 * T * (3 * D * D + D * D + 8 * D * D) + 4 * T * T * D)
        # HBM bytes of the decoder step, fp32 activations: im2col rows a1 / a2 written and read (forward in the operand
        # type, backward in fp32 again), y1 / dz / dy1, the weight-gradient slabs
        esz = {"bf16": 2, "bf16x3": 4, "fp32": 4}[args.precision]
        dec_bytes = Mr * (9 * D * (esz * 2 + 8) + 9 * mid * (esz * 2 + 8) + mid * 4 * 6 + 9 * oc * esz * 2)
        print(json.dumps({"bench": "linear_probing_step", "precision": args.precision, "batch": B, "depth": args.depth,
                          "ms": {"encoder_fwd": med[0], "decoder_fwd": med[1], "decoder_bwd": med[2], "adam": med[3]},
                          "decoder_over_encoder": (med[1] + med[2]) / med[0],
                          "gflop": {"encoder_fwd": enc / 1e9, "decoder_fwd": fwd / 1e9, "decoder_bwd": bwd / 1e9},
                          "decoder_gbytes": dec_bytes / 1e9,
                          "decoder_tflops": (fwd + bwd) / ((med[1] + med[2]) * 1e-3) / 1e12}), flush=True)
    # conv1 weight gradient vs the same-FLOP forward conv1 GEMM, at batch 8
    lib, prec = _lib.load(), _lib.PRECISIONS[args.precision]
    Mr, N, K = 8 * 48 * 48, mid, 9 * D
    g = torch.Generator().manual_seed(0)
    dy = torch.randn(Mr, N, generator=g).to(dev)
    a = torch.randn(Mr, K, generator=g).to(dev)
    dw, db = torch.empty(N, K, device=dev), torch.empty(N, device=dev)
    nb = lib.ocm_weight_grad_workspace_bytes(Mr, N, K)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    t_wg = time_call(lambda: lib.ocm_op_weight_grad(prec, _p(dy), _p(a), _p(dw), _p(db), Mr, N, K, _p(ws), nb, _stream()), 20)
    a_op, w_op = to_operand(a, prec), to_operand(torch.randn(N, K, generator=g).to(dev), prec)
    bias, out = torch.zeros(N, device=dev), torch.empty(Mr, N, device=dev)
    t_fw = time_call(lambda: lib.ocm_op_linear(prec, _p(a_op), _p(w_op), _p(bias), None, _p(out), Mr, N, K,
                                               _lib.OCM_EPI_BIAS_F32, _stream()), 20)
    flop = 2.0 * Mr * N * K
    print(json.dumps({"bench": "conv1_weight_grad", "precision": args.precision, "M": Mr, "N": N, "K": K,
                      "weight_grad_ms": t_wg, "forward_linear_ms": t_fw, "ratio": t_wg / t_fw,
                      "weight_grad_peak_share": flop / (t_wg * 1e-3) / PEAK[args.precision],
                      "forward_peak_share": flop / (t_fw * 1e-3) / PEAK[args.precision]}), flush=True)


if __name__ == "__main__":
    main()
