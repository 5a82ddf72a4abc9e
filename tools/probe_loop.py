#!/usr/bin/env python3
"""A linear-probing run shaped like finetune.py's train / evaluate loop (--finetune False) on the HIP path: a frozen
ViT-S/8 encoder, LinearProbing(encoder, encoder_stride=8, layer_num=2), model.train(), Adam on a sigmoid Dice loss, then
model.eval() under no_grad. Data are synthetic (synth.py tiles) with a segmentation target the patch features can carry:
patches whose mean intensity is above the median. Prints the loss per step and exits non-zero unless it falls."""
import argparse
import os
import sys
from functools import partial

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vit_ocm_wmsegmentation_amd import model as M, synth  # noqa: E402


def dice_loss(pred, target, smooth=1.0):
    p = torch.sigmoid(pred).reshape(-1)
    t = target.reshape(-1)
    return 1 - (2.0 * (p * t).sum() + smooth) / (p.sum() + t.sum() + smooth)


def batch(n, size, seed, dev):
    x = synth.synth_tiles(n, size, seed=seed)
    means = nn.functional.avg_pool2d(x[:, :1], 8)
    y = (means > means.median()).float().repeat_interleave(8, 2).repeat_interleave(8, 3)
    return x.to(dev), y.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--precision", default="bf16x3")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    enc = M.VisionTransformerForFinetune(patch_size=8, embed_dim=384, depth=args.depth, num_heads=6, mlp_ratio=4,
                                         img_size=[args.size], qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6),
                                         interpolate_encoding=True)
    enc.load_state_dict(synth.synth_state_dict(384, args.depth, 8, seed=3, img_size=224), strict=True)
    for p in enc.parameters():  # linear probing: the encoder is frozen
        p.requires_grad = False
    model = M.LinearProbing(enc.to(dev).set_precision(args.precision), encoder_stride=8, layer_num=2).to(dev)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)  # the frozen encoder's parameters get no gradient
    train_set = [batch(args.batch, args.size, 100 + i, dev) for i in range(4)]
    losses = []
    for step in range(args.steps):
        model.train()
        x, y = train_set[step % len(train_set)]
        optimizer.zero_grad()
        loss = dice_loss(model(x), y)
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        print(f"step {step:3d}  train loss {losses[-1]:.4f}", flush=True)
    model.eval()
    with torch.no_grad():
        ev = [dice_loss(model(x), y).item() for x, y in train_set]
    print(f"eval loss {sum(ev) / len(ev):.4f} (first train loss {losses[0]:.4f}, last {losses[-1]:.4f})")
    first, last = sum(losses[:4]) / 4, sum(losses[-4:]) / 4
    if not last < first:
        print(f"loss did not fall: {first:.4f} -> {last:.4f}")
        sys.exit(1)
    print(f"loss fell: {first:.4f} -> {last:.4f} (mean of the first / last four steps)")


if __name__ == "__main__":
    main()
