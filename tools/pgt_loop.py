#!/usr/bin/env python3
"""A run shaped like PGT.py's train / evaluate loop on the HIP path: a ViT-S/8 encoder (synthetic weights) segments synthetic
tiles with eval.segment_images(encoder, x, method="ours"); its masks / 255 are the pseudo ground truth, under no_grad. build_unet
(enable_training) then trains on them: model.train(), DiceLoss(net(x), y).backward(), Adam; then model.eval() under no_grad, as
PGT.py's evaluate does. Prints the loss per step and exits non-zero unless it falls."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits  # noqa: E402
from vit_ocm_wmsegmentation_amd import model as M, synth  # noqa: E402
from vit_ocm_wmsegmentation_amd.eval import segment_images  # noqa: E402
from vit_ocm_wmsegmentation_amd.utils import DiceLoss  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--precision", default="bf16x3")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    encoder = vits.vit_small(patch_size=8, num_classes=0)
    encoder.load_state_dict(synth.synth_arch_state_dict("vit_small", 8, seed=0, variant="sharp", img_size=224), strict=True)
    encoder = encoder.eval().to(dev)
    torch.manual_seed(0)
    net = M.build_unet().to(dev).enable_training()
    net.precision = args.precision
    optimizer = torch.optim.Adam(net.parameters(), lr=args.lr)
    dice_loss = DiceLoss()  # utils.py:410-424 on the HIP path
    train_set = []
    for i in range(4):
        x = synth.synth_tiles(args.batch, args.size, seed=100 + i).to(dev)
        with torch.no_grad():
            masks, _ = segment_images(encoder, x, method="ours")  # (B, S, S) uint8 in {0, 255}
            y = (masks.float() / 255).unsqueeze(1)
        train_set.append((x, y))
    print(f"pseudo ground truth: {sum(float(y.mean()) for _, y in train_set) / len(train_set):.3f} of the pixels are foreground")
    losses = []
    for step in range(args.steps):
        net.train()
        x, y = train_set[step % len(train_set)]
        optimizer.zero_grad()
        loss = dice_loss(net(x), y)
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        print(f"step {step:3d}  train loss {losses[-1]:.4f}", flush=True)
    net.eval()
    with torch.no_grad():
        ev = [dice_loss(net(x), y).item() for x, y in train_set]
    print(f"eval loss {sum(ev) / len(ev):.4f} (first train loss {losses[0]:.4f}, last {losses[-1]:.4f})")
    first, last = sum(losses[:4]) / 4, sum(losses[-4:]) / 4
    if not last < first:
        print(f"loss did not fall: {first:.4f} -> {last:.4f}")
        sys.exit(1)
    print(f"loss fell: {first:.4f} -> {last:.4f} (mean of the first / last four steps)")


if __name__ == "__main__":
    main()
