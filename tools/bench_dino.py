"""Time one DINO training step of ViT-S/16 on the HIP path, split by phase, beside a torch twin of head + loss + EMA.

The step: 2 x 224^2 + 8 x 96^2 crops of `--batch` images (random tiles), student and teacher MultiCropWrapper(vit_small(16),
DINOHead at its defaults: 384 -> 2048 -> 2048 -> 256 -> 65536), DINOLoss, ema_update. The autograd graph is cut between the
backbone, the head and the loss (detach + requires_grad_) so that each phase's forward and backward are timed on their own with
device events: teacher forward, backbone forward / backward, head forward / backward, loss forward / backward (the centre update
is part of the loss forward), optimizer.AdamW's step (reported, not part of the split), EMA. The twin runs the same head, loss and EMA through ATen / rocBLAS in fp32 on the same rows:
nn.Linear / nn.GELU / F.normalize / nn.utils.weight_norm, log_softmax / softmax, and p.mul_(m).add_((1 - m) * q) per parameter.
Candidates alternate within a round; per phase the median of `--steps` timings after `--warmup` steps and the spread of the
medians over `--rounds`.

  python tools/bench_dino.py [--batch 64] [--steps 10] [--warmup 3] [--rounds 3] [--precision bf16x3]
"""
import argparse
import json
import os
import socket
import statistics
import sys
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_ocm_wmsegmentation_amd  # noqa: E402,F401
from vit_ocm_wmsegmentation_amd import optimizer as OPT  # noqa: E402
from vit_ocm_wmsegmentation_amd.dino import utils as DU  # noqa: E402
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as VT  # noqa: E402

OUT_DIM, NCROPS, STUDENT_TEMP, TEACHER_TEMP, MOMENTUM = 65536, 10, 0.1, 0.04, 0.996


class Phases:
    """Device-event brackets: with phases("name"): ... ; ms() after a synchronise."""

    def __init__(self):
        self.events = []

    def __call__(self, name):
        self.name = name
        return self

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        self.events.append((self.name, self.a, b))

    def ms(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.events:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        self.events = []
        return out


def _cut(t):
    return t.detach().requires_grad_(True)


def hip_step(student, teacher, criterion, opt, crops, ph):
    with ph("teacher_forward"), torch.no_grad():
        tout = teacher(crops[:2])
    with ph("backbone_forward"):
        feats = torch.cat([student.backbone(torch.cat(crops[:2])), student.backbone(torch.cat(crops[2:]))])
    f2 = _cut(feats)
    with ph("head_forward"):
        out = student.head(f2)
    o2 = _cut(out)
    with ph("loss_forward"):
        loss = criterion(o2, tout, 0)
    with ph("loss_backward"):
        loss.backward()
    with ph("head_backward"):
        out.backward(o2.grad)
    with ph("backbone_backward"):
        feats.backward(f2.grad)
    with ph("optimizer"):  # (moves the student, so the next step rebuilds the head's weight-normed last layer as training does)
        opt.step()
    with ph("ema"):
        DU.ema_update(list(teacher.parameters()), list(student.parameters()), MOMENTUM)
    student.zero_grad(set_to_none=True)


class TorchHead(nn.Module):
    def __init__(self, in_dim, out_dim, hidden_dim=2048, bottleneck_dim=256):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, hidden_dim), nn.GELU(),
                                 nn.Linear(hidden_dim, bottleneck_dim))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.last_layer = nn.utils.weight_norm(nn.Linear(bottleneck_dim, out_dim, bias=False))
        self.last_layer.weight_g.data.fill_(1)
        self.last_layer.weight_g.requires_grad = False

    def forward(self, x):
        return self.last_layer(F.normalize(self.mlp(x), dim=-1, p=2))


def torch_loss(student_out, teacher_out, center, batch):
    logp = F.log_softmax(student_out / STUDENT_TEMP, dim=-1).chunk(NCROPS)
    q = F.softmax((teacher_out - center) / TEACHER_TEMP, dim=-1).detach().chunk(2)
    total, terms = 0, 0
    for i in range(2):
        for v in range(NCROPS):
            if v != i:
                total = total + torch.sum(-q[i] * logp[v], dim=-1).mean()
                terms += 1
    with torch.no_grad():
        center.copy_(center * 0.9 + (teacher_out.sum(0, keepdim=True) / len(teacher_out)) * 0.1)
    return total / terms


def torch_step(head, teacher_head, center, feats, tfeats, batch, ema_pairs, ph):
    with ph("teacher_head_forward"), torch.no_grad():
        tout = teacher_head(tfeats)
    f2 = _cut(feats)
    with ph("head_forward"):
        out = head(f2)
    o2 = _cut(out)
    with ph("loss_forward"):
        loss = torch_loss(o2, tout, center, batch)
    with ph("loss_backward"):
        loss.backward()
    with ph("head_backward"):
        out.backward(o2.grad)
    with ph("ema"), torch.no_grad():
        for p, q in ema_pairs:
            p.mul_(MOMENTUM).add_((1 - MOMENTUM) * q.detach())
    head.zero_grad(set_to_none=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="bf16x3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def wrapper(train):
        bb = VT.vit_small(16).set_precision(args.precision)
        head = VT.DINOHead(384, OUT_DIM)
        head.precision = args.precision
        if train:
            bb.enable_training()
        return DU.MultiCropWrapper(bb, head).to(dev).train()

    student, teacher = wrapper(True), wrapper(False)
    teacher.load_state_dict(student.state_dict())
    for p in teacher.parameters():
        p.requires_grad = False
    criterion = DU.DINOLoss(OUT_DIM, NCROPS, TEACHER_TEMP, TEACHER_TEMP, 0, 1).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    crops = [torch.rand(args.batch, 3, s, s, device=dev, generator=gen) * 0.3 for s in (224, 224) + (96,) * (NCROPS - 2)]

    thead, tteacher = TorchHead(384, OUT_DIM).to(dev), TorchHead(384, OUT_DIM).to(dev)
    for p in tteacher.parameters():
        p.requires_grad = False
    center = torch.zeros(1, OUT_DIM, device=dev)
    feats = torch.randn(NCROPS * args.batch, 384, device=dev, generator=gen)
    tfeats = torch.randn(2 * args.batch, 384, device=dev, generator=gen)

    # the twin's EMA moves tensors of the whole model's shapes, as ema_update does: the head's own and copies of the backbone's
    ema_pairs = list(zip(tteacher.parameters(), thead.parameters()))
    ema_pairs += [(torch.randn_like(p), p.detach().clone()) for p in student.backbone.parameters()]
    opt = OPT.AdamW(DU.get_params_groups(student), lr=1e-5)
    cands = {"hip": lambda ph: hip_step(student, teacher, criterion, opt, crops, ph),
             "torch_twin": lambda ph: torch_step(thead, tteacher, center, feats, tfeats, args.batch, ema_pairs, ph)}
    medians = {k: {} for k in cands}
    for _ in range(args.rounds):  # candidates alternate within a round
        for key, fn in cands.items():
            ph = Phases()
            for _ in range(args.warmup):
                fn(ph)
            ph.ms()
            per_step = []
            for _ in range(args.steps):
                fn(ph)
                per_step.append(ph.ms())
            for name in per_step[0]:
                medians[key].setdefault(name, []).append(statistics.median(s[name] for s in per_step))
    rows = {}
    for key, phases in medians.items():
        rows[key] = {name: dict(ms=round(statistics.median(v), 4), spread_ms=round(max(v) - min(v), 4)) for name, v in phases.items()}

    def total(key, names):
        return round(sum(rows[key][n]["ms"] for n in names), 4)

    hip = rows["hip"]
    split = dict(backbone=total("hip", ["teacher_forward", "backbone_forward", "backbone_backward"]),
                 head=total("hip", ["head_forward", "head_backward"]), loss=total("hip", ["loss_forward", "loss_backward"]),
                 ema=hip["ema"]["ms"], optimizer_not_in_split=hip["optimizer"]["ms"])
    twin = dict(head=total("torch_twin", ["head_forward", "head_backward"]), loss=total("torch_twin", ["loss_forward", "loss_backward"]),
                ema=rows["torch_twin"]["ema"]["ms"])
    note = "teacher_forward holds the teacher's backbone AND head and is counted under backbone"
    print(json.dumps(dict(box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), batch=args.batch, precision=args.precision,
                          rows_student=NCROPS * args.batch, out_dim=OUT_DIM, split_ms=split, torch_twin_ms=twin, phases=rows,
                          note=note, steps=args.steps, warmup=args.warmup, rounds=args.rounds)), flush=True)


if __name__ == "__main__":
    main()
