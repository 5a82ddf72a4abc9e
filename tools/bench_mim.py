"""Time one mim.py training step on the HIP path: B = 16 images of 384^2, build_model()'s encoder (depth 4, 3 heads of 128,
patch 8), MIM's 1x1-conv decoder, AdamW. Reports per phase (the weight re-pack that every forward after optimizer.step() runs,
training forward, backward, optimizer step; `step` is their sum), the decoder's forward + backward alone, the attention-backward
kernels alone at (B 16, H 3, N 2305, hd 128) with their FLOP rate next to the forward attention kernel at the same shape, and, as
a yardstick, a plain-PyTorch fp32 eager twin of the same step on the same GPU. The two are timed in alternation. The backward's
split by kernel class comes from a kernel trace of this tool (rocprofv3 --kernel-trace --stats).

  python tools/bench_mim.py [--batch 16] [--img 384] [--depth 4] [--precision bf16x3] [--reps 5]
"""
import argparse
import json
import math
import os
import socket
import sys
import time
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_ocm_wmsegmentation_amd  # noqa: E402,F401
from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402
from vit_ocm_wmsegmentation_amd import model as M  # noqa: E402
from vit_ocm_wmsegmentation_amd import optimizer as OPT  # noqa: E402


class EagerTwin(nn.Module):
    """SimMIM (model.py:10-83) in plain torch fp32: patch conv, mask blend, cls + interpolated pos, pre-norm blocks, final norm,
    1x1 conv + pixel shuffle, masked L1 loss."""

    def __init__(self, D, depth, heads, p, img):
        super().__init__()
        self.p, self.h, self.img = p, heads, img
        self.proj = nn.Conv2d(3, D, p, p)
        self.cls = nn.Parameter(torch.randn(1, 1, D) * .02)
        self.pos = nn.Parameter(torch.randn(1, (224 // p) ** 2 + 1, D) * .02)
        self.mask_token = nn.Parameter(torch.randn(1, 1, D) * .02)
        self.blocks = nn.ModuleList([nn.ModuleDict(dict(n1=nn.LayerNorm(D, eps=1e-6), qkv=nn.Linear(D, 3 * D),
                                                        proj=nn.Linear(D, D), n2=nn.LayerNorm(D, eps=1e-6),
                                                        fc1=nn.Linear(D, 4 * D), fc2=nn.Linear(4 * D, D)))
                                     for _ in range(depth)])
        self.norm = nn.LayerNorm(D, eps=1e-6)
        self.dec = nn.Conv2d(D, p * p * 3, 1)

    def forward(self, x, mask):
        t = self.proj(x).flatten(2).transpose(1, 2)
        B, L, D = t.shape
        w = mask.flatten(1).unsqueeze(-1).float()
        t = t * (1 - w) + self.mask_token.expand(B, L, -1) * w
        t = torch.cat((self.cls.expand(B, -1, -1), t), 1)
        n0 = self.pos.shape[1] - 1
        side, s = int(math.sqrt(n0)), self.img // self.p + 0.1
        g = F.interpolate(self.pos[:, 1:].reshape(1, side, side, D).permute(0, 3, 1, 2),
                          scale_factor=(s / math.sqrt(n0), s / math.sqrt(n0)), mode="bicubic")
        t = t + torch.cat((self.pos[:, :1], g.permute(0, 2, 3, 1).reshape(1, -1, D)), 1)
        H = self.h
        for b in self.blocks:
            q, k, v = b["qkv"](b["n1"](t)).reshape(B, L + 1, 3, H, D // H).permute(2, 0, 3, 1, 4)
            a = ((q @ k.transpose(-2, -1)) * (D // H) ** -0.5).softmax(-1)
            t = t + b["proj"]((a @ v).transpose(1, 2).reshape(B, L + 1, D))
            t = t + b["fc2"](F.gelu(b["fc1"](b["n2"](t))))
        z = self.norm(t)[:, 1:].transpose(1, 2).reshape(B, D, int(L ** .5), int(L ** .5))
        rec = F.pixel_shuffle(self.dec(z), self.p)
        m = mask.repeat_interleave(self.p, 1).repeat_interleave(self.p, 2).unsqueeze(1).float()
        return (F.l1_loss(x, rec, reduction="none") * m).sum() / (m.sum() + 1e-5) / 3


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--img", type=int, default=384)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--precision", default="bf16x3", choices=sorted(_lib.PRECISIONS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--optimizer", default="torch", choices=["torch", "hip"],
                    help="the HIP step's optimizer: torch.optim (default) or optimizer.py's multi-tensor kernels")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S, p, D, H = args.batch, args.img, 8, 384, 3
    torch.manual_seed(0)
    enc = M.VisionTransformerForSimMIM(patch_size=p, embed_dim=D, depth=args.depth, num_heads=H, mlp_ratio=4, img_size=[S],
                                       qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)
    mim = M.MIM(enc, p).to(dev).train()
    enc.set_precision(args.precision)
    opt = (OPT.AdamW if args.optimizer == "hip" else torch.optim.AdamW)(mim.parameters(), lr=1e-4, weight_decay=0.05)
    twin = EagerTwin(D, args.depth, H, p, S).to(dev).train()
    opt_t = torch.optim.AdamW(twin.parameters(), lr=1e-4, weight_decay=0.05)
    x = torch.rand(B, 3, S, S, device=dev) * 0.3
    mask = (torch.rand(B, S // p, S // p, device=dev) < 0.6).long()

    def hip_step():
        opt.zero_grad(set_to_none=True)
        # the engine re-packs its weight copies on their new (data_ptr, _version) inside the forward; timed on its own here
        tr, _ = _timed(lambda: enc._engine(dev))
        tf, (loss, _, _) = _timed(lambda: mim(x, mask))
        tb, _ = _timed(lambda: loss.backward())
        to, _ = _timed(opt.step)
        return tr, tf, tb, to

    def twin_step():
        opt_t.zero_grad(set_to_none=True)
        t0 = time.perf_counter()
        twin(x, mask).backward()
        opt_t.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # the attention-backward kernels alone at the step's shape
    N = (S // p) ** 2 + 1
    lib = _lib.load()
    qkv = torch.randn(3, B, H, N, D // H, device=dev)
    do, lse, delta = torch.randn(B * N, D, device=dev), torch.randn(B * H, N, device=dev) + 10, torch.randn(B * H, N, device=dev)
    dqkv = torch.empty(B * N, 3 * D, device=dev)

    prec = _lib.PRECISIONS[args.precision]
    adt = {0: torch.bfloat16, 1: torch.float32, 2: torch.int32}[prec]
    npad = lib.ocm_n_pad_prec(prec, N)
    qo = torch.zeros((B * H, npad, D // H), dtype=adt, device=dev)
    ko, vto = torch.zeros_like(qo), torch.zeros((B * H, D // H, npad), dtype=adt, device=dev)
    ctxo, lseo = torch.empty((B * N, D), dtype=adt, device=dev), torch.empty((B * H, N), device=dev)

    def attn_fwd():  # the forward attention kernel (context + lse2) of the step's precision at the same shape
        _lib.check(lib.ocm_op_attention_hd(prec, qo.data_ptr(), ko.data_ptr(), vto.data_ptr(), ctxo.data_ptr(), lseo.data_ptr(),
                                           B, N, H, D // H, (D // H) ** -0.5, None))

    tokens = torch.randn(B, N, D, device=dev, requires_grad=True)
    conv = mim.decoder[0]
    dmeta = M._head_meta(mim)

    def decoder():  # MIM's decoder alone: forward + backward into its weight, its bias and the tokens (the CLS row gets zeros)
        M._PixelShuffleHead.apply(dmeta, tokens[:, 1:].contiguous(), conv.weight, conv.bias).sum().backward()

    def attn_bwd():
        _lib.check(lib.ocm_op_attention_backward(qkv.data_ptr(), lse.data_ptr(), do.data_ptr(), delta.data_ptr(),
                                                 dqkv.data_ptr(), B, N, H, D // H, (D // H) ** -0.5, None))

    for _ in range(2):  # warm-up: packing, LDS opt-in, allocator
        hip_step()
        twin_step()
        attn_bwd()
        attn_fwd()
        decoder()
    torch.cuda.synchronize()
    rows = {k: [] for k in ("repack", "fwd", "bwd", "opt", "step", "twin", "attn_bwd", "attn_fwd", "decoder")}
    for _ in range(args.reps):
        tr, tf, tb, to = hip_step()
        rows["repack"].append(tr)
        rows["fwd"].append(tf)
        rows["bwd"].append(tb)
        rows["opt"].append(to)
        rows["step"].append(tr + tf + tb + to)
        rows["twin"].append(twin_step())
        rows["attn_bwd"].append(_timed(attn_bwd)[0])
        rows["attn_fwd"].append(_timed(attn_fwd)[0])
        rows["decoder"].append(_timed(decoder)[0])
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    flops = 14 * B * H * N * N * (D // H)  # dK/dV kernel: S, dP, dV, dK; dQ kernel: S, dP, dQ (2 N^2 hd each)
    res = dict(box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), batch=B, img=S, depth=args.depth,
               precision=args.precision, ms={k: round(v, 3) for k, v in med.items()},
               attn_bwd_tflops=round(flops / (med["attn_bwd"] * 1e-3) / 1e12, 1),
               attn_bwd_over_fwd=round(med["attn_bwd"] / med["attn_fwd"], 2),
               speedup_vs_eager=round(med["twin"] / med["step"], 2), reps=args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
