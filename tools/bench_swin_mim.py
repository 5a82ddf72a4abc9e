"""Time the Swin SimMIM loss operator and a whole pre-training step on the HIP path.

  loss   ocm_op_mim_l1_loss (reconstruction, loss, loss gradient in the decoder GEMM's row layout) plus the d_loss multiply of
         the backward, against the composed chain model.MIM._forward runs today on the same rows: ocm_op_pixel_shuffle,
         ocm_op_nearest_upsample, the elementwise torch ops of the masked L1, their autograd backward and
         ocm_op_pixel_shuffle_backward. Both sides start from the GEMM's output `lin` and end at the loss and d loss / d lin.
         Shape 1: Swin at 192^2, s = 32, p = 4, c = 3, B = 128. Shape 2: ViT's 384^2, s = p = 8, c = 3, B = 16.
         The bytes the fused operator must move (lin and x read, rec and dlin written, the mask) over its time is its achieved
         bandwidth; the multiply adds a read and a write of dlin.
  step   one SwinForMaskedImageModeling training step (Swin-T, 192^2, window 6, the 768 -> 3072 decoder): forward, backward,
         optimizer.AdamW, per phase.
The two sides of a comparison are timed in alternation, after a warm-up of every shape.

  python tools/bench_swin_mim.py [--precision bf16x3] [--reps 20] [--step-batch 32]
"""
import argparse
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_ocm_wmsegmentation_amd  # noqa: E402,F401
from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402
from vit_ocm_wmsegmentation_amd import model as M  # noqa: E402
from vit_ocm_wmsegmentation_amd import optimizer as OPT  # noqa: E402
from vit_ocm_wmsegmentation_amd import swin as SW  # noqa: E402
from vit_ocm_wmsegmentation_amd.engine import _p, _stream, _ws  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


class _Shuffle(torch.autograd.Function):
    """ocm_op_pixel_shuffle with its backward, as _PixelShuffleHead runs them behind the GEMM."""

    @staticmethod
    def forward(ctx, lin, B, hp, s):
        ctx.geo = (lin.shape[0], s, hp)
        return M._pixel_shuffle(lin, B, hp, hp, s)

    @staticmethod
    def backward(ctx, g):
        rows, s, hp = ctx.geo
        return M._pixel_shuffle_backward(g, rows, s, hp, hp), None, None, None


def loss_case(lib, dev, B, S, s, p, c, reps):
    hp = S // s
    lin = torch.randn(B * hp * hp, c * s * s, device=dev)
    x = torch.rand(B, c, S, S, device=dev) * 0.3
    mask = torch.rand(B, S // p, S // p, device=dev) < 0.6
    m8 = mask.to(torch.uint8).contiguous()
    dloss = torch.ones((), device=dev)
    nbytes = lib.ocm_mim_l1_loss_workspace_bytes(B, hp, hp, c, s)
    ws = _ws(nbytes, dev)
    rec, dlin, loss = torch.empty_like(x), torch.empty_like(lin), torch.empty((), device=dev)

    def fused():
        _lib.check(lib.ocm_op_mim_l1_loss(_p(lin), _p(x), _p(m8), B, hp, hp, c, s, p, _p(rec), _p(dlin), _p(loss), _p(ws), nbytes,
                                          _stream()))
        return dlin * dloss

    lin_g = lin.clone().requires_grad_(True)

    def composed():  # MIM._forward's chain behind the GEMM, and its backward down to d lin
        lin_g.grad = None
        r = _Shuffle.apply(lin_g, B, hp, s)
        m32 = mask.to(torch.float32).contiguous()
        pm = torch.empty((B, S, S), dtype=torch.float32, device=dev)
        _lib.check(lib.ocm_op_nearest_upsample(_p(m32), _p(pm), B, S // p, S // p, p, _stream()))
        pm = pm.unsqueeze(1)
        err = (x - r).abs() * pm
        ls = err.sum() / (pm.sum() + 1e-5) / c
        ls.backward()
        return ls, lin_g.grad

    for _ in range(3):
        d1 = fused()
        l2, d2 = composed()
    torch.cuda.synchronize()
    same = dict(loss_abs_diff=abs(float(loss) - float(l2.detach())), dlin_max_abs_diff=float((d1 - d2).abs().max()),
                dlin_scale=float(d1.abs().max()))
    tf, tc = [], []
    for _ in range(reps):
        tf.append(_timed(fused)[0])
        tc.append(_timed(composed)[0])
    tf, tc = sorted(tf), sorted(tc)
    mf, mc = tf[len(tf) // 2], tc[len(tc) // 2]
    moved = 4 * (lin.numel() * 2 + x.numel() * 2) + m8.numel() + 2 * 4 * lin.numel()  # the operator, then the multiply
    return dict(B=B, S=S, s=s, p=p, c=c, fused_ms=round(mf, 4), composed_ms=round(mc, 4), speedup=round(mc / mf, 2),
                fused_min_ms=round(tf[0], 4), fused_max_ms=round(tf[-1], 4), composed_min_ms=round(tc[0], 4),
                fused_gbytes_per_s=round(moved / (mf * 1e-3) / 1e9, 1), **same)


def step_case(dev, precision, B, reps):
    cfg = SW.SwinConfig(image_size=192, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=6,
                        encoder_stride=32, drop_path_rate=0.1)
    torch.manual_seed(0)
    m = SW.SwinForMaskedImageModeling(cfg).to(dev).set_precision(precision).train().requires_grad_(True)
    opt = OPT.AdamW(m.parameters(), lr=1e-4, weight_decay=0.05)
    x = torch.rand(B, 3, 192, 192, device=dev) * 0.3
    mask = torch.rand(B, 48 * 48, device=dev) < 0.6

    def step():
        opt.zero_grad(set_to_none=True)
        tf, out = _timed(lambda: m(pixel_values=x, bool_masked_pos=mask))
        tb, _ = _timed(lambda: out.loss.backward())
        to, _ = _timed(opt.step)
        return tf, tb, to

    for _ in range(2):
        step()
    rows = sorted((sum(t), t) for t in (step() for _ in range(reps)))
    tot, (tf, tb, to) = rows[len(rows) // 2]
    return dict(model="swin_tiny_patch4_window6_192", batch=B, precision=precision, fwd_ms=round(tf, 2), bwd_ms=round(tb, 2),
                opt_ms=round(to, 2), step_ms=round(tot, 2), images_per_s=round(B / (tot * 1e-3), 1),
                kept_mib_per_image=round(m.__dict__["_train_kept_bytes"] / B / 2 ** 20, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16x3", choices=sorted(_lib.PRECISIONS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-batch", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_swin_mim needs a HIP device")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = dict(box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), reps=args.reps,
               loss_swin_192=loss_case(lib, dev, 128, 192, 32, 4, 3, args.reps),
               loss_vit_384=loss_case(lib, dev, 16, 384, 8, 8, 3, args.reps),
               step=step_case(dev, args.precision, args.step_batch, max(3, args.reps // 4)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
