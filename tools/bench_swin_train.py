"""Time one train.py fine-tuning step of SwinForImageClassification on the HIP path: Swin-T at 224^2 (or --image-size: 384 is the
project's tile, whose grids 96 / 48 / 24 / 12 are padded to the windows of 7: the tool then turns enable_padded_training on and
prints the padded / real token counts per stage), 5 labels, AdamW (lr 5e-5), drop_path_rate 0.1. Reports per phase (training forward, which repacks the weights an optimizer step changed; backward; AdamW;
`step` is their sum) and, as a yardstick, an fp32 eager twin on the same GPU: the oracle's functions (oracle/swin_oracle.py)
under torch autograd with the same weights, timed in alternation with the HIP step in one process. Also reports the activations
the training forward keeps per image. The split by kernel class comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats). --arch swin_b_w12 times Swin-B / window 12 (embed_dim 128, depths 2/2/18/2, heads 4/8/16/32:
the window12-384 checkpoints' geometry, --image-size 384 tiles every stage without padding) with enable_wide_window_training on;
--embed-dim / --depths / --num-heads / --window-size override single fields of either architecture.

  python tools/bench_swin_train.py [--batch 8] [--precision bf16] [--reps 5] [--optimizer hip] [--image-size 384] [--no-twin]
                                   [--arch swin_b_w12] [--embed-dim 128] [--depths 2,2,18,2] [--num-heads 4,8,16,32]
                                   [--window-size 12]
"""
import argparse
import json
import os
import socket
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vit_ocm_wmsegmentation_amd  # noqa: E402,F401
from oracle import swin_oracle as SO  # noqa: E402
from vit_ocm_wmsegmentation_amd import _lib, synth  # noqa: E402
from vit_ocm_wmsegmentation_amd import optimizer as OPT  # noqa: E402
from vit_ocm_wmsegmentation_amd import swin as SW  # noqa: E402


ARCHS = {"swin_t": {}, "swin_b_w12": dict(embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="bf16", choices=sorted(_lib.PRECISIONS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--optimizer", default="torch", choices=["torch", "hip"],
                    help="the HIP step's optimizer: torch.optim (default) or optimizer.py's multi-tensor kernels")
    ap.add_argument("--image-size", type=int, default=224, help="square input side, a multiple of the patch size 4")
    ap.add_argument("--no-twin", action="store_true", help="skip the fp32 eager twin (for a kernel trace of the HIP step alone)")
    ints = lambda v: tuple(int(t) for t in v.split(","))  # noqa: E731
    ap.add_argument("--arch", default="swin_t", choices=sorted(ARCHS), help="swin_t, or swin_b_w12 (Swin-B with windows of 12)")
    ap.add_argument("--embed-dim", type=int, help="channels of stage 0 (32-wide heads: 32 * num_heads[0])")
    ap.add_argument("--depths", type=ints, help="layers per stage, comma separated")
    ap.add_argument("--num-heads", type=ints, help="heads per stage, comma separated")
    ap.add_argument("--window-size", type=int, help="2 to 12; above 7 the tool turns enable_wide_window_training on")
    args = ap.parse_args()
    dev, B, S = torch.device("cuda:0"), args.batch, args.image_size
    cfg = dict(synth.SWIN_TINY, **ARCHS[args.arch], image_size=S, num_labels=5)
    for k in ("embed_dim", "depths", "num_heads", "window_size"):
        if getattr(args, k) is not None:
            cfg[k] = getattr(args, k)
    sd = synth.synth_swin_state_dict(cfg, seed=3)
    m = SW.SwinForImageClassification(SW.SwinConfig(**{k: v for k, v in cfg.items() if k != "patch_size"}))
    m.load_state_dict(sd)
    m = m.to(dev).set_precision(args.precision).train().requires_grad_(True)
    tokens, side, ws = [], S // cfg["patch_size"], cfg["window_size"]
    for s in range(len(cfg["depths"])):  # per stage: the grid, and the grid padded to the window the attention runs on
        pad = -(-side // ws) * ws
        tokens.append(dict(stage=s, grid=side, padded_grid=pad, real=side * side, padded=pad * pad,
                           ratio=round(pad * pad / (side * side), 2), odd_merge=bool(side % 2 and s + 1 < len(cfg["depths"]))))
        side = (side + 1) // 2
    needs_padding = any(t["padded"] != t["real"] or t["odd_merge"] for t in tokens)
    if needs_padding:
        m.enable_padded_training()
    if ws > 7:
        m.enable_wide_window_training()
    for t in tokens:
        print(f"stage {t['stage']}: grid {t['grid']}^2 = {t['real']} tokens, padded {t['padded_grid']}^2 = {t['padded']} "
              f"({t['ratio']:.2f}x){', odd merge' if t['odd_merge'] else ''}")
    opt = (OPT.AdamW if args.optimizer == "hip" else torch.optim.AdamW)(m.parameters(), lr=5e-5)
    prm = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
    opt_t = torch.optim.AdamW(list(prm.values()), lr=5e-5)
    torch.manual_seed(0)
    x = torch.rand(B, 3, S, S, device=dev) * 0.3
    y = torch.randint(0, 5, (B,), device=dev)

    def hip_step():
        opt.zero_grad(set_to_none=True)
        tf, out = _timed(lambda: m(pixel_values=x, labels=y))
        tb, _ = _timed(lambda: out.loss.backward())
        to, _ = _timed(opt.step)
        return tf, tb, to

    def twin_step():
        if args.no_twin:
            return float("nan")
        opt_t.zero_grad(set_to_none=True)
        t0 = time.perf_counter()
        with torch.device(dev):  # the oracle builds its index tables and shift masks on the default device
            F.cross_entropy(SO.swin_forward.__wrapped__(prm, cfg, x)["logits"], y).backward()
        opt_t.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        hip_step()
        twin_step()
    rows = {k: [] for k in ("fwd", "bwd", "opt", "step", "twin")}
    for _ in range(args.reps):
        tf, tb, to = hip_step()
        rows["fwd"].append(tf)
        rows["bwd"].append(tb)
        rows["opt"].append(to)
        rows["step"].append(tf + tb + to)
        rows["twin"].append(twin_step())
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    res = dict(box=socket.gethostname(), gpu=torch.cuda.get_device_name(0), arch=args.arch, embed_dim=cfg["embed_dim"],
               depths=list(cfg["depths"]), num_heads=list(cfg["num_heads"]), window_size=ws, wide_window_training=ws > 7,
               batch=B, precision=args.precision, image_size=S,
               padded_training=needs_padding, padded_over_real_tokens=[t["ratio"] for t in tokens],
               ms={k: round(v, 2) for k, v in med.items()}, speedup_vs_eager=round(med["twin"] / med["step"], 2),
               kept_mib_per_image=round(m.__dict__["_train_kept_bytes"] / B / 2 ** 20, 1), reps=args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
