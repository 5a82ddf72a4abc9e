#!/usr/bin/env python3
"""Development tool (GPU box): times the split-bf16 (and bf16) nn.Linear kernels and the qkv projection of whichever library
OCM_VIT_LIB names (default: the in-tree build) at the bench shapes (ViT-S/16, B=64: M = 12608). To compare two builds, run it
once per library file.
    python tools/microbench_x3.py [--prec 2] [--iters 30] [--only fc1,fc2,proj,qkv_as_linear,qkv]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402
from vit_ocm_wmsegmentation_amd.engine import to_operand  # noqa: E402


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prec", type=int, default=2)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rows", type=int, default=12608)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    M, D = a.rows, a.dim
    shapes = {"fc1": (M, 4 * D, D, 2), "fc2": (M, D, 4 * D, 1), "proj": (M, D, D, 1), "qkv_as_linear": (M, 3 * D, D, 3)}
    only = set(filter(None, a.only.split(",")))
    for name, (m, n, k, epi) in shapes.items():
        if only and name not in only:
            continue
        x = torch.randn((m, k), generator=g).to(dev)
        w = (torch.randn((n, k), generator=g) * 0.02).to(dev)
        bias = torch.randn((n,), generator=g).to(dev)
        xa, wa = to_operand(x, a.prec), to_operand(w, a.prec)
        act_out = epi in (2, 3)
        odt = torch.float32 if not act_out else {0: torch.bfloat16, 1: torch.float32, 2: torch.int32}[a.prec]
        resid = torch.randn((m, n), generator=g).to(dev)
        out = torch.empty((m, n), dtype=odt, device=dev)

        def fn():  # (the residual epilogue reads resid and writes out: no in-place accumulation drift)
            return lib.ocm_op_linear(a.prec, p(xa), p(wa), p(bias), p(resid) if epi == 1 else None, p(out), m, n, k, epi, s())
        assert fn() == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        us = timeit(fn, a.iters)
        fl = 2.0 * m * n * k
        print(f"{name:14s}: {us:8.2f} us  {fl / us / 1e6:7.1f} TFLOP/s (algorithmic)")
    if not only or "qkv" in only:  # the real qkv projection (head-major q / k / V^T scatter epilogues)
        B, N, H = M // 197, 197, D // 64
        x = torch.randn((B * N, D), generator=g).to(dev)
        w = (torch.randn((3 * D, D), generator=g) * 0.02).to(dev)
        bias = torch.randn((3 * D,), generator=g).to(dev)
        xa, wa = to_operand(x, a.prec), to_operand(w, a.prec)
        npad = lib.ocm_n_pad_prec(a.prec, N)
        edt = {0: torch.bfloat16, 1: torch.float32, 2: torch.int32}[a.prec]
        q = torch.zeros((B * H, npad, 64), dtype=edt, device=dev)
        k = torch.zeros_like(q)
        vt = torch.zeros((B * H, 64, npad), dtype=edt, device=dev)

        def fn():
            return lib.ocm_op_qkv_proj(a.prec, p(xa), p(wa), p(bias), p(q), p(k), p(vt), None, B, N, H, s())
        assert fn() == 0, lib.ocm_last_error()
        torch.cuda.synchronize()
        us = timeit(fn, a.iters)
        print(f"qkv (B={B})    : {us:8.2f} us  {2.0 * B * N * D * 3 * D / us / 1e6:7.1f} TFLOP/s (algorithmic)")


if __name__ == "__main__":
    main()
