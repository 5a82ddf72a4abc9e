#!/usr/bin/env python3
"""Which kernels the GEMM-shaped operators launch, against what ocm_gemm_plan says they launch. Development tool, GPU box only.

    timeout -k 10 280 rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gemm_plan_trace.py run
    python tools/gemm_plan_trace.py check OUT LIST.txt

`run` calls ocm_op_linear, ocm_op_qkv_proj, ocm_op_conv3x3 and ocm_op_linear_resid_ln once at every row of
tests/test_gemm_plan_host.py that those operators can reach (the flagged rows — statistics epilogue, split-K workspace — are the
engine's, and the strided launcher is the Swin engine's). `check` reads the kernel trace of that run, writes the ordered list of
GEMM kernel names to LIST.txt and, where the library has ocm_gemm_plan, asserts for every launch that the GemmCfg<...> arguments,
the ring depth and the K-step count in the kernel's name are the plan's. A library from before ocm_gemm_plan only gets its list
written: two lists from the same LAUNCHES compare with diff.
"""
import csv
import ctypes as C
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vit_ocm_wmsegmentation_amd import _lib  # noqa: E402

BF16, FP32, X3 = _lib.OCM_PREC_BF16, _lib.OCM_PREC_FP32, _lib.OCM_PREC_BF16X3
LINEAR_X3 = [(1000, 384, 384), (333, 384, 1536), (70, 96, 192), (64, 192, 64), (12608, 1536, 384), (12609, 1536, 384),
             (12800, 1536, 384), (12608, 384, 384), (24576, 384, 1536), (32768, 1024, 768), (16384, 512, 384), (20000, 1024, 384),
             (6000, 96, 384), (6000, 288, 96), (5000, 576, 192), (5000, 192, 768), (197, 384, 1536)]
CONV3X3 = [(3, 105, 104, 64, 256), (1, 181, 181, 128, 256), (1, 181, 181, 256, 256), (1, 181, 181, 512, 256), (1, 9, 9, 64, 128),
           (2, 9, 7, 128, 128), (1, 9, 9, 256, 256), (2, 5, 7, 128, 64), (1, 5, 7, 256, 32), (1, 5, 7, 512, 64), (3, 1, 1, 32, 32),
           (1, 1, 9, 64, 64), (2, 6, 1, 32, 64), (1, 3, 3, 4096, 32), (1, 3, 3, 4064, 32)]
# (operator, precision, epilogue, shape): linear (M, N, K); qkv (batch, n_tokens, heads) with 64-wide heads; conv3x3 (B, h, w, C, O);
# resid_ln (M, D, K)
LAUNCHES = ([("linear", X3, e, s) for s in LINEAR_X3 for e in (0, 1, 2, 3)]
            + [("qkv", X3, 0, s) for s in [(64, 197, 6), (26, 577, 12), (3, 197, 6), (5, 50, 3), (2, 17, 2)]]
            + [("linear", BF16, e, s) for s in [(12608, 1536, 384), (12608, 384, 384), (32768, 1024, 768)] for e in (0, 1, 2, 3)]
            + [("qkv", BF16, 0, s) for s in [(26, 577, 12), (64, 197, 6)]]
            + [("linear", FP32, e, (32768, 1024, 768)) for e in (0, 1, 2, 3)]
            # ((1, 5, 7, 512, 64) is a row of the table in single bf16 only: 72 compile-time steps there, 144 run-time ones otherwise)
            + [("conv3x3", p, 0, s) for s in CONV3X3 for p in (FP32, X3, BF16) if p == BF16 or s != (1, 5, 7, 512, 64)]
            + [("resid_ln", p, 0, (12608, D, 384)) for D in (128, 256, 384) for p in (BF16, FP32, X3)])


def gemm_shape(op, shape):
    """(family, M, N, K, flags) of ocm_gemm_plan for a launch (the family and flag values: None in a binding from before it)."""
    const = lambda name: getattr(_lib, name, None)  # noqa: E731
    if op == "linear":
        return (const("OCM_GEMM_LINEAR"),) + tuple(shape) + (0,)
    if op == "qkv":
        B, n, H = shape
        return const("OCM_GEMM_QKV"), B * n, 3 * 64 * H, 64 * H, 0
    if op == "conv3x3":
        B, h, w, Cin, O = shape
        return const("OCM_GEMM_CONV"), B * h * w, O, 9 * Cin, const("OCM_PLAN_CONV3X3")
    M, D, K = shape
    return const("OCM_GEMM_RESID_LN"), M, D, K, 0


def run():
    import torch
    lib = _lib.load()
    dev = torch.device("cuda:0")
    esize = {BF16: 2, FP32: 4, X3: 4}

    def buf(nbytes):  # zeros: only the launch matters here
        return torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=dev)

    def p(t):
        return C.c_void_p(t.data_ptr())

    for op, prec, epi, shape in LAUNCHES:
        fam, M, N, K, _ = gemm_shape(op, shape)
        e = esize[prec]
        if op == "linear":
            a, w, bias, out = buf(M * K * e), buf(N * K * e), buf(N * 4), buf(M * N * 4)
            rc = lib.ocm_op_linear(prec, p(a), p(w), p(bias), p(out) if epi == 1 else None, p(out), M, N, K, epi, None)
        elif op == "qkv":
            B, n, H = shape
            npad = lib.ocm_n_pad_prec(prec, n)
            a, w, bias = buf(M * K * e), buf(N * K * e), buf(N * 4)
            q, k, vt = buf(B * H * npad * 64 * e), buf(B * H * npad * 64 * e), buf(B * H * npad * 64 * e)
            rc = lib.ocm_op_qkv_proj(prec, p(a), p(w), p(bias), p(q), p(k), p(vt), None, B, n, H, None)
        elif op == "conv3x3":
            B, h, wd, Cin, O = shape
            kp = -(-K // (64 if prec == BF16 else 32)) * (64 if prec == BF16 else 32)
            x, w, bias, out = buf(M * Cin * 4), buf(O * kp * e), buf(O * 4), buf(M * O * 4)
            rc = lib.ocm_op_conv3x3(prec, p(x), Cin, p(w), p(bias), p(out), O, B, h, wd, Cin, O, 0, None)
        else:
            a, w, bias, x, g, xn = buf(M * K * e), buf(N * K * e), buf(N * 4), buf(M * N * 4), buf(N * 4), buf(M * N * e)
            rc = lib.ocm_op_linear_resid_ln(prec, p(a), p(w), p(bias), p(x), p(x), p(g), p(g), p(xn), M, N, K, 1e-6, None)
        assert rc == 0, (op, prec, epi, shape, lib.ocm_last_error())
        torch.cuda.synchronize()
    print(f"{len(LAUNCHES)} launches")


KERNEL = re.compile(r"(?<![a-z_])(gemm_kernel|gemm_dma_kernel|qkv_kernel|qkv_dma_kernel)(?![a-z_])")  # (mangled names too)


def parse(name):
    """(bm, bn, waves, mfma16, lds_dma, stages, ksteps) from a demangled or a mangled kernel name."""
    kind = KERNEL.search(name).group(1)
    m = re.search(r"GemmCfg<(\d+), (\d+), (\d+), (\d+)(?:, (\d+))?>, \w+, (?:(?:true|false), )?(\d+)(?:, (\d+))?", name)
    if not m:  # a name the demangler gave up on (bf16 element types)
        m = re.search(r"GemmCfgILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE(?:DF16b|f|4sp32)(?:Lb[01]E)?Li(\d+)E(?:Li(\d+)E)?", name)
    assert m, name
    bm, bn, wm, wn, mf16, ks, st = (int(v) if v else 0 for v in m.groups())
    dma = kind.endswith("dma_kernel")
    return bm, bn, wm * wn, mf16, int(dma), st if dma else 2, ks


def check(outdir, listfile):
    traces = glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(traces) == 1, traces
    rows = list(csv.DictReader(open(traces[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows if KERNEL.search(r["Kernel_Name"])]
    with open(listfile, "w") as f:
        f.write("\n".join(names) + "\n")
    assert len(names) == len(LAUNCHES), f"{len(names)} GEMM kernels in the trace, {len(LAUNCHES)} launches"
    lib = _lib.load()
    if not hasattr(lib, "ocm_gemm_plan"):
        print(f"{len(names)} kernel names written to {listfile} (this library has no ocm_gemm_plan: nothing to compare)")
        return
    for (op, prec, epi, shape), name in zip(LAUNCHES, names):
        fam, M, N, K, flags = gemm_shape(op, shape)
        out = _lib.OcmGemmPlanInfo()
        assert lib.ocm_gemm_plan(fam, prec, epi, M, N, K, flags, C.byref(out)) == 0, lib.ocm_last_error()
        want = (out.bm, out.bn, out.waves, out.mfma16, out.lds_dma, out.stages, out.ksteps)
        assert out.splitk == 1 and parse(name) == want, f"{op} prec {prec} epilogue {epi} {shape}: plan {want}, kernel {name}"
    print(f"{len(names)} launches: every kernel name carries its plan's tile, loop, ring depth and K-step count; list in {listfile}")


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 4 and sys.argv[1] == "check":
        check(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
