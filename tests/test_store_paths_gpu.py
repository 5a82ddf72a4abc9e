"""How two split-bf16 kernels move their results to memory (the arithmetic is covered by tests/test_ops_x3_gpu.py):

* the V third of attn.qkv (gemm_kernels.h::EpiVt) writes V^T in aligned groups of eight tokens of the DESTINATION — two
  16-byte stores — wherever such a group lies inside the tile, and the at most seven tokens at either end of an image
  segment one by one. The shapes put image boundaries at every kind of place inside a tile; padding columns must stay
  untouched (they share 128-byte groups with valid keys).
* the probabilities of one block (kernels_attn.hip::attn_probs_x3_span_kernel for rows of up to 255 tokens, the
  tile-per-wave kernel beyond) leave as 16-byte stores over the contiguous span of 32 query rows, the <= 3 floats at either
  end of a span one by one: the output sits between sentinels at every 4-byte offset inside a 16-byte group.
* the selected rows, written by the same launch for short lists (kernels_attn.hip::PROBS_FOLD_ROWS) and by
  rows_from_probs_kernel for longer ones, are a slice of the probabilities bit for bit.
Runs on a real MI355X only."""
import ctypes as C
import math

import pytest
import torch

from tests.helpers import CASES, build_module, case_inputs
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.engine import from_split, to_operand

pytestmark = pytest.mark.gpu
X3, F32, BF16 = _lib.OCM_PREC_BF16X3, _lib.OCM_PREC_FP32, _lib.OCM_PREC_BF16


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.ocm_last_error().decode()


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# V^T
# ---------------------------------------------------------------------------------------------------------------------
# (B, N, H); M = B N token rows. Fewer than 1025 rows: 64-row tiles; (26, 577, 12) is the smallest shape of
# test_qkv_proj_x3 that takes the 256 x 256 tile; (20, 197, 6) has enough rows for the 128-row tiles of the LDS-DMA kernel.
#   (5, 37, 2)   odd N, one or two image boundaries inside a tile      (9, 17, 2)  up to eight images inside one tile
#   (3, 7, 2)    N < 8: no aligned group anywhere                      (4, 8, 2)   every image is exactly one group
#   (2, 200, 2)  N % 8 == 0, tiles straddle images                     (3, 197, 2), (1, 577, 12)  the model's odd N
VT_SHAPES = [(5, 37, 2), (9, 17, 2), (3, 7, 2), (4, 8, 2), (2, 200, 2), (3, 197, 2), (1, 577, 12), (26, 577, 12),
             (20, 197, 6)]


def _qkv_case(lib, dev, prec, B, N, H):
    """Runs ocm_op_qkv_proj on zero-filled destinations; returns (q, k, vt, qkv32) as fp32 tensors and the float64 product."""
    D = H * 64
    a, w, bias = _rand((B * N, D), dev, 50), _rand((3 * D, D), dev, 51, 0.05), _rand((3 * D,), dev, 52, 0.1)
    if prec == BF16:  # the reference is the product of the operands the kernel is given
        a, w = a.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
    npad = lib.ocm_n_pad_prec(prec, N)
    assert npad >= N
    dt = {X3: torch.int32, F32: torch.float32, BF16: torch.bfloat16}[prec]
    q = torch.zeros((B * H, npad, 64), dtype=dt, device=dev)
    k = torch.zeros_like(q)
    vt = torch.zeros((B * H, 64, npad), dtype=dt, device=dev)
    qkv32 = torch.full((3, B, H, N, 64), float("nan"), device=dev)
    a_s, w_s = to_operand(a, prec), to_operand(w, prec)  # named: the operands must outlive the call
    _ok(lib, lib.ocm_op_qkv_proj(prec, _p(a_s), _p(w_s), _p(bias), _p(q), _p(k), _p(vt), _p(qkv32), B, N, H, _s()))
    ref = (a.double() @ w.double().t() + bias.double()).reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    val = from_split if prec == X3 else (lambda t: t.float())
    return val(q), val(k), val(vt), qkv32, ref


def _check_qkv(q, k, vt, qkv32, ref, B, N, H, tol):
    BH = B * H
    e32 = (qkv32.double() - ref).abs().max().item()
    eq = (q[:, :N].double() - ref[0].reshape(BH, N, 64)).abs().max().item()
    ek = (k[:, :N].double() - ref[1].reshape(BH, N, 64)).abs().max().item()
    ev = (vt[:, :, :N].double() - ref[2].reshape(BH, N, 64).transpose(1, 2)).abs().max().item()
    print(f"GPUTEST qkv store paths B={B} N={N} H={H}: qkv32 {e32:.2e} q {eq:.2e} k {ek:.2e} vt {ev:.2e} (bound {tol:.2e})")
    assert e32 < tol and eq < tol and ek < tol and ev < tol
    assert (q[:, N:] == 0).all() and (k[:, N:] == 0).all()  # padding rows are never written
    assert (vt[:, :, N:] == 0).all()  # nor the padding columns, inside 128-byte groups of valid keys


@pytest.mark.parametrize("B,N,H", VT_SHAPES)
def test_vt_stores_x3(lib, dev, B, N, H):
    q, k, vt, qkv32, ref = _qkv_case(lib, dev, X3, B, N, H)
    _check_qkv(q, k, vt, qkv32, ref, B, N, H, 3e-5 * max(1.0, math.sqrt(H * 64) / 8))


def test_vt_stores_fp32_and_bf16_untouched(lib, dev):
    """The other two element types keep the token-per-lane form, under the bounds of test_qkv_proj_fp32 and test_qkv_proj:
    fp32 2e-5; single bf16: exact products of bf16 operands summed in fp32 (2e-4), then q / k / V^T rounded to bf16, whose
    unit roundoff is 2^-8 of each value."""
    B, N, H = 5, 37, 2
    q, k, vt, qkv32, ref = _qkv_case(lib, dev, F32, B, N, H)
    _check_qkv(q, k, vt, qkv32, ref, B, N, H, 2e-5)
    q, k, vt, qkv32, ref = _qkv_case(lib, dev, BF16, B, N, H)
    assert (qkv32.double() - ref).abs().max().item() < 2e-4
    want = (ref[0].reshape(B * H, N, 64), ref[1].reshape(B * H, N, 64), ref[2].reshape(B * H, N, 64).transpose(1, 2))
    for got, r in zip((q[:, :N], k[:, :N], vt[:, :, :N]), want):
        assert ((got.double() - r).abs() <= r.abs() * 2 ** -8 + 1e-5).all()
    assert (q[:, N:] == 0).all() and (k[:, N:] == 0).all() and (vt[:, :, N:] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# probabilities
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 64  # sentinel floats in front of and behind the output
SENTINEL = -7.0  # no probability


def _probs_case(lib, dev, B, N, H, HD, sharp):
    """Operands with NaN padding, the log-sum-exp from the attention operator, the float64 softmax."""
    g = torch.Generator().manual_seed(60)
    q = (torch.randn((B * H, N, HD), generator=g) * sharp).to(dev)
    k = (torch.randn((B * H, N, HD), generator=g) * sharp).to(dev)
    npad = lib.ocm_n_pad_prec(X3, N)
    nan = float("nan")
    qp = torch.full((B * H, npad, HD), nan, device=dev)
    kp = torch.full((B * H, npad, HD), nan, device=dev)
    qp[:, :N], kp[:, :N] = q, k
    qs, ks = to_operand(qp, X3), to_operand(kp, X3)
    vs = to_operand(torch.zeros((B * H, HD, npad), device=dev), X3)
    scale = HD ** -0.5
    pref = ((q.double() @ k.double().transpose(1, 2)) * scale).softmax(-1)
    lse = torch.empty((B * H, N), device=dev)
    if HD == 64:
        _ok(lib, lib.ocm_op_attention(X3, _p(qs), _p(ks), _p(vs), None, _p(lse), B, N, H, scale, _s()))
    else:
        _ok(lib, lib.ocm_op_attention_hd(X3, _p(qs), _p(ks), _p(vs), None, _p(lse), B, N, H, HD, scale, _s()))
    return qs, ks, lse, scale, pref


# (B, N, H, HD). One partial tile; one row into the second query block; the model's N = 197 (seven key tiles over four
# waves, a last block of five rows); 577 and 2305: rows too long for the span kernel; (16, 33, 8): 256 spans through the XCD
# remap; 128-wide heads on the span kernel, and at 300 tokens on the tile-per-wave kernel with its key split.
PROBS_SHAPES = [(1, 5, 1, 64), (2, 33, 2, 64), (3, 197, 3, 64), (1, 577, 2, 64), (1, 2305, 1, 64), (16, 33, 8, 64),
                (1, 255, 1, 64), (1, 256, 1, 64), (2, 65, 3, 128), (1, 300, 2, 128)]


@pytest.mark.parametrize("B,N,H,HD", PROBS_SHAPES)
@pytest.mark.parametrize("sharp", [1.0, 3.0])
def test_probs_between_sentinels_at_every_offset(lib, dev, B, N, H, HD, sharp):
    qs, ks, lse, scale, pref = _probs_case(lib, dev, B, N, H, HD, sharp)
    # a score is a sum of HD products of 2^-17-accurate operands of size ~sharp, times HD^-1/2: its error, and the relative
    # error of every probability, grows with sharp^2 at either head width (the bound of test_attention_x3)
    es = sharp * sharp
    total = B * H * N * N
    first = None
    for off in range(4):
        # the allocation is 256-byte aligned, the body starts 4 off bytes past a 16-byte boundary: so does every (b, h) slab
        # whose N N is a multiple of four, and the others take the remaining residues
        buf = torch.full((2 * GUARD + total + 4,), SENTINEL, device=dev)
        assert buf.data_ptr() % 16 == 0
        body = buf[GUARD + off:GUARD + off + total]
        if HD == 64:
            _ok(lib, lib.ocm_op_attention_probs(X3, _p(qs), _p(ks), _p(lse), _p(body), B, N, H, scale, _s()))
        else:
            _ok(lib, lib.ocm_op_attention_probs_hd(X3, _p(qs), _p(ks), _p(lse), _p(body), B, N, H, HD, scale, _s()))
        assert (buf[:GUARD + off] == SENTINEL).all() and (buf[GUARD + off + total:] == SENTINEL).all(), f"offset {off}"
        attn = body.reshape(B * H, N, N)
        err = (attn.double() - pref).abs().max().item()
        rs = (attn.sum(-1) - 1).abs().max().item()
        print(f"GPUTEST probs store paths B={B} N={N} H={H} hd={HD} sharp={sharp} offset={off}: {err:.2e} "
              f"(bound {2e-5 * es:.1e}), row sums {rs:.2e}")
        assert err < 2e-5 * es, f"offset {off}"
        assert rs < 1e-4, f"offset {off}"
        if first is None:
            first = attn.clone()
        else:
            assert torch.equal(attn, first), f"offset {off}: not the bits of offset 0"


# ---------------------------------------------------------------------------------------------------------------------
# selected rows through the engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(dev):
    case = CASES["tiny_p8"]
    return build_module(case, dev), [x.to(dev) for x in case_inputs(case)]


@pytest.mark.parametrize("last_only", [True, False], ids=["last_attn_only", "whole_forward"])
def test_rows_are_a_slice_of_the_probabilities(tiny, dev, last_only):
    """tiny_p8: N = 17 and N = 25 (two inputs). Lists up to the fold limit come from the probabilities launch itself, the
    twelve-entry list from rows_from_probs_kernel."""
    model, inputs = tiny
    flags = _lib.OCM_OUT_ATTN | _lib.OCM_OUT_ROWS | (_lib.OCM_LAST_ATTN_ONLY if last_only else 0)
    for x in inputs:
        N = (x.shape[2] // 8) * (x.shape[3] // 8) + 1
        for queries in ([0], [0, N - 1, N // 2], [3, 3], [0, 1, 2, 3, 4, 5, 6, 7], list(range(N - 1, N - 13, -1))):
            qr = torch.tensor(queries, dtype=torch.int32, device=dev)
            out = model._run(x, flags=flags, query_rows=qr)
            rows, attn = out["rows"], out["attn"][0]
            assert rows.shape == (x.shape[0], 2, len(queries), N - 1)
            assert torch.equal(rows, attn[:, :, queries, 1:]), f"N={N} query_rows={queries}"
            assert (attn.sum(-1) - 1).abs().max().item() < 1e-4


def test_rows_are_a_slice_of_the_probabilities_vit_small(dev):
    """ViT-S/16 at B = 3 (N = 197: seven query blocks per head, the requested rows in three of them), bench.py's flags."""
    case = CASES["vits16_full"]
    model = build_module(case, dev)
    x = torch.cat([case_inputs(case)[0], case_inputs(case)[0][:1].flip(-1)]).to(dev)
    N = 197
    flags = _lib.OCM_OUT_ATTN | _lib.OCM_OUT_ROWS | _lib.OCM_LAST_ATTN_ONLY
    for queries in ([0], [0, N - 1, N // 2], [3, 3], list(range(0, 180, 20))):
        qr = torch.tensor(queries, dtype=torch.int32, device=dev)
        out = model._run(x, flags=flags, query_rows=qr)
        rows, attn = out["rows"], out["attn"][0]
        assert rows.shape == (3, 6, len(queries), N - 1)
        assert torch.equal(rows, attn[:, :, queries, 1:]), f"query_rows={queries}"
