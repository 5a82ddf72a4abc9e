"""The split-bf16 flash attention at every key-tile count and on every branch of its dispatch, against float64 torch.

test_ops_x3_gpu.py puts all but one of its shapes on the wave-split kernel; here every case first asserts through
ocm_attention_plan (csrc/attn_plan.h; the rows are tests/attn_tile_cases.py, asserted without a GPU by test_attn_plan_host.py)
that it runs the kernel it is meant for:

  software-pipelined kernel   1..4 and 32 key tiles with 1, 31 and 32 valid keys in the last, a second workgroup per head whose
                              waves 1-3 have no query, 131 workgroups over the eight XCDs, one input in all 128 (image, head)
                              pairs (bit-identical outputs), deferred-maximum spikes in the first, a middle and the last tile
  key-split kernel + merge    through ocm_op_attention_ws on a guard-banded, NaN-poisoned workspace: four, three and two slices,
                              no split at 130 workgroups, no padding key, one ViT-S/8 window; a workspace one float short; spikes
                              that make all but one merge weight vanish
  128-wide heads              1, 2, 3, 4 and 33 key tiles on the two-stage ring
  wave-split kernel           one tile per wave, then wave 0 with two

The harness and the bounds are test_ops_x3_gpu.py::test_attention_x3's (NaN in every padding row and column; lse 1e-4, context
4e-5, probabilities 2e-5, each times sharp^2) and, for the spike inputs, those of the deferred-maximum test there (2e-4 / 1e-4 /
1e-4 times max(1, largest score / 8)). Every case runs twice and compares bits, and compares the statistics-only call's lse with
the full call's. Each case prints its measured maxima as a GPUTEST line before it asserts (DESIGN.md 3.25 holds them).
"""
import ctypes as C
import math

import pytest
import torch

from tests import attn_tile_cases as T
from tests.memcheck import PATTERNS, Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.engine import from_split, to_operand

pytestmark = pytest.mark.gpu
X3 = _lib.OCM_PREC_BF16X3
NAN = float("nan")
FIELDS = [name for name, _ in _lib.OcmAttentionPlanInfo._fields_][:8]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(lib, rc):
    assert rc == 0, lib.ocm_last_error().decode()


def _plan(lib, B, N, H, hd=64, workspace=0):
    out = _lib.OcmAttentionPlanInfo()
    _ok(lib, lib.ocm_attention_plan(X3, B, N, H, hd, workspace, C.byref(out)))
    return tuple(getattr(out, n) for n in FIELDS)


def _random_qkv(B, N, H, sharp, dev, hd=64, seed=60):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((B * H, N, hd), generator=g) * sharp).to(dev)
    k = (torch.randn((B * H, N, hd), generator=g) * sharp).to(dev)
    v = torch.randn((B * H, N, hd), generator=g).to(dev)
    return q, k, v


def _spike_qkv(B, N, H, spikes, dev):
    """The input of test_attention_x3_deferred_max_is_exact_when_the_maximum_jumps: scores that creep (|q|, |k| ~ 0.5) except at
    the spike keys, whose rows are `height` times a large multiple of two query directions."""
    g = torch.Generator().manual_seed(61)
    q = torch.randn((B * H, N, 64), generator=g) * 0.5
    k = torch.randn((B * H, N, 64), generator=g) * 0.5
    v = torch.randn((B * H, N, 64), generator=g)
    for key, height in spikes.items():
        k[:, key] = height * (6.0 * q[:, N // 2] + 3.0 * q[:, 1])
    return q.to(dev), k.to(dev), v.to(dev)


class Case:
    """One (q, k, v) on the device as NaN-padded split operands, with its float64 reference."""

    def __init__(self, lib, dev, B, N, H, q, k, v, hd=64):
        self.lib, self.dev, self.B, self.N, self.H, self.hd = lib, dev, B, N, H, hd
        self.scale = hd ** -0.5
        npad = lib.ocm_n_pad_prec(X3, N)
        qp = torch.full((B * H, npad, hd), NAN, device=dev)  # padding may hold anything, NaN included
        kp = torch.full((B * H, npad, hd), NAN, device=dev)
        vp = torch.full((B * H, hd, npad), NAN, device=dev)
        qp[:, :N], kp[:, :N], vp[:, :, :N] = q, k, v.transpose(1, 2)
        self.qs, self.ks, self.vs = to_operand(qp, X3), to_operand(kp, X3), to_operand(vp, X3)
        self.s = (q.double() @ k.double().transpose(1, 2)) * self.scale
        self.pref = self.s.softmax(-1)
        self.oref = (self.pref @ v.double()).reshape(B, H, N, hd).permute(0, 2, 1, 3).reshape(B, N, H * hd)
        self.lse_ref = torch.logsumexp(self.s, -1) / math.log(2.0)

    def attention(self, want_ctx=True, workspace=None, workspace_bytes=0):
        """(ctx as fp32 or None, lse) of one call: ocm_op_attention / _hd, or ocm_op_attention_ws when a workspace is given."""
        lib, B, N, H, hd = self.lib, self.B, self.N, self.H, self.hd
        ctx = torch.full((B, N, H * hd), NAN, device=self.dev).view(torch.int32) if want_ctx else None
        lse = torch.full((B * H, N), NAN, device=self.dev)
        if workspace is not None:
            _ok(lib, lib.ocm_op_attention_ws(X3, _p(self.qs), _p(self.ks), _p(self.vs), _p(ctx), _p(lse), B, N, H, hd, self.scale,
                                             C.c_void_p(workspace.ptr), workspace_bytes, _s()))
        elif hd == 64:
            _ok(lib, lib.ocm_op_attention(X3, _p(self.qs), _p(self.ks), _p(self.vs), _p(ctx), _p(lse), B, N, H, self.scale, _s()))
        else:
            _ok(lib, lib.ocm_op_attention_hd(X3, _p(self.qs), _p(self.ks), _p(self.vs), _p(ctx), _p(lse), B, N, H, hd, self.scale,
                                             _s()))
        return (from_split(ctx) if want_ctx else None), lse

    def check(self, tag, bounds, **call):
        """Runs the operator twice plus once without a context, measures against float64, prints, asserts. Returns (ctx, lse)."""
        lib, B, N, H, hd = self.lib, self.B, self.N, self.H, self.hd
        b_lse, b_ctx, b_probs = bounds
        ctx, lse = self.attention(**call)
        ctx2, lse2 = self.attention(**call)
        _, lse3 = self.attention(want_ctx=False, **call)
        e_lse = (lse.double() - self.lse_ref).abs().max().item()
        e_ctx = (ctx.double() - self.oref).abs().max().item()
        attn = torch.full((B, H, N, N), NAN, device=self.dev)
        if hd == 64:
            _ok(lib, lib.ocm_op_attention_probs(X3, _p(self.qs), _p(self.ks), _p(lse), _p(attn), B, N, H, self.scale, _s()))
        else:
            _ok(lib, lib.ocm_op_attention_probs_hd(X3, _p(self.qs), _p(self.ks), _p(lse), _p(attn), B, N, H, hd, self.scale, _s()))
        e_probs = (attn.reshape(B * H, N, N).double() - self.pref).abs().max().item()
        e_sum = (attn.sum(-1) - 1).abs().max().item()
        e_rows = 0.0
        if N > 1 and hd == 64:
            rows_idx = torch.tensor([0, N - 1, N // 2], dtype=torch.int32, device=self.dev)
            rows = torch.full((B, H, 3, N - 1), NAN, device=self.dev)
            _ok(lib, lib.ocm_op_attention_rows(X3, _p(self.qs), _p(self.ks), _p(rows_idx), 3, _p(rows), B, N, H, self.scale, _s()))
            e_rows = (rows.double() - self.pref.reshape(B, H, N, N)[:, :, rows_idx.long(), 1:]).abs().max().item()
        print(f"GPUTEST attention tiles {tag} B={B} N={N} H={H} hd={hd}: lse {e_lse:.2e} (bound {b_lse:.1e}), ctx {e_ctx:.2e} "
              f"({b_ctx:.1e}), probs {e_probs:.2e} ({b_probs:.1e}), rows {e_rows:.2e}, row sums {e_sum:.1e}")
        assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
        assert e_lse < b_lse and e_ctx < b_ctx and e_probs < b_probs and e_rows < b_probs and e_sum < 1e-4
        assert_same_bits(ctx, ctx2, "context of two runs", ("b", "query", "channel"))
        assert_same_bits(lse, lse2, "lse of two runs", ("bh", "query"))
        assert_same_bits(lse, lse3, "lse with and without a context", ("bh", "query"))
        return ctx, lse


def _random_bounds(sharp):
    # test_attention_x3: a score is a sum of products of 2^-17-accurate operands of size ~sharp, so its absolute error, and with
    # it the relative error of every probability, grows with sharp^2
    es = sharp * sharp
    return 1e-4 * es, 4e-5 * es, 2e-5 * es


def _spike_bounds(case):
    # the deferred-maximum test: operand rounding is relative, the score error scales with the largest score; and the jump is
    # far past the threshold of 8 log2 units
    s = case.s
    assert float((s.max(-1).values - s.median(-1).values).max()) * math.log2(math.e) > 16
    es = max(1.0, float(s.abs().max()) / 8)
    return 2e-4 * es, 1e-4 * es, 1e-4 * es


# ---- the software-pipelined kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sharp", [1.0, 3.0])
@pytest.mark.parametrize("B,N,H", sorted(T.PP_CASES))
def test_pipelined_kernel(lib, dev, B, N, H, sharp):
    assert _plan(lib, B, N, H) == T.PP_CASES[(B, N, H)]
    Case(lib, dev, B, N, H, *_random_qkv(B, N, H, sharp, dev)).check(f"pipelined sharp {sharp}", _random_bounds(sharp))


@pytest.mark.parametrize("B,N,H", T.PP_SAME_INPUT)
def test_pipelined_kernel_same_input_in_every_workgroup(lib, dev, B, N, H):
    """One (q, k, v) in all 128 (image, head) pairs: 128 workgroups must return the same bits — a race between waves, a wrong
    workgroup remap or a wrong (image, head) offset that a tolerance would hide."""
    assert _plan(lib, B, N, H) == T.pp_plan(1, B * H)
    q, k, v = (t.expand(B * H, N, 64).contiguous() for t in _random_qkv(1, N, 1, 1.0, dev))
    ctx, lse = Case(lib, dev, B, N, H, q, k, v).check("pipelined, one input in every workgroup", _random_bounds(1.0))
    per_head = ctx.reshape(B, N, H, 64)
    assert_same_bits(per_head, per_head[:1, :, :1].expand(B, N, H, 64), "contexts of the (image, head) pairs", ("b", "query", "head", "channel"))
    assert_same_bits(lse, lse[:1].expand(B * H, N), "lse of the (image, head) pairs", ("bh", "query"))


@pytest.mark.parametrize("B,N,H,spike_at", T.PP_SPIKES)
def test_pipelined_kernel_deferred_max_spike(lib, dev, B, N, H, spike_at):
    """The rescale after deferred tiles in the pipelined kernel's own places: the prologue's block (spike in tile 0), the loop,
    and the masked last tile whose only valid key is the spike."""
    assert _plan(lib, B, N, H)[0] == T.PP
    case = Case(lib, dev, B, N, H, *_spike_qkv(B, N, H, {spike_at: 1.0}, dev))
    case.check(f"pipelined spike at key {spike_at}", _spike_bounds(case))


# ---- the key-split kernel and its merge, as an operator ------------------------------------------------------------------
def _workspace(lib, dev, B, N, H):
    nbytes = lib.ocm_attention_workspace_bytes(X3, B, N, H, 64)
    return Guarded(nbytes, dev, "nan"), nbytes


def _holds_poison(ws):
    return bool((ws.payload(torch.int32) == PATTERNS["nan"]).all())


def _key_split_case(lib, dev, case, tag, bounds):
    """ocm_op_attention_ws on an exact, poisoned, guard-banded workspace against float64 and against ocm_op_attention; then with
    the workspace one float short of what the plan needs."""
    B, N, H = case.B, case.N, case.H
    want = T.KSPLIT_CASES[(B, N, H)]
    ws, nbytes = _workspace(lib, dev, B, N, H)
    assert _plan(lib, B, N, H, 64, nbytes) == want
    assert _plan(lib, B, N, H) == T.dma_plan(want[4], B * H)  # what ocm_op_attention runs: the unsplit eight-wave kernel
    ctx1, lse1 = case.check(f"{tag}, unsplit", bounds)
    ctx, lse = case.check(f"{tag}, {want[3]} slices", bounds, workspace=ws, workspace_bytes=nbytes)
    assert ws.check() is None, ws.check()
    if want[0] != T.KSPLIT:  # 130 workgroups: nothing to offer, the same kernel either way
        assert nbytes == 0
        assert_same_bits(ctx, ctx1, "context with an empty workspace", ("b", "query", "channel"))
        assert_same_bits(lse, lse1, "lse with an empty workspace", ("bh", "query"))
        return
    assert not _holds_poison(ws)  # the slices went through it
    d_ctx, d_lse = (ctx - ctx1).abs().max().item(), (lse - lse1).abs().max().item()
    print(f"GPUTEST attention tiles {tag} split vs unsplit: ctx {d_ctx:.2e}, lse {d_lse:.2e}")
    assert d_lse < bounds[0] and d_ctx < bounds[1]
    need = T.workspace_need((B, N, H), want[3])
    assert nbytes >= need
    ws.fill("nan")
    assert _plan(lib, B, N, H, 64, need - 4) == T.dma_plan(want[4], B * H)
    ctx0, lse0 = case.attention(workspace=ws, workspace_bytes=need - 4)
    assert_same_bits(ctx0, ctx1, "context with a short workspace", ("b", "query", "channel"))
    assert_same_bits(lse0, lse1, "lse with a short workspace", ("bh", "query"))
    assert _holds_poison(ws) and ws.check() is None


@pytest.mark.parametrize("sharp", [1.0, 3.0])
@pytest.mark.parametrize("B,N,H", sorted(T.KSPLIT_CASES))
def test_key_split_operator(lib, dev, B, N, H, sharp):
    case = Case(lib, dev, B, N, H, *_random_qkv(B, N, H, sharp, dev))
    _key_split_case(lib, dev, case, f"key split sharp {sharp}", _random_bounds(sharp))


@pytest.mark.parametrize("name", sorted(T.KSPLIT_SPIKES))
def test_key_split_operator_spikes(lib, dev, name):
    """Slices whose running maxima differ by tens of log2 units: the merge weights of all slices but the spike's underflow or
    nearly do; with one spike per slice of different heights every weight but one is far below 1."""
    B, N, H = 1, 1025, 1
    case = Case(lib, dev, B, N, H, *_spike_qkv(B, N, H, T.KSPLIT_SPIKES[name], dev))
    _key_split_case(lib, dev, case, f"key split spikes {name}", _spike_bounds(case))


# ---- 128-wide heads and the wave-split kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize("sharp", [1.0, 2.0])
@pytest.mark.parametrize("B,N,H", sorted(T.HD128_CASES))
def test_128_wide_heads(lib, dev, B, N, H, sharp):
    """Operands built directly (no projection); scale 128^-0.5, so scores spread as they do for 64-wide heads at 0.125."""
    assert _plan(lib, B, N, H, 128) == T.HD128_CASES[(B, N, H)]
    Case(lib, dev, B, N, H, *_random_qkv(B, N, H, sharp, dev, hd=128), hd=128).check(f"128-wide sharp {sharp}", _random_bounds(sharp))


@pytest.mark.parametrize("sharp", [1.0, 3.0])
@pytest.mark.parametrize("B,N,H", sorted(T.WS_CASES))
def test_wave_split_kernel(lib, dev, B, N, H, sharp):
    assert _plan(lib, B, N, H) == T.WS_CASES[(B, N, H)]
    Case(lib, dev, B, N, H, *_random_qkv(B, N, H, sharp, dev)).check(f"wave-split sharp {sharp}", _random_bounds(sharp))
