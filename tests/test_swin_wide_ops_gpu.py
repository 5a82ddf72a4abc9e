"""ocm_op_swin_window_attention and ocm_op_swin_window_probs on windows of 8 to 12 (the wide kernels: one workgroup of
ceil(ws^2 / 32) wavefronts per (window, head)) against float64 on the values the element format holds — the rule of
tests/test_swin_outputs_gpu.py, whose bounds apply unchanged: a softmax row is a convex combination, more keys do not widen it.

  probabilities  OP_BOUND of tests/test_swin_outputs_gpu.py (fp32 1.4e-6, split-bf16 1.8e-5, bf16 9e-7), and 1e-3 whatever
                 was measured in fp32 and split-bf16 (ATTENTION_MAP_BAR)
  context        the tolerances of tests/test_swin.py::test_window_attention_op (fp32 2e-5, split-bf16 1e-4, bf16 2e-2)

A = ws^2 = 64 is the full-tile edge (no padding key); 81, 100, 121 and 144 leave 17, 4, 25 and 16 real keys and queries in the
last 32-tile. Grids: one window; 2 x 2 windows with and without a shift (every masked class: last row, last column, corner);
3 x 3 shifted at ws 8 and 12 (interior windows skip the mask). Rows are wider than 3 * 32 * heads / 32 * heads: the q | k | v
padding columns hold -1 and must not be read, the context's padding columns and the rows behind the tokens hold NaN and must
not be written.
"""
import pytest
import torch

from tests import swin_wide_ref as WR
from tests import test_swin as TS
from tests.test_swin_outputs_gpu import ATTENTION_MAP_BAR, OP_BOUND
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.engine import from_split, to_operand

pytestmark = pytest.mark.gpu

# precision -> tolerance of the context, as tests/test_swin.py parametrises test_window_attention_op
CTX_TOL = dict(next(m for m in TS.test_window_attention_op.pytestmark
                    if m.name == "parametrize" and m.args[0] == "precision,tol").args[1])
assert set(CTX_TOL) == {"fp32", "bf16", "bf16x3"}

PAD = 32      # extra columns of every row (whole 16-byte pieces in each format)
TAIL = 3      # context rows behind the tokens


def _inputs(B, H, W, ws, heads, seed, q_gain=1.0):
    g = torch.Generator().manual_seed(seed)
    Cn = 32 * heads
    qkv = torch.randn(B * H * W, 3 * Cn, generator=g)
    qkv[:, :Cn] *= q_gain
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    return qkv, table


def _run(lib, dev, precision, qkv, table, B, H, W, ws, shift, heads):
    """-> (ctx, probs, float64 ctx, float64 probs): both operators on rows of stride 3 * 32 * heads + PAD / 32 * heads + PAD."""
    pc = _lib.PRECISIONS[precision]
    T, Cn = B * H * W, 32 * heads
    ld, ldc = 3 * Cn + PAD, Cn + PAD
    wide = torch.full((T, ld), -1.0)
    wide[:, :3 * Cn] = qkv
    op = to_operand(wide.to(dev), pc)
    held = (wide.to(dev) if precision == "fp32" else from_split(op) if precision == "bf16x3" else op.float())[:, :3 * Cn]
    tb = table.to(dev)
    if precision == "bf16x3":
        ctx = torch.full((T + TAIL, ldc), -1, dtype=torch.int32, device=dev)  # 0xFFFF pairs: NaN + NaN
    else:
        ctx = torch.full((T + TAIL, ldc), float("nan"), dtype=torch.float32 if precision == "fp32" else torch.bfloat16, device=dev)
    fill = ctx.clone()
    A, nW = ws * ws, (H // ws) * (W // ws)
    probs = torch.full((B * nW, heads, A, A), float("nan"), device=dev)
    n = lib.ocm_swin_window_scratch_floats(ws, heads)
    assert n > 0
    scratch = torch.full((n,), float("nan"), device=dev)
    _lib.check(lib.ocm_op_swin_window_attention(pc, op.data_ptr(), ld, ctx.data_ptr(), ldc, tb.data_ptr(), scratch.data_ptr(),
                                                B, H, W, ws, shift, heads, None))
    scratch.fill_(float("nan"))
    _lib.check(lib.ocm_op_swin_window_probs(pc, op.data_ptr(), ld, probs.data_ptr(), tb.data_ptr(), scratch.data_ptr(),
                                            B, H, W, ws, shift, heads, None))
    torch.cuda.synchronize()
    # nothing outside the tokens' own columns is written
    assert torch.equal(ctx[T:].view(torch.uint8), fill[T:].view(torch.uint8)), "rows behind the tokens were written"
    assert torch.equal(ctx[:T, Cn:].contiguous().view(torch.uint8), fill[:T, Cn:].contiguous().view(torch.uint8)), \
        "padding columns of the context were written"
    got = (from_split(ctx[:T].contiguous()) if precision == "bf16x3" else ctx[:T].float())[:, :Cn]
    want_ctx, want_p = WR.window_context(held.cpu().double(), B, H, W, heads, ws, shift, table.double())
    return got, probs, want_ctx, want_p


def _err(got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all()
    return float((got - want).abs().max())


def _cases(ws):
    """(H = W, shift, heads, B)"""
    few = ((1, 2), (3, 1), (4, 2))
    out = [(ws, 0, h, b) for h, b in few]
    out += [(2 * ws, shift, h, b) for shift in (0, ws // 2) for h in (1, 3, 4) for b in (1, 2)]
    if ws in (8, 12):
        out += [(3 * ws, ws // 2, h, b) for h, b in few]
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("ws", [8, 9, 10, 11, 12])
def test_wide_window_operators(lib, dev, ws, precision):
    worst_p, worst_c, worst_sum, worst_masked = 0.0, 0.0, 0.0, 0.0
    seed = 1000 * ws
    for H, shift, heads, B in _cases(ws):
        seed += 1
        qkv, table = _inputs(B, H, H, ws, heads, seed)
        ctx, probs, want_ctx, want_p = _run(lib, dev, precision, qkv, table, B, H, H, ws, shift, heads)
        worst_c, worst_p = max(worst_c, _err(ctx, want_ctx)), max(worst_p, _err(probs, want_p))
        worst_sum = max(worst_sum, float((probs.double().sum(-1) - 1).abs().max()))
        m = WR.masked_entries(H, H, ws, shift)
        if m is not None:
            nW = m.shape[0]
            sel = m.view(1, nW, 1, ws * ws, ws * ws).expand(B, nW, heads, -1, -1).reshape(probs.shape)
            assert bool(sel.any())
            worst_masked = max(worst_masked, float(probs.cpu()[sel].max()))
    # a rerun of the last case: the same bits from both operators
    ctx2, probs2, _, _ = _run(lib, dev, precision, qkv, table, B, H, H, ws, shift, heads)
    print(f"GPUTEST swin wide ops ws{ws} {precision}: probs {worst_p:.2e}, ctx {worst_c:.2e}, row sums {worst_sum:.2e}, "
          f"masked {worst_masked:.2e}")
    assert torch.equal(ctx2, ctx) and torch.equal(probs2, probs), "a rerun gives other bits"
    assert worst_sum <= 1e-5
    assert worst_masked <= 1e-30
    assert worst_p <= OP_BOUND[precision], worst_p
    if precision != "bf16":
        assert worst_p <= ATTENTION_MAP_BAR
    assert worst_c <= CTX_TOL[precision], worst_c


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_wide_window_operators_peaked(lib, dev, precision):
    """q scaled by 3, the smallest whole gain at which the float64 reference's largest probability exceeds 0.99 (0.9985 at ws 12,
    0.9982 at ws 9; asserted on the reference itself): rows with one dominant key next to near-uniform ones. ws 12 (five tiles,
    16 keys in the last) and ws 9 (three tiles, 17 keys). The bounds are those of the unpeaked cases; for scale, the same
    operator evaluated in fp32 by torch on the CPU is 7.9e-7 (probabilities) / 2.9e-6 (context) from float64 here, and larger
    gains saturate the rows (gain 8: largest probability 1.0000, the CPU's own fp32 evaluation 2.3e-6 off)."""
    for ws, heads, B, seed in ((12, 3, 1, 77), (9, 4, 2, 78)):
        H = 2 * ws
        qkv, table = _inputs(B, H, H, ws, heads, seed, q_gain=3.0)
        ctx, probs, want_ctx, want_p = _run(lib, dev, precision, qkv, table, B, H, H, ws, 0, heads)
        assert float(want_p.max()) > 0.99
        e_p, e_c = _err(probs, want_p), _err(ctx, want_ctx)
        sums = float((probs.double().sum(-1) - 1).abs().max())
        print(f"GPUTEST swin wide ops peaked ws{ws} {precision}: max p {float(want_p.max()):.4f}, probs {e_p:.2e}, ctx {e_c:.2e}, "
              f"row sums {sums:.2e}")
        assert sums <= 1e-5
        assert e_p <= OP_BOUND[precision], e_p
        if precision != "bf16":
            assert e_p <= ATTENTION_MAP_BAR
        assert e_c <= CTX_TOL[precision], e_c
