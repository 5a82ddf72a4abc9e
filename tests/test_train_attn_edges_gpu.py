"""The two attention backwards at the inputs and shapes training produces and their own tests do not: token counts on and next
to a multiple of the walked tile (32) and of the owned block (128), scales other than hd ** -0.5, grids far above the CU
count, the batch * heads refusal, peaked logits (the float64 softmax's median row maximum at least 0.8) under a forward in each
precision, the delta operator at rows that are not a multiple of four; for the Swin window attention a peaked case, windows
whose rows keep a single unmasked key under table entries of +-30, and three first-level chunks of the table gradient.

Every comparison is against float64 torch on the CPU, every operator runs twice (torch.equal) and every output starts as NaN.
Where a bound is "4x eager", the test measures torch's own fp32 autograd on the CPU against the same float64 reference on the
same inputs and allows the kernel four times that error (it sums 32-wide tiles in another order and uses the hardware exp2),
never less than the bound the unpeaked tests hold. Needs an MI355X."""
import pytest
import torch

from oracle import swin_oracle as SO
from tests.test_mim_train_ops_gpu import PRECS, _attention_ref, _attention_run
from tests.test_swin import _window_attention_oracle
from tests.test_swin_train_ops_gpu import _wattn_bwd
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.engine import _p, _stream, from_split, to_operand

pytestmark = pytest.mark.gpu

ATTN_BOUND = 1e-4  # test_attention_backward_matches_float64: per block of dqkv, relative to the block's max
CTX_BOUND = 1e-5
MODE_TOL = {"fp32": 1e-4, "bf16x3": 1e-3, "bf16": 5e-2}  # TOL of tests/test_mim_train_gpu.py
WATTN_BOUND = 2e-5  # test_window_attention_backward_vs_float64
PEAK_GAIN = 3.5  # q and k ~ N(0, 3.5^2): logit sigma 12, |logit| up to ~65; median row maximum 0.90 .. 0.94 (asserted below)


def _worst(got, want, den=None):
    """(max |got - want| / den, index, got there, want there); den defaults to max |want|."""
    d = (got.detach().double().cpu() - want).abs()
    i = int(d.argmax())
    den = float(want.abs().max()) if den is None else den
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), d.shape))
    return float(d.flatten()[i]) / max(den, 1e-300), idx, float(got.detach().flatten()[i]), float(want.flatten()[i])


def _case(B, H, N, hd, seed, gain=1.5):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(3, B, H, N, hd, generator=g, dtype=torch.float64)
    qkv[:2] *= gain
    do = torch.randn(B, N, H * hd, generator=g, dtype=torch.float64)
    do[:, : N // 2] *= 1e-3  # mixed scale
    return qkv, do


def _check_blocks(dqkv, ref, D, N, bounds, what):
    """dQ | dK | dV each against its own maximum (with one token dQ = dK = 0 exactly: against the whole gradient)."""
    for which, name in enumerate(("dq", "dk", "dv")):
        blk, rblk = dqkv[:, which * D:(which + 1) * D], ref[:, which * D:(which + 1) * D]
        den = float(rblk.abs().max()) if N > 1 else float(ref.abs().max())
        e, idx, got, want = _worst(blk, rblk, den)
        print(f"GPUTEST attention backward {what} {name}: {e:.3e} (bound {bounds[which]:.1e}) worst at {idx}: got {got!r} want {want!r}")
        assert e <= bounds[which], f"{what} {name}: {e:.3e} > {bounds[which]:.1e} at {idx}: got {got!r}, want {want!r}"


def _run_and_compare(dev, qkv64, do64, scale, what):
    _, B, H, N, hd = qkv64.shape
    (dqkv, delta, c32), (dqkv2, delta2, c322) = _attention_run(qkv64, do64, scale, dev)
    ref, ctx64 = _attention_ref(qkv64, do64, scale)
    assert torch.equal(dqkv, dqkv2) and torch.equal(delta, delta2) and torch.equal(c32, c322), what
    assert not torch.isnan(dqkv).any(), what
    e, idx, got, want = _worst(c32, ctx64.reshape(B * N, -1))
    assert e <= CTX_BOUND, f"{what} context: {e:.3e} at {idx}: got {got!r}, want {want!r}"
    _check_blocks(dqkv, ref, H * hd, N, [ATTN_BOUND] * 3, what)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("N", [31, 32, 33, 127, 128, 129, 256, 577])
def test_attention_backward_tile_edge_token_counts(dev, hd, N):
    """N on and next to 32 (the walked tile) and 128 (the owned block): `q0 + r < N` / `key0 + kk < N` go from some lanes to
    none, and the last workgroup owns 1, 32 or 128 live rows."""
    B, H = 2, 3
    qkv64, do64 = _case(B, H, N, hd, seed=7 * N + hd)
    _run_and_compare(dev, qkv64, do64, hd ** -0.5, f"N={N} hd={hd}")


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("scale", [0.05, 0.3])
def test_attention_backward_other_scales(dev, hd, scale):
    """The ABI takes any scale: dQ and dK carry it once each, the recomputed logits through c2 = scale * log2(e)."""
    qkv64, do64 = _case(2, 3, 197, hd, seed=int(scale * 100) + hd)
    _run_and_compare(dev, qkv64, do64, scale, f"scale={scale} hd={hd}")


@pytest.mark.parametrize("hd", [64, 128])
def test_attention_backward_many_heads(dev, hd):
    """batch * heads = 520 at N = 33: grid y of twice the CU count, one workgroup of one live wave plus one row per head."""
    qkv64, do64 = _case(130, 4, 33, hd, seed=520 + hd)
    _run_and_compare(dev, qkv64, do64, hd ** -0.5, f"BxH=520 hd={hd}")


def test_attention_backward_refuses_65536_heads(dev):
    """batch * heads = 65536 exceeds grid y: OCM_EINVAL before any launch. The buffers have the full size the call describes
    (about 50 MB each for qkv and dqkv), and dqkv keeps the NaN it started with."""
    lib = _lib.load()
    B, H, N, hd = 16384, 4, 1, 64
    D = H * hd
    qkv = torch.zeros((3, B, H, N, hd), device=dev)
    lse, delta = torch.zeros((B * H, N), device=dev), torch.zeros((B * H, N), device=dev)
    do = torch.zeros((B * N, D), device=dev)
    dqkv = torch.full((B * N, 3 * D), float("nan"), device=dev)
    with torch.cuda.device(dev):
        rc = lib.ocm_op_attention_backward(_p(qkv), _p(lse), _p(do), _p(delta), _p(dqkv), B, N, H, hd, hd ** -0.5, _stream())
    torch.cuda.synchronize()
    assert rc == _lib.OCM_EINVAL
    assert bool(torch.isnan(dqkv).all())


def _softmax64(qkv64, scale):
    return (qkv64[0] @ qkv64[1].transpose(-1, -2) * scale).softmax(-1)


def _eager_fp32(qkv64, do64, scale):
    """torch's own fp32 autograd on the CPU for the same inputs: (dqkv, ctx, P column sums)."""
    ref, ctx = _attention_ref(qkv64.float(), do64.float(), scale)
    return ref, ctx, _softmax64(qkv64.float(), scale).sum(-2)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("N", [197, 785])
def test_attention_backward_peaked_logits(dev, N, hd, prec):
    """Logits in the tens. The backward recomputes P = exp2(s c2 - lse2) from fp32 q and k against the lse2 of a forward that in
    bf16 / split-bf16 mode ran on rounded operands: the rows of P then no longer sum to one exactly.

    fp32 forward: each block within 4x the fp32-eager CPU error (never less than 1e-4). Split-bf16 forward: 1e-3. bf16 forward: not
    claimed on peaked attention, printed; finite and bitwise reproducible. In every mode, with dO = 1, dV[key] equals the column sum
    of the recomputed P: per key against the float64 column sums and in total against B H N, within the mode's tolerance.

    Measured on the MI355X (max over N and hd): see DESIGN.md 3.19."""
    B, H = (1, 3) if N >= 785 else (2, 3)
    D, scale = H * hd, hd ** -0.5
    qkv64, do64 = _case(B, H, N, hd, seed=N + hd, gain=PEAK_GAIN)
    p64 = _softmax64(qkv64, scale)
    median = float(p64.max(-1).values.median())
    assert median >= 0.8, f"the case went soft: median row maximum {median:.3f}"
    ref, ctx64 = _attention_ref(qkv64, do64, scale)
    blocks = [float(ref[:, i * D:(i + 1) * D].abs().max()) for i in range(3)]
    assert min(blocks) >= 1e-6 * max(blocks), blocks  # a relative bound never divides by noise
    eref, ectx, ecol = _eager_fp32(qkv64, do64, scale)
    eager = [_worst(eref[:, i * D:(i + 1) * D], ref[:, i * D:(i + 1) * D])[0] for i in range(3)]
    eager_ctx = _worst(ectx.reshape(B * N, -1), ctx64.reshape(B * N, -1))[0]
    what = f"peaked N={N} hd={hd} {prec} (median row max {median:.3f})"
    print(f"GPUTEST attention backward {what}: fp32 eager CPU dq {eager[0]:.3e} dk {eager[1]:.3e} dv {eager[2]:.3e} "
          f"ctx {eager_ctx:.3e}")

    (dqkv, delta, c32), (dqkv2, delta2, c322) = _attention_run(qkv64, do64, scale, dev, PRECS[prec])
    assert torch.equal(dqkv, dqkv2) and torch.equal(delta, delta2) and torch.equal(c32, c322), what
    assert bool(torch.isfinite(dqkv).all()), what
    if prec == "fp32":
        e, idx, got, want = _worst(c32, ctx64.reshape(B * N, -1))
        print(f"GPUTEST attention backward {what} ctx: {e:.3e} (eager {eager_ctx:.3e})")
        assert e <= max(CTX_BOUND, 4 * eager_ctx), f"{what} context: {e:.3e} at {idx}: got {got!r}, want {want!r}"
        _check_blocks(dqkv, ref, D, N, [max(ATTN_BOUND, 4 * x) for x in eager], what)
    elif prec == "bf16x3":
        _check_blocks(dqkv, ref, D, N, [MODE_TOL[prec]] * 3, what)
    else:
        e, idx, got, want = _worst(dqkv, ref)
        print(f"GPUTEST attention backward {what}: whole dqkv {e:.3e} (not claimed; worst at {idx}: got {got!r} want {want!r})")

    # dO = 1: dV[b, key, h, :] = sum_q P[b, h, q, key] in every channel
    ones = torch.ones_like(do64)
    (g1, _, _), (g2, _, _) = _attention_run(qkv64, ones, scale, dev, PRECS[prec])
    assert torch.equal(g1, g2), what
    dv = g1[:, 2 * D:].double().cpu().reshape(B, N, H, hd)
    e_chan = float((dv - dv.mean(-1, keepdim=True)).abs().max())
    col = dv.sum(-1).div(hd).permute(0, 2, 1)  # (B, H, N)
    col64 = p64.sum(-2)
    eager_col = _worst(ecol, col64)[0]
    tol = max(MODE_TOL[prec], 4 * eager_col) if prec == "fp32" else MODE_TOL[prec]
    e, idx, got, want = _worst(col, col64)
    total = float(col.sum()) / (B * H * N)
    print(f"GPUTEST attention backward {what} column sums of P: {e:.3e} (eager {eager_col:.3e}, bound {tol:.1e}) worst at {idx}: "
          f"got {got!r} want {want!r}; total / (B H N) - 1 = {total - 1:+.3e}; spread over channels {e_chan:.3e}")
    assert e <= tol, f"{what}: column sums of P off by {e:.3e} at {idx}: got {got!r}, want {want!r}"
    assert abs(total - 1) <= tol, f"{what}: the rows of the recomputed P sum to {total:.6f} on average"


@pytest.mark.parametrize("prec", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("hd", [64, 128])
def test_attention_backward_delta_partial_row_group(dev, hd, prec):
    """delta = rowsum(dO o O) from each operand type at B x N = 2 x 33 rows (the last workgroup has two live waves of four),
    without the optional fp32 copy of the context: against float64 on the very operand values the kernel reads."""
    lib = _lib.load()
    B, N, H = 2, 33, 3
    D, pc = H * hd, PRECS[prec]
    g = torch.Generator().manual_seed(hd + len(prec))
    ctx32 = torch.randn(B * N, D, generator=g) * (1 + 30 * torch.rand(B * N, 1, generator=g))
    do = torch.randn(B * N, D, generator=g)
    do[: N // 2] *= 1e-3
    op = to_operand(ctx32.to(dev), pc)
    seen = (from_split(op) if prec == "bf16x3" else op.float()).double().cpu()
    want = (seen * do.double()).reshape(B, N, H, hd).sum(-1).permute(0, 2, 1).reshape(B * H, N)
    dod = do.to(dev)
    outs = []
    with torch.cuda.device(dev):
        for _ in range(2):
            delta = torch.full((B * H, N), float("nan"), device=dev)
            _lib.check(lib.ocm_op_attention_backward_delta(pc, _p(op), _p(dod), _p(delta), None, B, N, H, hd, _stream()))
            outs.append(delta)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    e, idx, got, wnt = _worst(outs[0], want)
    print(f"GPUTEST attention delta hd={hd} {prec}: {e:.3e}")
    assert e <= 1e-5, f"delta {prec} hd={hd}: {e:.3e} at {idx}: got {got!r}, want {wnt!r}"  # an fp32 dot product of hd terms


# ---- Swin window attention backward ------------------------------------------------------------------------------------
def _window_probs(qkv, B, H, W, heads, ws, shift, table):
    """The softmax of _window_attention_oracle (same scores, same -100 shift mask): (windows, heads, ws^2, ws^2)."""
    C_ = heads * 32
    t = qkv.view(B, H, W, 3 * C_)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(t, ws).view(-1, ws * ws, 3, heads, 32)
    q, k = (win[:, :, i].transpose(1, 2) for i in range(2))
    bias = table[SO.relative_position_index(ws).view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1).unsqueeze(0)
    s = q @ k.transpose(2, 3) * 32 ** -0.5 + bias
    m = SO.shift_mask(H, W, ws, shift)
    if m is not None:
        nW = m.shape[0]
        s = s + m.unsqueeze(1).unsqueeze(0).expand(win.shape[0] // nW, -1, -1, -1, -1).reshape(-1, 1, ws * ws, ws * ws)
    return torch.softmax(s, -1), m


def _wattn_compare(lib, dev, qkv, dctx, table, B, H, W, ws, shift, heads, what, eager_rule):
    """Kernel against float64 autograd of the oracle; with `eager_rule` the bound is 4x the error of the same oracle run in
    float32 on the CPU, never less than WATTN_BOUND."""
    C_ = heads * 32
    q64, t64 = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    _window_attention_oracle(q64, B, H, W, heads, ws, shift, t64).backward(dctx.double())
    blocks = [float(q64.grad[:, i * C_:(i + 1) * C_].abs().max()) for i in range(3)]
    assert min(blocks) >= 1e-6 * max(blocks) and float(t64.grad.abs().max()) > 0, blocks
    bq = bt = WATTN_BOUND
    if eager_rule:
        q32, t32 = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
        _window_attention_oracle(q32, B, H, W, heads, ws, shift, t32).backward(dctx)
        eq, et = _worst(q32.grad, q64.grad)[0], _worst(t32.grad, t64.grad)[0]
        print(f"GPUTEST swin window attention backward {what}: fp32 eager CPU dqkv {eq:.3e} table {et:.3e}")
        bq, bt = max(WATTN_BOUND, 4 * eq), max(WATTN_BOUND, 4 * et)
    got, gtab = _wattn_bwd(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    again, gtab2 = _wattn_bwd(lib, qkv.to(dev), dctx.to(dev), table.to(dev), B, H, W, ws, shift, heads)
    assert torch.equal(again, got) and torch.equal(gtab2, gtab), what
    e, idx, g_, w_ = _worst(got, q64.grad)
    et, idxt, gt_, wt_ = _worst(gtab, t64.grad)
    print(f"GPUTEST swin window attention backward {what}: dqkv {e:.3e} (bound {bq:.1e}), table {et:.3e} (bound {bt:.1e})")
    assert e <= bq, f"{what}: dqkv {e:.3e} at {idx}: got {g_!r}, want {w_!r}"
    assert et <= bt, f"{what}: table {et:.3e} at {idxt}: got {gt_!r}, want {wt_!r}"


@pytest.mark.parametrize("B,H,W,heads", [(2, 14, 14, 3), (2, 14, 14, 6), (2, 28, 28, 3), (2, 28, 28, 6)])
def test_window_attention_backward_peaked(lib, dev, B, H, W, heads):
    """q, k ~ N(0, 3^2) and a table ~ N(0, 3^2): the float64 softmax's median row maximum is at least 0.8 (0.93 .. 0.95)."""
    ws, shift, C_ = 7, 3, heads * 32
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + shift + heads)
    qkv = torch.randn(B * H * W, 3 * C_, generator=g)
    qkv[:, :2 * C_] *= 3.0
    dctx = torch.randn(B * H * W, C_, generator=g)
    table = 3.0 * torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    p, _ = _window_probs(qkv.double(), B, H, W, heads, ws, shift, table.double())
    median = float(p.max(-1).values.median())
    assert median >= 0.8, f"the case went soft: median row maximum {median:.3f}"
    _wattn_compare(lib, dev, qkv, dctx, table, B, H, W, ws, shift, heads, f"peaked {H}x{W} heads{heads} (median {median:.3f})",
                   eager_rule=True)


@pytest.mark.parametrize("B,H,W,ws,shift,heads", [(3, 4, 4, 2, 1, 2), (2, 6, 6, 3, 1, 3), (2, 14, 14, 7, 3, 3)])
def test_window_attention_backward_single_unmasked_key(lib, dev, B, H, W, ws, shift, heads):
    """Table entries of +-30 under the -100 shift mask. With windows of 2 and 3 shifted by 1 the last window holds tokens that
    are alone in their region: every other key of their row carries the mask (asserted on the oracle's mask), and the kept
    key's own bias may be -30 while a masked key's is +30, so the row's scores span -130 .. 0."""
    C_ = heads * 32
    g = torch.Generator().manual_seed(ws * 100 + heads)
    qkv = torch.randn(B * H * W, 3 * C_, generator=g)
    qkv[:, :2 * C_] *= 1.5
    dctx = torch.randn(B * H * W, C_, generator=g)
    table = 30.0 * torch.sign(torch.randn((2 * ws - 1) ** 2, heads, generator=g))
    p, m = _window_probs(qkv.double(), B, H, W, heads, ws, shift, table.double())
    alone = int(((m == 0).sum(-1) == 1).sum())
    if ws < 7:
        assert alone >= 1, "no row with a single unmasked key"
    assert float(p.max()) > 0.999  # saturated rows are present
    _wattn_compare(lib, dev, qkv, dctx, table, B, H, W, ws, shift, heads, f"table +-30 ws{ws} shift{shift} ({alone} lone rows)",
                   eager_rule=True)


def test_window_attention_backward_three_table_chunks(lib, dev):
    """130 images of one window each: the table gradient's first level sums 64 windows per chunk, so 64 + 64 + 2."""
    B, H, W, ws, shift, heads = 130, 7, 7, 7, 0, 3
    C_ = heads * 32
    g = torch.Generator().manual_seed(130)
    qkv = torch.randn(B * H * W, 3 * C_, generator=g)
    qkv[:, :2 * C_] *= 1.5
    dctx = torch.randn(B * H * W, C_, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    _wattn_compare(lib, dev, qkv, dctx, table, B, H, W, ws, shift, heads, "B=130 7x7", eager_rule=False)
