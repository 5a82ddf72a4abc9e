"""The encoder-backward operators (kernels_train.hip, kernels_train_attn.hip) against float64 torch autograd, and their
bitwise determinism (every operator runs twice: torch.equal). Needs an MI355X."""
import pytest
import torch
import torch.nn.functional as F

from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.engine import _p, _stream, to_operand

pytestmark = pytest.mark.gpu
PRECS = {"bf16": _lib.OCM_PREC_BF16, "fp32": _lib.OCM_PREC_FP32, "bf16x3": _lib.OCM_PREC_BF16X3}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _rel(a, ref):
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _attention_case(B, H, N, hd, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(3, B, H, N, hd, generator=g, dtype=torch.float64)
    qkv[:2] *= 1.5
    do = torch.randn(B, N, H * hd, generator=g, dtype=torch.float64)
    do[:, : N // 2] *= 1e-3  # mixed scale
    return qkv, do


def _attention_run(qkv64, do64, scale, dev, prec=_lib.OCM_PREC_FP32):
    """Forward (lse2, ctx) with the product's kernels, then delta and the backward. Returns dqkv (B*N, 3D) and ctx."""
    lib = _lib.load()
    _, B, H, N, hd = qkv64.shape
    D = H * hd
    qkv = qkv64.float().to(dev).contiguous()
    npad = lib.ocm_n_pad_prec(prec, N)
    adt = {0: torch.bfloat16, 1: torch.float32, 2: torch.int32}[prec]
    qk32 = torch.zeros((2, B * H, npad, hd), device=dev)
    qk32[:, :, :N] = qkv[:2].reshape(2, B * H, N, hd)
    vt32 = torch.zeros((B * H, hd, npad), device=dev)
    vt32[:, :, :N] = qkv[2].reshape(B * H, N, hd).transpose(1, 2)
    q, k, vt = to_operand(qk32[0], prec), to_operand(qk32[1], prec), to_operand(vt32, prec)
    ctx = torch.empty((B * N, D), dtype=adt, device=dev)
    lse = torch.empty((B * H, N), device=dev)
    do = do64.float().to(dev).reshape(B * N, D).contiguous()
    outs = []
    with torch.cuda.device(dev):
        _lib.check(lib.ocm_op_attention_hd(prec, _p(q), _p(k), _p(vt), _p(ctx), _p(lse), B, N, H, hd, scale, _stream()))
        for _ in range(2):
            delta = torch.empty((B * H, N), device=dev)
            c32 = torch.empty((B * N, D), device=dev)
            _lib.check(lib.ocm_op_attention_backward_delta(prec, _p(ctx), _p(do), _p(delta), _p(c32), B, N, H, hd, _stream()))
            dqkv = torch.full((B * N, 3 * D), float("nan"), device=dev)
            _lib.check(lib.ocm_op_attention_backward(_p(qkv), _p(lse), _p(do), _p(delta), _p(dqkv), B, N, H, hd, scale,
                                                     _stream()))
            outs.append((dqkv, delta, c32))
    torch.cuda.synchronize()
    return outs


def _attention_ref(qkv64, do64, scale):
    _, B, H, N, hd = qkv64.shape
    qkv = qkv64.clone().requires_grad_(True)
    a = (qkv[0] @ qkv[1].transpose(-1, -2) * scale).softmax(-1)
    ctx = (a @ qkv[2]).transpose(1, 2).reshape(B, N, H * hd)
    (g,) = torch.autograd.grad(ctx, qkv, do64)
    # (3, B, H, N, hd) -> (B*N, 3*H*hd) in qkv.weight's (3, H, hd) column order
    return g.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * hd), ctx.detach()


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("N", [1, 65, 197, 785, 1601, 2305])
def test_attention_backward_matches_float64(dev, hd, N):
    B, H = (1, 3) if N >= 785 else (2, 3)  # B*H odd and even
    if N <= 65:
        B, H = 2, 2
    qkv64, do64 = _attention_case(B, H, N, hd, seed=N + hd)
    scale = hd ** -0.5
    (dqkv, delta, c32), (dqkv2, delta2, c322) = _attention_run(qkv64, do64, scale, dev)
    ref, ctx64 = _attention_ref(qkv64, do64, scale)
    assert torch.equal(dqkv, dqkv2) and torch.equal(delta, delta2) and torch.equal(c32, c322)
    assert not torch.isnan(dqkv).any()
    assert _rel(c32, ctx64.reshape(B * N, -1)) <= 1e-5
    D = H * hd
    for which in range(3):
        blk, rblk = dqkv[:, which * D:(which + 1) * D], ref[:, which * D:(which + 1) * D]
        # with one token dQ and dK are exactly zero (P = 1, dS = dO.v - dO.o = 0): measure them against the whole gradient
        den = float(rblk.abs().max()) if N > 1 else float(ref.abs().max())
        assert float((blk.double().cpu() - rblk).abs().max()) / den <= 1e-4, which


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_attention_backward_from_each_precisions_forward(dev, prec):
    """lse2 and the context come from the forward in the engine's precision; delta reads that context's operand type."""
    B, H, N, hd = 2, 3, 197, 128
    qkv64, do64 = _attention_case(B, H, N, hd, seed=3)
    (dqkv, _, _), (dqkv2, _, _) = _attention_run(qkv64, do64, hd ** -0.5, dev, PRECS[prec])
    ref, _ = _attention_ref(qkv64, do64, hd ** -0.5)
    assert torch.equal(dqkv, dqkv2)
    assert _rel(dqkv, ref) <= (5e-2 if prec == "bf16" else 1e-3)


@pytest.mark.parametrize("offset", [0.0, 30.0])
def test_layernorm_backward_matches_float64(dev, offset):
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    rows, dim, eps = 1000, 384, 1e-6
    x64 = torch.randn(rows, dim, generator=g, dtype=torch.float64) + offset * torch.randn(rows, 1, generator=g,
                                                                                         dtype=torch.float64).abs()
    w64 = 1 + 0.1 * torch.randn(dim, generator=g, dtype=torch.float64)
    dy64 = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    res64 = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    xr, wr = x64.clone().requires_grad_(True), w64.clone().requires_grad_(True)
    br = torch.zeros(dim, dtype=torch.float64, requires_grad=True)
    dx_ref, dw_ref, db_ref = torch.autograd.grad(F.layer_norm(xr, (dim,), wr, br, eps), (xr, wr, br), dy64)
    dx_ref = dx_ref + res64
    x, w, dy, res = (t.float().to(dev) for t in (x64, w64, dy64, res64))
    outs = []
    for _ in range(2):
        dx, dw, db = torch.empty_like(x), torch.empty(dim, device=dev), torch.empty(dim, device=dev)
        nbytes = lib.ocm_layernorm_backward_workspace_bytes(rows, dim)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.ocm_op_layernorm_backward(_p(dy), _p(x), _p(w), _p(res), _p(dx), _p(dw), _p(db), rows, dim, eps, _p(ws),
                                                 nbytes, _stream()))
        outs.append((dx, dw, db))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    dx, dw, db = outs[0]
    assert _rel(dx, dx_ref) <= 1e-5 and _rel(dw, dw_ref) <= 1e-5 and _rel(db, db_ref) <= 1e-5


def test_gelu_and_backward_match_float64(dev):
    lib = _lib.load()
    g = torch.Generator().manual_seed(2)
    h64 = 3 * torch.randn(64, 1536, generator=g, dtype=torch.float64)
    dg64 = torch.randn(64, 1536, generator=g, dtype=torch.float64)
    hr = h64.clone().requires_grad_(True)
    y = F.gelu(hr)
    (dh_ref,) = torch.autograd.grad(y, hr, dg64)
    h, dg = h64.float().to(dev), dg64.float().to(dev)
    n = h.numel()
    for name, prec in PRECS.items():
        adt = {0: torch.bfloat16, 1: torch.float32, 2: torch.int32}[prec]
        out, out32 = torch.empty(h.shape, dtype=adt, device=dev), torch.empty_like(h)
        _lib.check(lib.ocm_op_gelu(prec, _p(h), _p(out), _p(out32), n, _stream()))
        assert _rel(out32, y.detach()) <= 1e-6, name
        ref_op = to_operand(out32, prec)
        assert torch.equal(out, ref_op), name
    res = []
    for _ in range(2):
        dh, g32 = torch.empty_like(h), torch.empty_like(h)
        _lib.check(lib.ocm_op_gelu_backward(_p(dg), _p(h), _p(dh), _p(g32), n, _stream()))
        res.append((dh, g32))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert _rel(res[0][0], dh_ref) <= 1e-5
    assert _rel(res[0][1], y.detach()) <= 1e-6


def test_patch_reductions_match_float64(dev):
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    B, hp, D, p, Cc = 3, 6, 128, 8, 3
    N = hp * hp + 1
    dt64 = torch.randn(B, N, D, generator=g, dtype=torch.float64)
    w64 = (torch.rand(B, N - 1, generator=g) < 0.6).double()
    img = torch.rand(B, Cc, hp * p, hp * p, generator=g)
    dt, w = dt64.float().to(dev), w64.float().to(dev)
    res = []
    for _ in range(2):
        dpatch, dmask, dpos = torch.empty((B * (N - 1), D), device=dev), torch.empty(D, device=dev), torch.empty((N, D), device=dev)
        nbytes = lib.ocm_patch_embed_backward_workspace_bytes(B, N, D)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.ocm_op_patch_embed_backward(_p(dt), _p(w), _p(dpatch), _p(dmask), _p(dpos), B, N, D, _p(ws), nbytes,
                                                   _stream()))
        cols = torch.empty((B * hp * hp, Cc * p * p), device=dev)
        imgd = img.to(dev)
        _lib.check(lib.ocm_op_patch_unfold(_p(imgd), _p(cols), B, Cc, hp * p, hp * p, p, _stream()))
        res.append((dpatch, dmask, dpos, cols))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)
    dpatch, dmask, dpos, cols = res[0]
    wv = w64.unsqueeze(-1)
    assert _rel(dpatch, ((1 - wv) * dt64[:, 1:]).reshape(-1, D)) <= 1e-7
    assert _rel(dmask, (wv * dt64[:, 1:]).sum((0, 1))) <= 1e-6
    assert _rel(dpos, dt64.sum(0)) <= 1e-6
    ref_cols = F.unfold(img, p, stride=p).transpose(1, 2).reshape(-1, Cc * p * p)
    assert torch.equal(cols.cpu(), ref_cols)
