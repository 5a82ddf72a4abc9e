"""The Dice-loss kernels and the decoder's data-gradient path (conv1's transposed convolution as im2col3x3 + linear, the 1x1
head's dlin W) on poisoned workspaces and guard-banded outputs (tests/memcheck.py): no store outside an output, no read of a
workspace byte the call did not write, every output byte written. Counts and shapes include ones that end mid-vector and
mid-tile, and pointers that are not 16-byte aligned (the scalar variants). Needs an MI355X."""
import pytest
import torch

from tests.memcheck import PATTERNS, Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu

_ACT = {_lib.OCM_PREC_BF16: torch.bfloat16, _lib.OCM_PREC_FP32: torch.float32, _lib.OCM_PREC_BF16X3: torch.int32}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return _lib.load()


def _run(lib, what, outs, ws_bytes, call, shift=0):
    """outs: name -> (nbytes, dtype). Runs `call(ptrs, ws_ptr)` with outputs / workspace under two fills; returns the outputs.
    shift: the outputs start that many bytes into their payloads (a pointer off the 16-byte grid); the bytes in front of them
    must keep the fill."""
    results = []
    for out_fill, ws_fill in (("nan", "big"), ("zero", "unit")):
        g = {k: Guarded(nb + shift, "cuda", out_fill) for k, (nb, _) in outs.items()}
        ws = Guarded(ws_bytes, "cuda", ws_fill) if ws_bytes is not None else None
        torch.cuda.synchronize()
        rc = call({k: v.ptr + shift for k, v in g.items()}, ws.ptr if ws is not None else None)
        assert rc == 0, f"{what}: {lib.ocm_last_error().decode()}"
        torch.cuda.synchronize()
        for k, v in g.items():
            assert v.check() is None, f"{what}: {k}: {v.check()}"
            if shift:
                front = v.payload()[:shift].view(torch.int32).cpu()  # shift is a multiple of 4
                assert bool((front == PATTERNS[out_fill] - ((PATTERNS[out_fill] >> 31) << 32)).all()), \
                    f"{what}: {k}: bytes in front of the output changed"
        if ws is not None:
            assert ws.check() is None, f"{what}: workspace: {ws.check()}"
        results.append({k: v.payload()[shift:].clone().view(outs[k][1]) for k, v in g.items()})
    for k in outs:
        assert_same_bits(results[0][k], results[1][k], f"{what}: {k} under two output / workspace fills")
    return results[0]


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("count", [1, 3, 4, 255, 4097, 3 * 4096 + 5, 3 * 384 * 384, 1024 * 4096 + 6])
def test_dice_kernels_guarded(lib, count, shift):
    g = torch.Generator().manual_seed(count)
    pad = shift // 4
    x = (torch.randn(count + pad, generator=g) * 5).cuda()[pad:]  # shift 4: inputs off the 16-byte grid too
    t = (torch.rand(count + pad, generator=g) < 0.5).float().cuda()[pad:]
    gl = torch.ones(1).cuda()
    nbytes = lib.ocm_dice_loss_workspace_bytes(count)
    assert 12 <= nbytes <= 12 * 1024
    fwd = _run(lib, f"dice_loss count={count}", {"loss": (4, torch.float32), "sums": (12, torch.float32)}, nbytes,
               lambda o, ws: lib.ocm_op_dice_loss(x.data_ptr(), t.data_ptr(), o["loss"], o["sums"], count, 1.0, ws, nbytes, None),
               shift=shift)
    assert torch.isfinite(fwd["loss"]).all() and torch.isfinite(fwd["sums"]).all()
    p = torch.sigmoid(x.double())
    want = torch.stack([(p * t).sum(), p.sum(), t.double().sum()])
    assert float((fwd["sums"].double() - want).abs().max()) <= 1e-5 * float(want.abs().max().clamp_min(1.0))
    sums = fwd["sums"].clone()
    bwd = _run(lib, f"dice_loss_backward count={count}", {"dx": (count * 4, torch.float32)}, None,
               lambda o, _: lib.ocm_op_dice_loss_backward(x.data_ptr(), t.data_ptr(), sums.data_ptr(), gl.data_ptr(), o["dx"],
                                                          count, 1.0, None), shift=shift)
    assert torch.isfinite(bwd["dx"]).all()
    # a workspace one byte short is refused, not overrun
    ws = Guarded(nbytes, "cuda", "nan")
    out = torch.empty(4).cuda()
    assert lib.ocm_op_dice_loss(x.data_ptr(), t.data_ptr(), out.data_ptr(), out[1:].data_ptr(), count, 1.0, ws.ptr, nbytes - 1,
                                None) == _lib.OCM_ENOMEM


@pytest.mark.parametrize("precision", ["bf16x3", "fp32", "bf16"])
@pytest.mark.parametrize("B,hp,D,s", [(1, 3, 128, 8), (2, 5, 384, 8), (3, 7, 128, 4), (1, 48, 384, 8)])
def test_decoder_data_gradient_guarded(lib, precision, B, hp, D, s):
    """_DecoderTrain's patch gradient as the C ABI runs it: im2col3x3 of dy1 (M x 4 s^2) and the GEMM with the flipped conv1 kernel
    (K = 9 * 4 s^2, N = D), and the 1x1 head's dlin W (K = s^2, N = D). M = B hp^2 ends mid-tile (9, 50, 147) or is the 384^2 grid."""
    pc = _lib.PRECISIONS[precision]
    mid, Mr = 4 * s * s, B * hp * hp
    g = torch.Generator().manual_seed(Mr + D)
    dy1 = torch.randn(Mr, mid, generator=g).cuda()
    w1 = (torch.randn(mid, D, 3, 3, generator=g) * 0.02).cuda()
    w1f = to_operand(M.flip_conv3x3(w1).contiguous(), pc)  # (D, 9 mid)
    zero = torch.zeros(D).cuda()
    cols = _run(lib, f"im2col3x3 of dy1 [{precision}]", {"d1": (Mr * 9 * mid * torch.empty((), dtype=_ACT[pc]).element_size(),
                                                              _ACT[pc])}, None,
                lambda o, _: lib.ocm_op_im2col3x3(pc, dy1.data_ptr(), o["d1"], B, hp, hp, mid, 0, None))
    d1 = cols["d1"].reshape(Mr, 9 * mid).clone()
    got = _run(lib, f"conv1 data gradient [{precision}]", {"dx": (Mr * D * 4, torch.float32)}, None,
               lambda o, _: lib.ocm_op_linear(pc, d1.data_ptr(), w1f.data_ptr(), zero.data_ptr(), None, o["dx"], Mr, D, 9 * mid,
                                              _lib.OCM_EPI_BIAS_F32, None))
    want = torch.nn.grad.conv2d_input((B, D, hp, hp), w1.double().cpu(),
                                      dy1.double().cpu().reshape(B, hp, hp, mid).permute(0, 3, 1, 2), padding=1)
    want = want.permute(0, 2, 3, 1).reshape(Mr, D)
    tol = {"fp32": 2e-5, "bf16x3": 2e-4, "bf16": 3e-2}[precision]
    assert float((got["dx"].reshape(Mr, D).double().cpu() - want).abs().max()) <= tol * float(want.abs().max())
    # the 1x1 head: dlin (M x s^2) times W (s^2 x D)
    O = s * s
    dlin = torch.randn(Mr, O, generator=g).cuda()
    w = (torch.randn(O, D, generator=g) * 0.05).cuda()
    if O % 64:
        return  # the operands' K granularity (64 in single bf16): strides of 8 and 16, as the reference's decoders have
    wt, a = to_operand(w.t().contiguous(), pc), to_operand(dlin, pc)
    got = _run(lib, f"1x1 head data gradient [{precision}]", {"dx": (Mr * D * 4, torch.float32)}, None,
               lambda o, _: lib.ocm_op_linear(pc, a.data_ptr(), wt.data_ptr(), zero.data_ptr(), None, o["dx"], Mr, D, O,
                                              _lib.OCM_EPI_BIAS_F32, None))
    want = dlin.double().cpu() @ w.double().cpu()
    assert float((got["dx"].reshape(Mr, D).double().cpu() - want).abs().max()) <= tol * float(want.abs().max())
