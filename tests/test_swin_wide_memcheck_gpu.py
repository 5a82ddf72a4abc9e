"""The wide-window Swin kernels (windows of 8 to 12) on poisoned scratch / workspaces and guard-banded outputs
(tests/memcheck.py): ocm_op_swin_window_attention, ocm_op_swin_window_probs and a forward with every map store nothing outside
the buffers asked for, read no scratch or workspace byte the call did not write, and write every byte of every output."""
import ctypes as C

import pytest
import torch

from tests import swin_wide_ref as WR
from tests.memcheck import Guarded, assert_same_bits
from tests.test_swin_outputs_memcheck_gpu import _run
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import swin as SW
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu

ESZ = {"fp32": 4, "bf16x3": 4, "bf16": 2}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("B,H,W,ws,shift,heads", [(3, 18, 18, 9, 4, 3), (1, 9, 9, 9, 0, 1), (2, 24, 24, 12, 6, 2), (1, 12, 12, 12, 0, 4)])
def test_wide_probs_guarded(lib, precision, B, H, W, ws, shift, heads):
    """ws 9: blocks of 81^2 floats and query tiles of 32 * 81 floats start off 16-byte boundaries; the scratch is exactly
    ocm_swin_window_scratch_floats."""
    pc = _lib.PRECISIONS[precision]
    g = torch.Generator().manual_seed(B + H)
    T, Cn = B * H * W, 32 * heads
    op = to_operand(torch.randn(T, 3 * Cn, generator=g).cuda(), pc)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).cuda()
    shape = (B * (H // ws) * (W // ws), heads, ws * ws, ws * ws)
    out = _run(lib, f"wide window_probs {precision}", {"probs": shape}, 4 * lib.ocm_swin_window_scratch_floats(ws, heads),
               lambda o, sc: lib.ocm_op_swin_window_probs(pc, op.data_ptr(), 3 * Cn, o["probs"], table.data_ptr(), sc, B, H, W, ws,
                                                          shift, heads, None))
    assert float((out["probs"].double().sum(-1) - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("B,H,W,ws,shift,heads", [(2, 18, 18, 9, 4, 3), (1, 24, 24, 12, 6, 2), (1, 12, 12, 12, 0, 1)])
def test_wide_attention_guarded(lib, precision, B, H, W, ws, shift, heads):
    """The context in a guarded allocation of exactly tokens x 32 * heads elements: every byte written, none beyond."""
    pc = _lib.PRECISIONS[precision]
    g = torch.Generator().manual_seed(B + H + 1)
    T, Cn = B * H * W, 32 * heads
    op = to_operand(torch.randn(T, 3 * Cn, generator=g).cuda(), pc)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).cuda()
    results = []
    for out_fill, sc_fill in (("nan", "big"), ("zero", "unit")):
        ctx = Guarded(T * Cn * ESZ[precision], "cuda", out_fill)
        sc = Guarded(4 * lib.ocm_swin_window_scratch_floats(ws, heads), "cuda", sc_fill)
        torch.cuda.synchronize()
        rc = lib.ocm_op_swin_window_attention(pc, op.data_ptr(), 3 * Cn, ctx.ptr, Cn, table.data_ptr(), sc.ptr, B, H, W, ws, shift,
                                              heads, None)
        assert rc == 0, lib.ocm_last_error().decode()
        torch.cuda.synchronize()
        assert ctx.check() is None, ctx.check()
        assert sc.check() is None, sc.check()
        results.append(ctx.payload(torch.int32 if ESZ[precision] == 4 else torch.int16).clone())
    assert_same_bits(results[0], results[1], f"wide window_attention {precision} under two output / scratch fills")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_wide_forward_ex_guarded(lib, precision):
    """The 96 / window 12 geometry with every hidden state and every map, each output in its own guarded allocation, the
    workspace poisoned."""
    name, B = "w96", 2
    cfg, sd, x = WR.case(name, batch=B)
    hf = SW.SwinConfig(image_size=cfg["image_size"], embed_dim=cfg["embed_dim"], depths=cfg["depths"], num_heads=cfg["num_heads"],
                       window_size=cfg["window_size"], num_labels=cfg["num_labels"])
    model = SW.SwinForImageClassification(hf)
    model.load_state_dict(sd)
    model = model.cuda().eval().set_precision(precision)
    eng = model._get_engine(torch.device("cuda:0"))
    x = x.cuda()
    n_hidden, n_layers = len(cfg["depths"]) + 1, sum(cfg["depths"])

    def shape(kind, i):
        dims = (C.c_int64 * 4)()
        _lib.check(lib.ocm_swin_output_shape(C.byref(eng["cfg"]), B, kind, i, dims))
        return tuple(dims)

    last = shape(_lib.OCM_SWIN_OUT_HIDDEN, n_hidden - 1)[:3]
    outs = {"logits": (B, cfg["num_labels"]), "pooled": (B, last[2]), "last": last}
    outs.update({f"hidden{i}": shape(_lib.OCM_SWIN_OUT_HIDDEN, i)[:3] for i in range(n_hidden)})
    outs.update({f"reshaped{i}": shape(_lib.OCM_SWIN_OUT_RESHAPED, i) for i in range(n_hidden)})
    outs.update({f"attn{i}": shape(_lib.OCM_SWIN_OUT_ATTENTION, i) for i in range(n_layers)})
    nbytes = lib.ocm_swin_workspace_bytes(eng["h"], B)

    def call(p, ws):
        o = _lib.OcmSwinOutputs()
        for i in range(n_hidden):
            o.hidden[i], o.reshaped[i] = p[f"hidden{i}"], p[f"reshaped{i}"]
        ptrs = (C.c_void_p * n_layers)()
        for i in range(n_layers):
            ptrs[i] = p[f"attn{i}"]
        o.attentions = C.cast(ptrs, C.POINTER(C.c_void_p))
        return lib.ocm_swin_forward_ex(eng["h"], x.data_ptr(), B, p["logits"], p["pooled"], p["last"], C.byref(o), ws, nbytes, None)

    got = _run(lib, f"wide forward_ex {precision}", outs, nbytes, call)
    want = model(pixel_values=x, output_hidden_states=True, output_attentions=True)
    assert_same_bits(got["logits"], want.logits, "logits")
    assert_same_bits(got["last"], want.last_hidden_state, "last_hidden_state")
    for i in range(n_hidden):
        assert_same_bits(got[f"hidden{i}"], want.hidden_states[i], f"hidden_states[{i}]")
    for i in range(n_layers):
        assert_same_bits(got[f"attn{i}"], want.attentions[i], f"attentions[{i}]")
