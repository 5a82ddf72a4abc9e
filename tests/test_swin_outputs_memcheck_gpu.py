"""The Swin backbone outputs on poisoned workspaces and guard-banded outputs (tests/memcheck.py): ocm_op_swin_window_probs,
ocm_op_swin_tokens_to_nchw and ocm_swin_forward_ex store nothing outside the buffers asked for, read no workspace byte the call
did not write, and write every byte of every output. Needs an MI355X."""
import ctypes as C

import pytest
import torch

from tests import swin_outputs_ref as R
from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import swin as SW
from vit_ocm_wmsegmentation_amd.engine import to_operand

pytestmark = pytest.mark.gpu

FILLS = (("nan", "big"), ("zero", "unit"))  # (outputs, workspace / scratch)


def _run(lib, what, outs, ws_bytes, call):
    """outs: name -> (shape, fp32). Runs `call(ptrs, ws_ptr)` with outputs / workspace under two fills; the outputs must hold the
    same bits under both (so no output byte is left unwritten and no unwritten workspace byte is read) and no guard may change."""
    results = []
    for out_fill, ws_fill in FILLS:
        g = {k: Guarded(4 * int(torch.Size(shape).numel()), "cuda", out_fill) for k, shape in outs.items()}
        ws = Guarded(ws_bytes, "cuda", ws_fill) if ws_bytes is not None else None
        torch.cuda.synchronize()
        rc = call({k: v.ptr for k, v in g.items()}, ws.ptr if ws is not None else None)
        assert rc == 0, f"{what}: {lib.ocm_last_error().decode()}"
        torch.cuda.synchronize()
        for k, v in g.items():
            assert v.check() is None, f"{what}: {k}: {v.check()}"
        if ws is not None:
            assert ws.check() is None, f"{what}: workspace: {ws.check()}"
        results.append({k: v.payload(torch.float32, outs[k]).clone() for k, v in g.items()})
    for k in outs:
        assert_same_bits(results[0][k], results[1][k], f"{what}: {k} under two output / workspace fills")
        assert torch.isfinite(results[0][k]).all(), f"{what}: {k}"
    return results[0]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("B,H,W,ws,shift,heads", [(3, 14, 14, 7, 3, 3), (1, 7, 7, 7, 0, 1), (2, 8, 12, 4, 2, 2), (5, 3, 3, 3, 1, 1)])
def test_window_probs_guarded(lib, precision, B, H, W, ws, shift, heads):
    """Odd windows give blocks of an odd number of floats (ws^4): every second block starts off a 16-byte boundary."""
    pc = _lib.PRECISIONS[precision]
    g = torch.Generator().manual_seed(B + H)
    T, Cn = B * H * W, 32 * heads
    op = to_operand(torch.randn(T, 3 * Cn, generator=g).cuda(), pc)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).cuda()
    shape = (B * (H // ws) * (W // ws), heads, ws * ws, ws * ws)
    out = _run(lib, f"window_probs {precision}", {"probs": shape}, 4 * heads * (4096 + ws ** 4),
               lambda o, sc: lib.ocm_op_swin_window_probs(pc, op.data_ptr(), 3 * Cn, o["probs"], table.data_ptr(), sc, B, H, W, ws,
                                                          shift, heads, None))
    assert float((out["probs"].double().sum(-1) - 1).abs().max()) <= 1e-5


@pytest.mark.parametrize("B,L,Cn", [(2, 25, 64), (3, 100, 32), (1, 33, 96), (2, 49, 40)])
def test_tokens_to_nchw_guarded(lib, B, L, Cn):
    x = torch.randn(B, L, Cn).cuda()
    out = _run(lib, "tokens_to_nchw", {"out": (B, Cn, L)}, None,
               lambda o, _: lib.ocm_op_swin_tokens_to_nchw(x.data_ptr(), o["out"], B, L, Cn, None))
    assert torch.equal(out["out"], x.transpose(1, 2).contiguous())


def _engine(name, precision, backbone=False):
    cfg, sd, _ = R.case(name)
    hf = SW.SwinConfig(image_size=cfg["image_size"], embed_dim=cfg["embed_dim"], depths=cfg["depths"], num_heads=cfg["num_heads"],
                       window_size=cfg["window_size"], num_labels=cfg["num_labels"])
    model = SW.SwinForImageClassification(hf)
    model.load_state_dict(sd)
    if backbone:
        alone = SW.SwinModel(hf)
        alone.load_state_dict(model.swin.state_dict())
        model = alone
    model = model.cuda().eval().set_precision(precision)
    return cfg, model, model._get_engine(torch.device("cuda:0"))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name,layers", [("g40w4", (0, 1, 2, 3)), ("g40w4", (3,)), ("g56w7c96", (0, 1, 2, 3)), ("g56w7c96", (1, 2)),
                                         ("g56w7c96", ())])
def test_forward_ex_guarded(lib, name, layers, precision):
    """Every output in its own guarded allocation, the workspace poisoned: the padded geometry (g40w4) and the one whose
    split-bf16 layers leave their fused kernels for a requested map (g56w7c96). With only some attention pointers non-null the
    other layers' buffers are not even allocated: nothing outside the requested buffers is written."""
    B = 3
    cfg, model, eng = _engine(name, precision)
    x = R.case(name, batch=B)[2].cuda()
    n_hidden, n_layers = len(cfg["depths"]) + 1, sum(cfg["depths"])

    def shape(kind, i):
        dims = (C.c_int64 * 4)()
        _lib.check(lib.ocm_swin_output_shape(C.byref(eng["cfg"]), B, kind, i, dims))
        return tuple(dims)

    last = shape(_lib.OCM_SWIN_OUT_HIDDEN, n_hidden - 1)[:3]
    outs = {"logits": (B, cfg["num_labels"]), "pooled": (B, last[2]), "last": last}
    outs.update({f"hidden{i}": shape(_lib.OCM_SWIN_OUT_HIDDEN, i)[:3] for i in range(n_hidden)})
    outs.update({f"reshaped{i}": shape(_lib.OCM_SWIN_OUT_RESHAPED, i) for i in range(n_hidden)})
    outs.update({f"attn{i}": shape(_lib.OCM_SWIN_OUT_ATTENTION, i) for i in layers})
    nbytes = lib.ocm_swin_workspace_bytes(eng["h"], B)

    def call(p, ws):
        o = _lib.OcmSwinOutputs()
        for i in range(n_hidden):
            o.hidden[i], o.reshaped[i] = p[f"hidden{i}"], p[f"reshaped{i}"]
        ptrs = (C.c_void_p * n_layers)()
        for i in layers:
            ptrs[i] = p[f"attn{i}"]
        if layers:
            o.attentions = C.cast(ptrs, C.POINTER(C.c_void_p))
        return lib.ocm_swin_forward_ex(eng["h"], x.data_ptr(), B, p["logits"], p["pooled"], p["last"], C.byref(o), ws, nbytes, None)

    got = _run(lib, f"forward_ex {name} {precision} layers {layers}", outs, nbytes, call)
    want = model(pixel_values=x, output_hidden_states=True, output_attentions=list(layers))
    assert_same_bits(got["logits"], want.logits, "logits")
    assert_same_bits(got["last"], want.last_hidden_state, "last_hidden_state")
    for i in range(n_hidden):
        assert_same_bits(got[f"hidden{i}"], want.hidden_states[i], f"hidden_states[{i}]")
        assert_same_bits(got[f"reshaped{i}"], want.reshaped_hidden_states[i], f"reshaped_hidden_states[{i}]")
    for i in layers:
        assert_same_bits(got[f"attn{i}"], want.attentions[i], f"attentions[{i}]")
    # a null `outputs` is ocm_swin_forward, bit for bit
    plain = _run(lib, f"forward_ex null outputs {name} {precision}", {k: outs[k] for k in ("logits", "pooled", "last")}, nbytes,
                 lambda p, ws: lib.ocm_swin_forward_ex(eng["h"], x.data_ptr(), B, p["logits"], p["pooled"], p["last"], None, ws,
                                                       nbytes, None))
    old = _run(lib, f"forward {name} {precision}", {k: outs[k] for k in ("logits", "pooled", "last")}, nbytes,
               lambda p, ws: lib.ocm_swin_forward(eng["h"], x.data_ptr(), B, p["logits"], p["pooled"], p["last"], ws, nbytes, None))
    for k in plain:
        assert_same_bits(plain[k], old[k], f"forward_ex(null) vs forward: {k}")


def test_backbone_engine_needs_no_classifier(lib):
    """OCM_SWIN_CFG_BACKBONE: no classifier.* parameter is waited for, logits may be null and nothing is written for them."""
    B = 2
    cfg, model, eng = _engine("g32w4", "fp32", backbone=True)
    assert eng["labels"] == 0 and lib.ocm_swin_params_ready(eng["h"]) == 0
    assert lib.ocm_swin_set_param(eng["h"], b"classifier.weight", 256, 5 * 64, None) == _lib.OCM_ENAME
    x = R.case("g32w4", batch=B)[2].cuda()
    nbytes = lib.ocm_swin_workspace_bytes(eng["h"], B)
    got = _run(lib, "backbone forward", {"pooled": (B, 64), "last": (B, 16, 64)}, nbytes,
               lambda p, ws: lib.ocm_swin_forward_ex(eng["h"], x.data_ptr(), B, None, p["pooled"], p["last"], None, ws, nbytes, None))
    want = model(x)
    assert_same_bits(got["pooled"], want.pooler_output, "pooler_output")
    assert_same_bits(got["last"], want.last_hidden_state, "last_hidden_state")
    _, cls, ceng = _engine("g32w4", "fp32")
    assert lib.ocm_swin_forward_ex(ceng["h"], x.data_ptr(), B, None, None, None, None, 256, nbytes, None) == _lib.OCM_EINVAL
