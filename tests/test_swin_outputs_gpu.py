"""The Swin backbone outputs on the HIP path against the float64 twin (tests/swin_outputs_ref.py, pinned on live transformers by
tests/test_swin_outputs_host.py): ocm_op_swin_window_probs, and hidden_states / reshaped_hidden_states / attentions of
SwinForImageClassification, SwinModel and the `.swin` view (ocm_swin_forward_ex). Same weights and seeds as the host file,
whose conditioning test holds that a wrong bias bin, head order or shift mask moves a probability by >= 0.05.

Bounds. hidden_states[-1] takes the bound tests/test_swin_geometry_gpu.py applies to the last hidden state (max |error|, per
precision). For the earlier hidden states and the probabilities the project had no number: the bounds below are 3 x the worst
error measured on MI355X over this file's cases (the margin test_swin_geometry_gpu.py shows between measured and asserted):

  measured worst max |GPU - float64 twin|        fp32        split-bf16   bf16 (sanity only)
    window_probs operator (inputs as rounded)   4.7e-7      5.9e-6       3.0e-7
    model probabilities                         2.9e-7      4.3e-6       1.5e-3
    model hidden states before the last         1.2e-6      7.7e-6       4.4e-3

(The operator's reference is computed from the values the element format holds: its fp32 and bf16 columns are fp32 rounding
(bf16 products are exact in the fp32 accumulator), the split-bf16 column is the lo x lo term the three-MFMA product drops,
2^-16 of each product, on standard-normal q and k. At model level single bf16 rounds every GEMM operand to 8 bits and its rows
are a sanity check, as in test_swin_geometry_gpu.py.
Measured on the same cases: row sums within 5.4e-7 of 1; hidden_states[-1] fp32 1.4e-6, split-bf16 8.6e-6, bf16 5.2e-3; with
all maps requested logits / pooler_output / last_hidden_state fp32 6.2e-8 / 3.6e-7 / 3.3e-6, split-bf16 1.2e-6 / 8.2e-6 / 2.3e-5.)

A probability error above 1e-3 in fp32 or split-bf16 would be a bug whatever was measured (the project's attention-map bar);
the asserted bounds are far below it.
"""
import pytest
import torch

from tests import swin_outputs_ref as R
from tests.test_swin_geometry_gpu import BOUNDS as GEOMETRY_BOUNDS
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import swin as SW
from vit_ocm_wmsegmentation_amd.engine import from_split, to_operand

pytestmark = pytest.mark.gpu

# 3 x the measured worst errors of the docstring table
OP_BOUND = {"fp32": 1.4e-6, "bf16x3": 1.8e-5, "bf16": 9e-7}
PROB_BOUND = {"fp32": 8.7e-7, "bf16x3": 1.3e-5, "bf16": 4.6e-3}
HIDDEN_BOUND = {"fp32": 3.5e-6, "bf16x3": 2.3e-5, "bf16": 1.3e-2}
ATTENTION_MAP_BAR = 1e-3

MODEL_GEOMETRIES = ("g32w4", "g40w4", "g56w7c96")
_TWIN = {}


def twin(name, batch):
    if (name, batch) not in _TWIN:
        cfg, sd, x = R.case(name, torch.float64, batch)
        _TWIN[name, batch] = R.backbone_outputs(sd, cfg, x)
    return _TWIN[name, batch]


def maxerr(got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all()
    return float((got - want).abs().max())


# ---- the operator ----------------------------------------------------------------------------------------------------------
def _probs_case(lib, dev, precision, B, H, W, ws, shift, heads, seed):
    """-> (probs from the operator, float64 reference on the values the element format holds)."""
    pc = _lib.PRECISIONS[precision]
    g = torch.Generator().manual_seed(seed)
    T, Cn = B * H * W, 32 * heads
    qkv = torch.randn(T, 3 * Cn, generator=g).to(dev)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g).to(dev)
    op = to_operand(qkv, pc)
    held = qkv if precision == "fp32" else from_split(op) if precision == "bf16x3" else op.float()
    nW = (H // ws) * (W // ws)
    out = torch.full((B * nW, heads, ws * ws, ws * ws), float("nan"), device=dev)
    scratch = torch.empty(heads * (4096 + ws ** 4), device=dev)
    _lib.check(lib.ocm_op_swin_window_probs(pc, op.data_ptr(), 3 * Cn, out.data_ptr(), table.data_ptr(), scratch.data_ptr(),
                                            B, H, W, ws, shift, heads, None))
    want = R.window_probs(held.cpu().double(), B, H, W, heads, ws, shift, table.cpu().double())
    return out, want


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("ws", [2, 3, 4, 5, 6, 7])
def test_window_probs_operator(lib, dev, ws, precision):
    """Windows 2 .. 7, shift 0 and ws / 2, 1 .. 3 heads, grids of 1 x 1, 2 x 2 and 3 x 3 windows (only 3 x 3 has an unmasked
    interior window under a shift), B = 1 and 3, and for ws 4 a non-square 8 x 12 grid."""
    worst, worst_sum = 0.0, 0.0
    grids = [(n * ws, n * ws) for n in (1, 2, 3)] + ([(8, 12)] if ws == 4 else [])
    seed = 100 * ws
    for shift in (0, ws // 2):
        for heads in (1, 2, 3):
            for H, W in grids:
                for B in (1, 3):
                    seed += 1
                    got, want = _probs_case(lib, dev, precision, B, H, W, ws, shift, heads, seed)
                    worst = max(worst, maxerr(got, want))
                    worst_sum = max(worst_sum, float((got.double().sum(-1) - 1).abs().max()))
    again, _ = _probs_case(lib, dev, precision, 3, grids[-1][0], grids[-1][1], ws, ws // 2, 3, seed)
    assert torch.equal(again, got), "a rerun gives other bits"
    print(f"GPUTEST swin outputs window_probs ws{ws} {precision}: probs {worst:.2e}, row sums {worst_sum:.2e}")
    assert worst_sum <= 1e-5
    assert worst <= OP_BOUND[precision], worst
    assert worst <= ATTENTION_MAP_BAR


# ---- the model -------------------------------------------------------------------------------------------------------------
def _models(name, precision, dev):
    cfg, sd, _ = R.case(name)
    hf = SW.SwinConfig(image_size=cfg["image_size"], num_channels=cfg["num_channels"], embed_dim=cfg["embed_dim"],
                       depths=cfg["depths"], num_heads=cfg["num_heads"], window_size=cfg["window_size"],
                       mlp_ratio=cfg["mlp_ratio"], layer_norm_eps=cfg["layer_norm_eps"], num_labels=cfg["num_labels"])
    model = SW.SwinForImageClassification(hf)
    msg = model.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    return cfg, hf, model.to(dev).eval().set_precision(precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("batch", [2, 3])
@pytest.mark.parametrize("name", MODEL_GEOMETRIES)
def test_model_outputs_vs_twin(dev, name, batch, precision):
    cfg, hf, model = _models(name, precision, dev)
    x = R.case(name, batch=batch)[2].to(dev)
    want = twin(name, batch)
    n_layers, n_hidden = sum(cfg["depths"]), len(cfg["depths"]) + 1

    plain = model(pixel_values=x, output_hidden_states=False)
    assert plain.hidden_states is None and plain.reshaped_hidden_states is None and plain.attentions is None
    assert plain.last_hidden_state is None

    hid = model(pixel_values=x, output_hidden_states=True)
    assert len(hid.hidden_states) == len(hid.reshaped_hidden_states) == n_hidden and hid.attentions is None
    e_h = [maxerr(t, w) for t, w in zip(hid.hidden_states, want["hidden_states"])]
    for h, r, w in zip(hid.hidden_states, hid.reshaped_hidden_states, want["reshaped_hidden_states"]):
        assert tuple(r.shape) == tuple(w.shape)
        assert torch.equal(r, h.transpose(1, 2).reshape(r.shape))
    # hidden states are copies: asking for them changes nothing that is computed
    assert torch.equal(hid.logits, plain.logits) and torch.equal(hid.pooler_output, plain.pooler_output)

    full = model(pixel_values=x, output_hidden_states=True, output_attentions=True)
    assert len(full.attentions) == n_layers
    e_p = [maxerr(t, w) for t, w in zip(full.attentions, want["attentions"])]
    sums = max(float((t.double().sum(-1) - 1).abs().max()) for t in full.attentions)
    e_h2 = [maxerr(t, w) for t, w in zip(full.hidden_states, want["hidden_states"])]
    e_out = (maxerr(full.logits, want["logits"]), maxerr(full.pooler_output, want["pooled"]),
             maxerr(full.last_hidden_state, want["last_hidden_state"]))
    print(f"GPUTEST swin outputs model {name} B{batch} {precision}: probs {max(e_p):.2e}, row sums {sums:.2e}, "
          f"hidden[:-1] {max(e_h[:-1] + e_h2[:-1]):.2e}, hidden[-1] {max(e_h[-1], e_h2[-1]):.2e}, "
          f"with maps: logits {e_out[0]:.2e}, pooled {e_out[1]:.2e}, last {e_out[2]:.2e}")
    if precision in ("fp32", "bf16"):  # no fused half exists: the maps' layers run the chain the plain call runs
        for a, b in ((full.logits, plain.logits), (full.pooler_output, plain.pooler_output),
                     (full.last_hidden_state, hid.last_hidden_state)):
            assert torch.equal(a, b)
        for a, b in zip(full.hidden_states, hid.hidden_states):
            assert torch.equal(a, b)
    # split-bf16 (and the others): within what tests/test_swin_geometry_gpu.py asks of logits, pooler_output, last_hidden_state
    bl, bp, bh = GEOMETRY_BOUNDS[precision]
    assert e_out[0] <= bl and e_out[1] <= bp and e_out[2] <= bh, e_out
    assert maxerr(hid.last_hidden_state, want["last_hidden_state"]) <= bh
    assert max(e_h[-1], e_h2[-1]) <= bh, (e_h, e_h2)
    assert max(e_h[:-1] + e_h2[:-1]) <= HIDDEN_BOUND[precision], (e_h, e_h2)
    assert sums <= 1e-5
    assert max(e_p) <= PROB_BOUND[precision], e_p
    if precision != "bf16":
        assert max(e_p) <= ATTENTION_MAP_BAR

    # one layer only: that layer's map, bit-equal to the all-layers call; the others are not built
    for layer in (1, n_layers - 1):
        one = model(pixel_values=x, output_attentions=[layer])
        assert [a is not None for a in one.attentions] == [i == layer for i in range(n_layers)]
        assert torch.equal(one.attentions[layer], full.attentions[layer]), layer
        assert one.hidden_states is None

    # the backbone: the view over the classifier's parameters and engine, and a SwinModel loaded from them
    view = model.swin
    vo = view(x, output_hidden_states=True, output_attentions=True)
    assert torch.equal(vo.last_hidden_state, full.last_hidden_state) and torch.equal(vo.pooler_output, full.pooler_output)
    assert all(torch.equal(a, b) for a, b in zip(vo.attentions, full.attentions))
    assert all(torch.equal(a, b) for a, b in zip(vo.reshaped_hidden_states, full.reshaped_hidden_states))
    assert model._engine is not None and view._engine is None  # one engine: the owner's
    alone = SW.SwinModel(hf)
    assert not alone.load_state_dict(view.state_dict(), strict=True).missing_keys
    alone = alone.to(dev).eval().set_precision(precision)
    ao = alone(x)
    assert ao.hidden_states is None and ao.attentions is None
    assert torch.equal(ao.last_hidden_state, hid.last_hidden_state) and torch.equal(ao.pooler_output, plain.pooler_output)
    assert ao[0] is ao.last_hidden_state and ao["pooler_output"] is ao.pooler_output
    nopool = SW.SwinModel(hf, add_pooling_layer=False)
    nopool.load_state_dict(view.state_dict())
    assert nopool.to(dev).eval().set_precision(precision)(x).pooler_output is None
