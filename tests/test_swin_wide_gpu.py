"""Swin with windows of 8 to 12 on the HIP path against the float64 twin (tests/swin_outputs_ref.py, pinned on live transformers
at these geometries by tests/test_swin_wide_host.py): logits, pooler_output, last_hidden_state, every hidden state, every
layer's attentions and the output_attentions=[...] subset form, on SwinForImageClassification, SwinModel and the `.swin` view.

Bounds are the project's own for the same quantities at windows of 2 to 7, imported unchanged: PROB_BOUND and HIDDEN_BOUND of
tests/test_swin_outputs_gpu.py, BOUNDS of tests/test_swin_geometry_gpu.py for logits / pooler_output / last_hidden_state (and
the last hidden state before the final LayerNorm). A probability error above 1e-3 in fp32 or split-bf16 is a failure whatever
was measured; single bf16 at model level is a sanity row.
"""
import pytest
import torch

from tests import swin_outputs_ref as R
from tests import swin_wide_ref as WR
from tests.test_swin_geometry_gpu import BOUNDS as GEOMETRY_BOUNDS
from tests.test_swin_outputs_gpu import ATTENTION_MAP_BAR, HIDDEN_BOUND, PROB_BOUND
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import swin as SW

pytestmark = pytest.mark.gpu

# hidden states before the last at Swin-B widths: 3 x the CPU-emulated error of each mode (test_wide_model_swin_b_widths)
SWINB_HIDDEN_BOUND = {"fp32": 3 * 2.61e-6, "bf16x3": 3 * 3.66e-5, "bf16": 3 * 1.92e-2}

_TWIN = {}


def twin(name, batch):
    if (name, batch) not in _TWIN:
        cfg, sd, x = WR.case(name, torch.float64, batch)
        _TWIN[name, batch] = R.backbone_outputs(sd, cfg, x)
    return _TWIN[name, batch]


def maxerr(got, want):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    assert torch.isfinite(got).all()
    return float((got - want).abs().max())


def _models(name, precision, dev):
    cfg, sd, _ = WR.case(name)
    hf = SW.SwinConfig(image_size=cfg["image_size"], num_channels=cfg["num_channels"], embed_dim=cfg["embed_dim"],
                       depths=cfg["depths"], num_heads=cfg["num_heads"], window_size=cfg["window_size"],
                       mlp_ratio=cfg["mlp_ratio"], layer_norm_eps=cfg["layer_norm_eps"], num_labels=cfg["num_labels"])
    model = SW.SwinForImageClassification(hf)
    msg = model.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    return cfg, hf, model.to(dev).eval().set_precision(precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", WR.TINY)
def test_wide_model_outputs_vs_twin(dev, name, precision):
    batch = 2
    cfg, hf, model = _models(name, precision, dev)
    x = WR.case(name, batch=batch)[2].to(dev)
    want = twin(name, batch)
    n_layers, n_hidden = sum(cfg["depths"]), len(cfg["depths"]) + 1
    bl, bp, bh = GEOMETRY_BOUNDS[precision]

    plain = model(pixel_values=x)
    assert plain.hidden_states is None and plain.attentions is None
    e_plain = (maxerr(plain.logits, want["logits"]), maxerr(plain.pooler_output, want["pooled"]))

    hid = model(pixel_values=x, output_hidden_states=True)
    assert len(hid.hidden_states) == len(hid.reshaped_hidden_states) == n_hidden and hid.attentions is None
    e_h = [maxerr(t, w) for t, w in zip(hid.hidden_states, want["hidden_states"])]
    for h, r, w in zip(hid.hidden_states, hid.reshaped_hidden_states, want["reshaped_hidden_states"]):
        assert tuple(r.shape) == tuple(w.shape)
        assert torch.equal(r, h.transpose(1, 2).reshape(r.shape))
    assert torch.equal(hid.logits, plain.logits) and torch.equal(hid.pooler_output, plain.pooler_output)
    e_last = maxerr(hid.last_hidden_state, want["last_hidden_state"])

    full = model(pixel_values=x, output_hidden_states=True, output_attentions=True)
    assert len(full.attentions) == n_layers
    e_p = [maxerr(t, w) for t, w in zip(full.attentions, want["attentions"])]
    sums = max(float((t.double().sum(-1) - 1).abs().max()) for t in full.attentions)
    e_h2 = [maxerr(t, w) for t, w in zip(full.hidden_states, want["hidden_states"])]
    e_out = (maxerr(full.logits, want["logits"]), maxerr(full.pooler_output, want["pooled"]),
             maxerr(full.last_hidden_state, want["last_hidden_state"]))
    print(f"GPUTEST swin wide model {name} {precision}: probs {max(e_p):.2e}, row sums {sums:.2e}, "
          f"hidden[:-1] {max(e_h[:-1] + e_h2[:-1]):.2e}, hidden[-1] {max(e_h[-1], e_h2[-1]):.2e}, plain logits {e_plain[0]:.2e}, "
          f"pooled {e_plain[1]:.2e}, last {e_last:.2e}; with maps: logits {e_out[0]:.2e}, pooled {e_out[1]:.2e}, last {e_out[2]:.2e}")
    if precision in ("fp32", "bf16"):  # no fused half exists: the maps' layers run the chain the plain call runs
        assert torch.equal(full.logits, plain.logits) and torch.equal(full.pooler_output, plain.pooler_output)
        assert torch.equal(full.last_hidden_state, hid.last_hidden_state)
        for a, b in zip(full.hidden_states, hid.hidden_states):
            assert torch.equal(a, b)
    assert e_plain[0] <= bl and e_plain[1] <= bp and e_last <= bh, (e_plain, e_last)
    assert e_out[0] <= bl and e_out[1] <= bp and e_out[2] <= bh, e_out
    assert max(e_h[-1], e_h2[-1]) <= bh, (e_h, e_h2)
    assert max(e_h[:-1] + e_h2[:-1]) <= HIDDEN_BOUND[precision], (e_h, e_h2)
    assert sums <= 1e-5
    assert max(e_p) <= PROB_BOUND[precision], e_p
    if precision != "bf16":
        assert max(e_p) <= ATTENTION_MAP_BAR

    # the subset form: that layer's map, bit-equal to the all-layers call; the others are not built
    for layer in (1, n_layers - 1):
        one = model(pixel_values=x, output_attentions=[layer])
        assert [a is not None for a in one.attentions] == [i == layer for i in range(n_layers)]
        assert torch.equal(one.attentions[layer], full.attentions[layer]), layer

    # the backbone: the view over the classifier's parameters and engine, and a SwinModel loaded from them
    view = model.swin
    vo = view(x, output_hidden_states=True, output_attentions=True)
    assert torch.equal(vo.last_hidden_state, full.last_hidden_state) and torch.equal(vo.pooler_output, full.pooler_output)
    assert all(torch.equal(a, b) for a, b in zip(vo.attentions, full.attentions))
    assert all(torch.equal(a, b) for a, b in zip(vo.hidden_states, full.hidden_states))
    alone = SW.SwinModel(hf)
    assert not alone.load_state_dict(view.state_dict(), strict=True).missing_keys
    alone = alone.to(dev).eval().set_precision(precision)
    ao = alone(x)
    assert ao.hidden_states is None and ao.attentions is None
    assert torch.equal(ao.last_hidden_state, hid.last_hidden_state) and torch.equal(ao.pooler_output, plain.pooler_output)
    # (the layers behind the last requested map stay on their fused kernels: only the map itself is compared)
    assert torch.equal(alone(x, output_attentions=[0]).attentions[0], full.attentions[0])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_wide_model_swin_b_widths(dev, precision):
    """384^2, embed_dim 128, heads 4 / 8 / 16 / 32, C up to 1024, two layers per stage, B = 1: logits and hidden states.

    logits, pooler_output, last_hidden_state and the last hidden state take tests/test_swin_geometry_gpu.py's bounds (measured
    there at 1024 channels). HIDDEN_BOUND for the hidden states before the last was measured on two-stage models of 32 to 192
    channels and does not hold at these widths for any arithmetic: the float64 twin's own float32 evaluation on the CPU
    (tools/emulate_swin_wide.py swinb) is 1.2e-6 / 1.5e-6 / 1.9e-6 / 2.6e-6 off on hidden_states[0..3], with split-bf16
    operand rounding emulated 1.1e-5 / 2.0e-5 / 3.7e-5 on [1..3], with bf16 rounding 5.4e-3 / 1.0e-2 / 1.9e-2 (the residual stream
    is carried through four stages, the contractions are up to 4096 long). SWINB_HIDDEN_BOUND is 3 x the largest emulated error
    of each mode, the project's margin; measured on MI355X: fp32 6.9e-6."""
    cfg, hf, model = _models("swinb", precision, dev)
    x = WR.case("swinb", batch=1)[2].to(dev)
    want = twin("swinb", 1)
    out = model(pixel_values=x, output_hidden_states=True)
    e_h = [maxerr(t, w) for t, w in zip(out.hidden_states, want["hidden_states"])]
    e = (maxerr(out.logits, want["logits"]), maxerr(out.pooler_output, want["pooled"]),
         maxerr(out.last_hidden_state, want["last_hidden_state"]))
    print(f"GPUTEST swin wide model swinb {precision}: logits {e[0]:.2e}, pooled {e[1]:.2e}, last {e[2]:.2e}, "
          f"hidden[:-1] {max(e_h[:-1]):.2e}, hidden[-1] {e_h[-1]:.2e}")
    bl, bp, bh = GEOMETRY_BOUNDS[precision]
    assert e[0] <= bl and e[1] <= bp and e[2] <= bh, e
    assert e_h[-1] <= bh and max(e_h[:-1]) <= SWINB_HIDDEN_BOUND[precision], e_h


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_wide_fuse_option(lib, dev, precision):
    """OCM_SWIN_OPT_FUSE_MLP 0 against 1 at embed_dim 128 (where split-bf16 has fused LayerNorm + qkv and MLP kernels): the
    same bits in fp32 and bf16, agreement to fp32 rounding — within the geometry bounds of either against the twin — in
    split-bf16."""
    cfg, hf, model = _models("swinb", precision, dev)
    x = WR.case("swinb", batch=1)[2].to(dev)
    want = twin("swinb", 1)
    fused = model(pixel_values=x, output_hidden_states=True)
    eng = model._get_engine(torch.device(dev))
    _lib.check(lib.ocm_swin_set_option(eng["h"], _lib.OCM_SWIN_OPT_FUSE_MLP, 0))
    try:
        plain = model(pixel_values=x, output_hidden_states=True)
    finally:
        _lib.check(lib.ocm_swin_set_option(eng["h"], _lib.OCM_SWIN_OPT_FUSE_MLP, 1))
    d = (maxerr(plain.logits, fused.logits.cpu().double()), maxerr(plain.last_hidden_state, fused.last_hidden_state.cpu().double()))
    print(f"GPUTEST swin wide fuse option {precision}: |unfused - fused| logits {d[0]:.2e}, last {d[1]:.2e}")
    bl, bp, bh = GEOMETRY_BOUNDS[precision]
    if precision == "bf16x3":
        assert d[0] > 0 or d[1] > 0  # the two chains really differ
        assert d[0] <= bl and d[1] <= bh
        assert maxerr(plain.logits, want["logits"]) <= bl and maxerr(plain.last_hidden_state, want["last_hidden_state"]) <= bh
    else:
        assert torch.equal(plain.logits, fused.logits) and torch.equal(plain.last_hidden_state, fused.last_hidden_state)
