"""SwinForImageClassification.enable_wide_window_training on the HIP path: training with windows of 8 to 12 (the window12-384
geometry). Every parameter's gradient and the training-forward logits against the float64 CPU twin
(oracle.swin_oracle.swin_forward under torch autograd; with stochastic depth the restated layer of tests/test_swin_train_gpu.py with
the masks the module drew), a frozen subset, accumulation, the eval-mode forward after AdamW steps, and no drift for windows of 7.
Needs an MI355X.

Error measure and limits are those of tests/test_swin_train_gpu.py, imported unchanged (max |g - g64| / max |g64| per tensor).
Measured worst per precision and case: DESIGN.md 3.36."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import swin_oracle as SO
from tests import swin_outputs_ref as R
from tests import swin_wide_ref as WR
from tests import test_swin_train_gpu as TG
from tests.test_swin_train_gpu import TOL, _check, _grads, _loss, _rel
from vit_ocm_wmsegmentation_amd import synth
from vit_ocm_wmsegmentation_amd import swin as SW

pytestmark = pytest.mark.gpu

# (config, seed, batch, needs enable_padded_training)
CASES = {k: (dict(synth.SWIN_TINY, **WR.GEOMETRIES[k][0]), WR.GEOMETRIES[k][1], 2, k == "w80") for k in WR.TINY}
# Swin-B's first two widths: grids 24 -> 12, 4 and 8 heads
CASES["b96"] = (dict(synth.SWIN_TINY, image_size=96, embed_dim=128, depths=(2, 2), num_heads=(4, 8), window_size=12), 27, 2, False)
# Swin-B's four widths on a 384^2 tile, two layers per stage, one image
CASES["swinb"] = (dict(synth.SWIN_TINY, **WR.SWIN_B[0]), WR.SWIN_B[1], 1, False)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cfg, seed, batch, _ = CASES[name]
    sd = synth.synth_swin_state_dict(cfg, seed=seed, qk_gain=R.QK_GAIN)
    x = synth.synth_tiles(batch, cfg["image_size"], seed=seed + 50, channels=cfg["num_channels"])
    labels = torch.randint(0, cfg["num_labels"], (batch,), generator=torch.Generator().manual_seed(seed))
    return cfg, sd, x, labels


def _model(name, precision, dev, rate=0.0):
    cfg, sd, x, labels = _inputs(name)
    m = SW.SwinForImageClassification(SW.SwinConfig(**{k: v for k, v in cfg.items() if k != "patch_size"}, drop_path_rate=rate))
    assert not m.load_state_dict(sd, strict=True).missing_keys
    m = m.to(dev).set_precision(precision).train().requires_grad_(True).enable_wide_window_training()
    return m.enable_padded_training(CASES[name][3]), x.to(dev), labels.to(dev)


def _twin(name, masks=None):
    """(gradients, logits) of the float64 twin."""
    cfg, sd, x, labels = _inputs(name)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    if masks is None:
        logits = SO.swin_forward.__wrapped__(prm, cfg, x.double())["logits"]
    else:
        logits = TG._twin_logits(prm, cfg, x.double(), masks)
    F.cross_entropy(logits, labels).backward()
    return {k: v.grad for k, v in prm.items()}, logits.detach()


@functools.lru_cache(maxsize=None)
def _reference(name):
    return _twin(name)


def _grads_and_logits(dev, name, precision):
    m, x, labels = _model(name, precision, dev)
    out = m(pixel_values=x, labels=labels)
    out.loss.backward()
    ref, logits64 = _reference(name)
    e = _rel(out.logits, logits64)
    per = m.__dict__["_train_kept_bytes"] / x.shape[0]
    print(f"GPUTEST swin wide train {name} {precision}: logits {e:.3e}, kept {per / 2 ** 20:.1f} MiB per image")
    errs = _check(m, ref, TOL[precision], f"wide {name} {precision}")
    worst = max(v for k, v in errs.items() if k.endswith("relative_position_bias_table"))
    print(f"GPUTEST swin wide train {name} {precision}: worst relative_position_bias_table {worst:.3e}")
    assert e <= TOL[precision], f"{name} {precision}: logits {e:.3e} > {TOL[precision]:.0e}"


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", list(WR.TINY) + ["b96"])
def test_grads_and_logits_match_float64(dev, name, precision):
    """Drop-path rate 0, batch 2: windows of 12 (grid = window, shift in both stages), 8 on padded grids, 9 and 11, and Swin-B's
    first two widths."""
    _grads_and_logits(dev, name, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_swin_b_widths_match_float64(dev, precision):
    """384^2, C = 128 .. 1024, 4 .. 32 heads, windows of 12 on grids 96 / 48 / 24 / 12."""
    _grads_and_logits(dev, "swinb", precision)


def test_grads_match_float64_with_drop_path(dev):
    """drop_path_rate 0.1 on w192: the masks the module drew, redrawn from the same seed, go to the twin."""
    m, x, labels = _model("w192", "bf16x3", dev, rate=0.1)
    torch.manual_seed(123)
    out = m(pixel_values=x, labels=labels)
    out.loss.backward()
    torch.manual_seed(123)
    masks = SW.draw_drop_path_masks(m.config, x.shape[0], dev)
    assert masks[0] is None and all(mk is not None for mk in masks[1:])
    ref, logits64 = _twin("w192", masks)
    _check(m, ref, TOL["bf16x3"], "wide w192 drop path 0.1 bf16x3")
    assert _rel(out.logits, logits64) <= TOL["bf16x3"]


def test_frozen_subset_and_accumulation(dev):
    """w88: frozen parameters get .grad None and the others the full run's bits; a second loss.backward() from a second forward
    doubles every gradient exactly."""
    m, x, labels = _model("w88", "bf16x3", dev)
    _loss(m, x, labels, None).backward()
    full = {k: g.clone() for k, g in _grads(m).items()}
    _loss(m, x, labels, None).backward()
    for k, g in _grads(m).items():
        assert torch.equal(g, 2 * full[k]), k

    def frozen(k):
        return k.startswith("swin.embeddings.") or k.startswith("swin.encoder.layers.0.")

    m.zero_grad(set_to_none=True)
    for n, p in m.named_parameters():
        p.requires_grad_(not frozen(m._names[n]))
    _loss(m, x, labels, None).backward()
    for k, g in _grads(m).items():
        if frozen(k):
            assert g is None, k
        else:
            assert torch.equal(g, full[k]), k
    assert any(frozen(k) for k in full) and not all(frozen(k) for k in full)


def test_eval_after_adamw_steps_matches_a_fresh_module(dev):
    """Two AdamW steps on w96, then eval(): the engine sees the trained weights — the logits of a fresh module loaded with the
    trained state_dict, bit for bit. The opt-in is not in the state_dict."""
    m, x, labels = _model("w96", "bf16x3", dev)
    before = m.eval()(pixel_values=x).logits.clone()
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    for _ in range(2):
        m(pixel_values=x, labels=labels).loss.backward()
        opt.step()
        opt.zero_grad()
    got = m.eval()(pixel_values=x).logits
    assert not torch.equal(got, before)
    assert not any("wide" in k for k in m.state_dict())
    fresh = SW.SwinForImageClassification(m.config)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev).set_precision("bf16x3").eval()
    assert torch.equal(got, fresh(pixel_values=x).logits)
    assert not fresh.__dict__.get("_wide_window_training", False)


def test_opt_in_changes_nothing_for_windows_of_7(dev):
    """Geometry H (windows of 7): the same logits, gradient bits and kept bytes with the flag on and off."""
    got = []
    for wide in (False, True):
        m, x, labels, up = TG._model("geom_H", "bf16x3", dev)
        m.enable_wide_window_training(wide)
        out = m(pixel_values=x, labels=labels)
        out.loss.backward()
        got.append((out.logits.detach().clone(), _grads(m), m.__dict__["_train_kept_bytes"]))
    assert torch.equal(got[0][0], got[1][0]) and got[0][2] == got[1][2]
    for k, g in got[0][1].items():
        assert torch.equal(g, got[1][1][k]), k


def test_refused_without_the_opt_in(dev):
    m, x, labels = _model("w96", "bf16x3", dev)
    m.enable_wide_window_training(False)
    with pytest.raises(NotImplementedError, match="windows of 2 to 7.*enable_wide_window_training"):
        m(pixel_values=x, labels=labels)
    out = m.enable_wide_window_training()(pixel_values=x, labels=labels, output_hidden_states=True)
    assert out.last_hidden_state.shape == (2, 144, 64) and out.hidden_states is None  # 12 x 12 tokens, C = 64
    out.loss.backward()
