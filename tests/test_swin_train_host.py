"""CPU-side checks of Swin training: the config fields, the stochastic-depth masks against transformers' SwinDropPath draws, the
output object's Trainer-style indexing and the refusal of a CPU input."""
import pytest
import torch

from vit_ocm_wmsegmentation_amd import swin as SW


def test_config_training_fields():
    c = SW.SwinConfig(num_labels=5)
    assert c.drop_path_rate == 0.1 and c.hidden_dropout_prob == 0.0 and c.attention_probs_dropout_prob == 0.0
    rates = SW.drop_path_rates(c)
    assert len(rates) == 12 and rates[0] == 0.0 and rates[-1] == pytest.approx(0.1)
    assert SW.drop_path_rates(SW.SwinConfig(depths=(1,), num_heads=(3,))) == [0.0]


def test_drop_path_masks_match_transformers():
    """Same generator state, same order: the masks equal what transformers' SwinDropPath modules of a SwinEncoder draw."""
    tr = pytest.importorskip("transformers")
    from transformers.models.swin import modeling_swin as MS
    cfg = dict(image_size=32, patch_size=4, embed_dim=32, depths=[2, 3], num_heads=[1, 2], window_size=4, drop_path_rate=0.3)
    enc = MS.SwinEncoder(tr.SwinConfig(**cfg), (8, 8)).train()
    mods = [blk.drop_path for stage in enc.layers for blk in stage.blocks]
    B = 6
    torch.manual_seed(7)
    want = []
    for mod in mods:
        if isinstance(mod, MS.SwinDropPath):
            keep = 1 - mod.drop_prob
            want.append((keep, (mod(torch.ones(B, 4, 8)) * keep)[:, 0, 0]))
        else:
            want.append(None)
    torch.manual_seed(7)
    got = SW.draw_drop_path_masks(SW.SwinConfig(**cfg), B, torch.device("cpu"))
    assert len(got) == len(want) == 5 and got[0] is None and want[0] is None
    for g, w in zip(got[1:], want[1:]):
        assert g[0] == pytest.approx(w[0], abs=1e-12)
        assert torch.equal(g[1], torch.round(w[1]))
    assert any(float(g[1].min()) == 0 for g in got[1:]) and any(float(g[1].max()) == 1 for g in got[1:])


def test_output_indexing():
    loss, logits = torch.tensor(1.0), torch.zeros(2, 5)
    out = SW.SwinOutput(loss=loss, logits=logits, pooler_output=None, last_hidden_state=None)
    assert out["loss"] is loss and out[0] is loss and out[1] is logits and out.to_tuple() == (loss, logits)
    out = SW.SwinOutput(loss=None, logits=logits, pooler_output=None, last_hidden_state=None)
    assert out[0] is logits and out["logits"] is logits


def test_training_mode_on_cpu_still_refuses_first():
    m = SW.SwinForImageClassification(SW.SwinConfig(image_size=56, depths=(2, 2), num_heads=(3, 6), num_labels=5))
    m.train().requires_grad_(True)
    with pytest.raises(RuntimeError, match="HIP"):
        m(pixel_values=torch.zeros(1, 3, 56, 56), labels=torch.zeros(1, dtype=torch.int64))
