"""End-to-end parity AT THE BATCH SIZES BASELINE.json names. Kernel selection depends on the row count (tile shapes,
LDS-DMA vs register staging, fused GEMM + LayerNorm, 4- / 8-wave attention), and the golden fixtures have B <= 2: these
tests run the launches the bench runs and compare sampled images / windows with the CPU oracle on the same inputs.

  config 2  ViT-S/16, 64 tiles of 224^2 : images 0, 31, 63 on the init / sharp / peaked weight sets
  config 3  ViT-B/16, 128 tiles of 384^2: images 0 and 127 on the full and the calibrated stress ("qkv6.5") sets
  config 4  ViT-S/8, 4096^2 slab, 900 windows of 384^2 through SlidingWindowAttention's auto batch plan: the two
            corner windows and the centre one (CLS rows)
Bar: 1e-3 absolute on attention probabilities (north star), in the default split-bf16 arithmetic. Needs an MI355X."""
import pytest
import torch

from oracle import vit_oracle as O
from tests.memcheck import assert_same_bits
import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
from vit_ocm_wmsegmentation_amd import synth
from vit_ocm_wmsegmentation_amd.sw_processing import SlidingWindowAttention, sliding_window_origins

pytestmark = pytest.mark.gpu
ATTN_TOL = 1e-3


def _model(arch, patch, variant, dev):
    model = vits.__dict__[arch](patch_size=patch, num_classes=0)
    sd = synth.synth_arch_state_dict(arch, patch, seed=0, variant=variant)
    model.load_state_dict(sd)
    return model.eval().to(dev), sd, O.make_cfg(sd, patch, synth.ARCHS[arch][2])


@pytest.mark.parametrize("variant", ["init", "sharp", "peaked"])
def test_config2_batch64_sampled_images(dev, variant):
    model, sd, cfg = _model("vit_small", 16, variant, dev)
    x = synth.synth_tiles(64, 224, seed=1234)
    attn = model.get_last_selfattention(x.to(dev))  # the bench's call: 12 608 token rows
    rows = model.get_last_attention_rows(x.to(dev))  # CLS rows through the flash statistics (the sliding-window route)
    assert attn.shape == (64, 6, 197, 197) and rows.shape == (64, 6, 1, 196)
    pick = [0, 31, 63]
    ref = O.get_last_selfattention(sd, cfg, x[pick])
    e = float((attn[pick].cpu() - ref).abs().max())
    e_rows = float((rows[pick, :, 0].cpu() - ref[:, :, 0, 1:]).abs().max())
    print(f"\n[config 2, {variant}] attention L_inf on images {pick}: {e:.2e} (CLS rows {e_rows:.2e}), attn max {float(ref.max()):.3f}")
    assert e <= ATTN_TOL and e_rows <= ATTN_TOL
    assert float((attn.sum(-1) - 1).abs().max()) < 1e-4  # every row of every image is a distribution
    # the same images one per call (other kernels: M <= 1024 paths) agree with their batched results
    one = model.get_last_selfattention(x[31:32].to(dev))
    assert float((one[0] - attn[31]).abs().max()) <= (2e-4 if variant == "peaked" else 2e-6)
    # intermediate features / qkv of the last block through get_intermediate_feat at the same batch
    feat, attns, qkvs = model.get_intermediate_feat(x.to(dev), n=1)
    assert_same_bits(attns[0], attn, "get_intermediate_feat attns[0] vs get_last_selfattention", ("image", "head", "row", "col"))
    ofeat, _, oqkv = O.get_intermediate_feat(sd, cfg, x[pick], 1)
    scale = float(ofeat[0].abs().max())
    assert float((feat[0][pick].cpu() - ofeat[0]).abs().max()) / scale < (2e-3 if variant == "peaked" else 2e-4)
    assert float((qkvs[0][:, pick].cpu() - oqkv[0]).abs().max()) / float(oqkv[0].abs().max()) < (2e-3 if variant == "peaked" else 2e-4)


@pytest.mark.parametrize("variant", ["full", "qkv6.5"])
def test_config3_vitb_batch128_sampled_images(dev, variant):
    model, sd, cfg = _model("vit_base", 16, variant, dev)
    x = synth.synth_tiles(128, 384, seed=99)
    attn = model.get_last_selfattention(x.to(dev))  # 73 856 token rows: 256 x 256 LDS-DMA tiles
    assert attn.shape == (128, 12, 577, 577)
    pick = [0, 127]
    ref = O.get_last_selfattention(sd, cfg, x[pick])
    e = float((attn[pick].cpu() - ref).abs().max())
    print(f"\n[config 3, {variant}] attention L_inf on images {pick}: {e:.2e}, attn max {float(ref.max()):.3f}")
    assert e <= ATTN_TOL
    rs = attn.sum(-1)
    assert float((rs - 1).abs().max()) < 1e-4
    del attn, rs
    rows = model.get_last_attention_rows(x.to(dev))
    assert float((rows[pick, :, 0].cpu() - ref[:, :, 0, 1:]).abs().max()) <= ATTN_TOL


def test_config4_slab_sweep_sampled_windows(dev):
    model, sd, cfg = _model("vit_small", 8, "sharp", dev)
    slab = synth.synth_tiles(1, 4096, seed=7)[0]
    sweep = SlidingWindowAttention(model, window=384, stride=128)  # auto batch plan, as bench.py's slab_sweep
    maps = sweep(slab.to(dev))
    assert maps.shape == (900, 6, 1, 48, 48)
    # forwards of this size keep their LayerNorm kernels ("auto"); the folded form of the same sweep agrees with them
    eng = model._engine(dev)
    try:
        eng.set_fold_layernorm("always")
        maps_folded = sweep(slab.to(dev))
    finally:
        eng.set_fold_layernorm("auto")
    assert float((maps_folded - maps).abs().max()) < 1e-6
    origins = sliding_window_origins(4096, 4096, 128)
    assert origins.shape == (900, 2) and tuple(origins[-1]) == (3712, 3712)
    pick = [0, 15 * 30 + 15, 899]  # first corner, centre, last corner
    crops = torch.stack([slab[:, y:y + 384, x:x + 384] for (y, x) in origins[pick].tolist()])
    ref = O.get_last_selfattention(sd, cfg, crops)[:, :, 0, 1:].reshape(3, 6, 48, 48)
    e = float((maps[pick, :, 0].cpu() - ref).abs().max())
    print(f"\n[config 4] CLS-row L_inf on windows {pick}: {e:.2e} (row max {float(ref.max()):.4f})")
    assert e <= ATTN_TOL
    # relative check too: CLS rows over 2304 keys are ~4e-4 each, so 1e-3 absolute alone would not see much
    assert float(((maps[pick, :, 0].cpu() - ref).abs() / ref).max()) < 1e-2
    assert float((maps.sum((-1, -2)) - 1).abs().max()) < 1e-2  # CLS row minus its own CLS column: close to 1


def test_misaligned_slab_view_is_copied(dev):
    """a unit-stride view whose rows do not start on 16-byte boundaries must not reach the float4 gather."""
    case_model, sd, cfg = _model("vit_small", 16, "sharp", dev)
    big = torch.zeros(3, 224 + 128, 224 + 128 + 8, device=dev)
    tile = synth.synth_tiles(1, 224 + 128, seed=3)[0].to(dev)
    big[:, :, 1:1 + 352] = tile
    view = big[:, :, 1:1 + 352]  # stride(2) == 1, width % 4 == 0, data_ptr % 16 == 4
    assert view.stride(2) == 1 and view.data_ptr() % 16 != 0
    sweep = SlidingWindowAttention(case_model, window=224, stride=64, batch_tiles=4)
    assert torch.equal(sweep(view), sweep(tile))


@pytest.mark.parametrize("precision,tol", [("bf16x3", 1e-3), ("fp32", 2e-4)])
def test_config5_swin_batch256_sampled_images(dev, precision, tol):
    """BASELINE config 5 at ITS batch: Swin-T 224^2, 256 images (Allen_data_Backbone/train.py:70-85). At B = 256 the stages
    dispatch other kernels than the B = 2 / 3 fixtures (802 816 .. 12 544 token rows: 128 x 192 / 256 x 256 / eight-wave
    128 x 128 LDS-DMA tiles instead of the small-row paths; profiles/r03_kernel_stats_swin.csv), so the first, middle and
    last image are compared with the transformers-pinned oracle run on the same synthetic weights: logits and pooled output
    at the ViT path's 1e-3 in the default split-bf16 arithmetic, 2e-4 in fp32 mode."""
    from oracle import swin_oracle as SO
    from vit_ocm_wmsegmentation_amd import swin as SW
    cfg = dict(synth.SWIN_TINY)
    sd = synth.synth_swin_state_dict(cfg, seed=21, qk_gain=6.0)
    x = synth.synth_tiles(256, 224, seed=71)
    model = SW.SwinForImageClassification(SW.SwinConfig(num_labels=cfg["num_labels"]))
    assert not model.load_state_dict(sd, strict=True).missing_keys
    model = model.to(dev).eval().set_precision(precision)
    out = model(pixel_values=x.to(dev), output_hidden_states=True)
    assert tuple(out.logits.shape) == (256, cfg["num_labels"])
    pick = [0, 127, 255]
    want = SO.swin_forward(sd, cfg, x[pick])
    e_log = float((out.logits[pick].cpu() - want["logits"]).abs().max())
    e_pool = float((out.pooler_output[pick].cpu() - want["pooled"]).abs().max())
    e_hid = float((out.last_hidden_state[pick].cpu() - want["last_hidden_state"]).abs().max())
    print(f"\n[config 5, {precision}] Swin-T B=256 images {pick}: logits {e_log:.2e}, pooled {e_pool:.2e}, last hidden {e_hid:.2e}")
    assert e_log <= tol and e_pool <= tol and e_hid <= 4 * tol
    assert torch.equal(out.logits[pick].argmax(-1).cpu(), want["logits"].argmax(-1))
    # the same three images as a batch of three (the small-row dispatch) agree with their rows of the big batch
    small = model(pixel_values=x[pick].to(dev))
    assert float((small.logits - out.logits[pick]).abs().max()) <= tol
    assert torch.isfinite(out.logits).all()
