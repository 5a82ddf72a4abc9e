"""End-to-end parity AT THE BATCH SIZES BASELINE.json names. Kernel selection depends on the row count (tile shapes,
LDS-DMA vs register staging, fused GEMM + LayerNorm, 4- / 8-wave attention), and the golden fixtures have B <= 2: these
tests run the launches the bench runs and compare sampled images / windows with the CPU oracle on the same inputs.

  config 2  ViT-S/16, 64 tiles of 224^2 : images 0, 31, 63 on the init / sharp / peaked weight sets
  config 3  ViT-B/16, 128 tiles of 384^2: images 0 and 127 on the full and the calibrated stress ("qkv6.5") sets
  config 4  ViT-S/8, 4096^2 slab, 900 windows of 384^2 through SlidingWindowAttention's auto batch plan: the two
            corner windows and the centre one (CLS rows)
Each config runs in all three precisions of DESIGN §5. Bars on attention probabilities: 1e-3 absolute (north star) in the
default split-bf16 arithmetic; in fp32, about 3x the measured value (the oracle's own fp32 round-off); in single bf16,
1e-3 on the init / sharp / full sets and the sweep, and on the peaked and calibrated stress sets, where that mode is not
claimed, 2-3x the measured 5.2e-2 / 0.18, beside the checks that hold in every mode (every row a distribution,
B = 1 against batched, the two entry points and bench.py's call bit for bit).
Needs an MI355X."""
import functools

import pytest
import torch

from oracle import vit_oracle as O
from tests.memcheck import assert_same_bits
import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
from vit_ocm_wmsegmentation_amd import _lib, synth
from vit_ocm_wmsegmentation_amd.sw_processing import SlidingWindowAttention, sliding_window_origins

pytestmark = pytest.mark.gpu
ATTN_TOL = 1e-3
BENCH_FLAGS = _lib.OCM_OUT_ATTN | _lib.OCM_OUT_ROWS | _lib.OCM_LAST_ATTN_ONLY  # bench.py's timed call


def _model(arch, patch, variant, dev, precision="bf16x3"):
    model = vits.__dict__[arch](patch_size=patch, num_classes=0)
    sd = synth.synth_arch_state_dict(arch, patch, seed=0, variant=variant)
    model.load_state_dict(sd)
    return model.eval().to(dev).set_precision(precision), sd, O.make_cfg(sd, patch, synth.ARCHS[arch][2])


@functools.lru_cache(maxsize=None)
def _oracle(arch, patch, variant, what):
    """The CPU oracle's result for the sampled images / windows of one config and weight set: computed once, shared by
    the three precisions (it does not depend on them)."""
    sd = synth.synth_arch_state_dict(arch, patch, seed=0, variant=variant)
    cfg = O.make_cfg(sd, patch, synth.ARCHS[arch][2])
    if what == "config2":
        x = synth.synth_tiles(64, 224, seed=1234)[[0, 31, 63]]
        return O.get_last_selfattention(sd, cfg, x), O.get_intermediate_feat(sd, cfg, x, 1)
    if what == "config3":
        return O.get_last_selfattention(sd, cfg, synth.synth_tiles(128, 384, seed=99)[[0, 127]])
    slab = synth.synth_tiles(1, 4096, seed=7)[0]
    origins = sliding_window_origins(4096, 4096, 128)[[0, 15 * 30 + 15, 899]]
    crops = torch.stack([slab[:, y:y + 384, x:x + 384] for (y, x) in origins.tolist()])
    return O.get_last_selfattention(sd, cfg, crops)[:, :, 0, 1:].reshape(3, 6, 48, 48)


# Config 2 bounds per (precision, weight set): attention and CLS rows against the oracle, one image per call against its
# batched result, feat / qkv of the last block relative to their largest value. split-bf16: as before; fp32: about 3x the
# measured value; single bf16: 1e-3 off the stress sets, 1e-1 on the peaked one (measured 5.2e-2),
# feat / qkv about 3x the measured value. B = 1 against batched measures 0 in fp32 and bf16: the split-bf16 bounds hold.
C2_BOUNDS = {
    ("bf16x3", "init"): (ATTN_TOL, 2e-6, 2e-4), ("bf16x3", "sharp"): (ATTN_TOL, 2e-6, 2e-4),
    ("bf16x3", "peaked"): (ATTN_TOL, 2e-4, 2e-3),
    ("fp32", "init"): (2e-8, 2e-6, 5e-6), ("fp32", "sharp"): (3e-7, 2e-6, 5e-6), ("fp32", "peaked"): (5e-5, 2e-4, 3e-5),
    ("bf16", "init"): (ATTN_TOL, 2e-6, 2e-2), ("bf16", "sharp"): (ATTN_TOL, 2e-6, 2e-2), ("bf16", "peaked"): (1e-1, 2e-4, 6e-2),
}


def _ids(cases):  # the split-bf16 cases keep the ids they had before the precision axis was added
    return [pytest.param(p, v, id=v if p == "bf16x3" else f"{p}-{v}") for p, v in cases]


@pytest.mark.parametrize("precision,variant", _ids((p, v) for p in ("bf16x3", "fp32", "bf16") for v in ("init", "sharp", "peaked")))
def test_config2_batch64_sampled_images(dev, precision, variant):
    model, sd, cfg = _model("vit_small", 16, variant, dev, precision)
    tol, tol_one, tol_rel = C2_BOUNDS[(precision, variant)]
    x = synth.synth_tiles(64, 224, seed=1234)
    attn = model.get_last_selfattention(x.to(dev))  # the bench's call: 12 608 token rows
    rows = model.get_last_attention_rows(x.to(dev))  # CLS rows through the flash statistics (the sliding-window route)
    assert attn.shape == (64, 6, 197, 197) and rows.shape == (64, 6, 1, 196)
    pick = [0, 31, 63]
    ref, (ofeat, _, oqkv) = _oracle("vit_small", 16, variant, "config2")
    e = float((attn[pick].cpu() - ref).abs().max())
    e_rows = float((rows[pick, :, 0].cpu() - ref[:, :, 0, 1:]).abs().max())
    # the same images one per call (other kernels: M <= 1024 paths) agree with their batched results
    one = model.get_last_selfattention(x[31:32].to(dev))
    e_one = float((one[0] - attn[31]).abs().max())
    # intermediate features / qkv of the last block through get_intermediate_feat at the same batch
    feat, attns, qkvs = model.get_intermediate_feat(x.to(dev), n=1)
    e_feat = float((feat[0][pick].cpu() - ofeat[0]).abs().max()) / float(ofeat[0].abs().max())
    e_qkv = float((qkvs[0][:, pick].cpu() - oqkv[0]).abs().max()) / float(oqkv[0].abs().max())
    print(f"\n[config 2, {precision}, {variant}] attention L_inf on images {pick}: {e:.2e} (CLS rows {e_rows:.2e}), "
          f"attn max {float(ref.max()):.3f}; B = 1 vs batched {e_one:.2e}; feat rel {e_feat:.2e}, qkv rel {e_qkv:.2e}")
    assert e <= tol and e_rows <= tol
    assert float((attn.sum(-1) - 1).abs().max()) < 1e-4  # every row of every image is a distribution
    assert e_one <= tol_one
    assert_same_bits(attns[0], attn, "get_intermediate_feat attns[0] vs get_last_selfattention", ("image", "head", "row", "col"))
    assert e_feat < tol_rel and e_qkv < tol_rel
    _assert_bench_call(model, x.to(dev), attn)


def _assert_bench_call(model, x, attn):
    """bench.py's timed call (probabilities and CLS rows from one forward, the rows sliced out of the probabilities)
    returns the bits of get_last_selfattention."""
    out = model._run(x, flags=BENCH_FLAGS)
    assert_same_bits(out["attn"][0], attn, "bench call attn vs get_last_selfattention", ("image", "head", "row", "col"))
    assert_same_bits(out["rows"], attn[:, :, :1, 1:], "bench call CLS rows vs attn[:, :, 0, 1:]", ("image", "head", "row", "col"))


# config 3: fp32 about 3x the measured value; single bf16 1e-3 on the full set and 0.5 on the calibrated one (measured 0.18:
# ViT-B's twelve layers amplify 8-bit operands further than ViT-S's)
C3_BOUNDS = {("bf16x3", "full"): ATTN_TOL, ("bf16x3", "qkv6.5"): ATTN_TOL, ("fp32", "full"): 2e-8, ("fp32", "qkv6.5"): 1.5e-4,
             ("bf16", "full"): ATTN_TOL, ("bf16", "qkv6.5"): 0.5}


@pytest.mark.parametrize("precision,variant", _ids((p, v) for p in ("bf16x3", "fp32", "bf16") for v in ("full", "qkv6.5")))
def test_config3_vitb_batch128_sampled_images(dev, precision, variant):
    model, sd, cfg = _model("vit_base", 16, variant, dev, precision)
    tol = C3_BOUNDS[(precision, variant)]
    x = synth.synth_tiles(128, 384, seed=99)
    attn = model.get_last_selfattention(x.to(dev))  # 73 856 token rows: 256 x 256 LDS-DMA tiles (split-bf16)
    assert attn.shape == (128, 12, 577, 577)
    pick = [0, 127]
    ref = _oracle("vit_base", 16, variant, "config3")
    e = float((attn[pick].cpu() - ref).abs().max())
    rs = attn.sum(-1)
    e_sum = float((rs - 1).abs().max())
    del rs
    _assert_bench_call(model, x.to(dev), attn)
    del attn
    rows = model.get_last_attention_rows(x.to(dev))
    e_rows = float((rows[pick, :, 0].cpu() - ref[:, :, 0, 1:]).abs().max())
    print(f"\n[config 3, {precision}, {variant}] attention L_inf on images {pick}: {e:.2e} (CLS rows {e_rows:.2e}), "
          f"attn max {float(ref.max()):.3f}")
    assert e <= tol
    assert e_sum < 1e-4
    assert e_rows <= tol


# Config 4 bounds per precision: CLS rows against the oracle, absolute and relative to the row's values (fp32 and the relative
# bound of single bf16: about 3x the measured value)
C4_BOUNDS = {"bf16x3": (ATTN_TOL, 1e-2), "fp32": (2e-8, 3e-5), "bf16": (ATTN_TOL, 1e-1)}


def _config4(dev, precision):
    model, sd, cfg = _model("vit_small", 8, "sharp", dev, precision)
    tol, tol_rel = C4_BOUNDS[precision]
    slab = synth.synth_tiles(1, 4096, seed=7)[0]
    sweep = SlidingWindowAttention(model, window=384, stride=128)  # auto batch plan, as bench.py's slab_sweep
    maps = sweep(slab.to(dev))
    assert maps.shape == (900, 6, 1, 48, 48)
    if precision == "bf16x3":  # the folded LayerNorm exists for the split-bf16 kernels only (engine.hip: can_fold)
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
    ref = _oracle("vit_small", 8, "sharp", "config4")
    e = float((maps[pick, :, 0].cpu() - ref).abs().max())
    # relative check too: CLS rows over 2304 keys are ~4e-4 each, so 1e-3 absolute alone would not see much
    e_rel = float(((maps[pick, :, 0].cpu() - ref).abs() / ref).max())
    print(f"\n[config 4, {precision}] CLS-row L_inf on windows {pick}: {e:.2e} (row max {float(ref.max()):.4f}), relative {e_rel:.2e}")
    assert e <= tol
    assert e_rel < tol_rel
    assert float((maps.sum((-1, -2)) - 1).abs().max()) < 1e-2  # CLS row minus its own CLS column: close to 1


def test_config4_slab_sweep_sampled_windows(dev):
    _config4(dev, "bf16x3")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_config4_slab_sweep_sampled_windows_in(dev, precision):
    _config4(dev, precision)


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


@pytest.mark.parametrize("precision,tol", [("bf16x3", 1e-3), ("fp32", 2e-4), ("bf16", 5e-2)])
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
