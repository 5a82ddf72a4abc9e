"""Stochastic depth on the ViT training path (model.py::_EncoderTrain, kernels_drop_path.hip): outputs and every gradient of
SimMIM (MIM loss and x_rec), of VisionTransformerForFinetune and of a DINO student (MultiCropWrapper, two crop sizes: two draws
per step) against a float64 twin (tests/drop_path_ref.py) whose scale tables are redrawn from the seed the device forward used;
exact checks with draw_drop_path_scales replaced; frozen blocks, accumulation, eval mode. Needs an MI355X.

Encoder: D = 128, 2 heads of 64, depth 3, patch 8, 64^2 tiles (N = 65), batch 4, drop_path_rate 0.5: rates 0 / 0.25 / 0.5, so an
unscaled block, a scaled site followed by a scaled site, and the final norm behind a scaled branch. Weights: synth "sharp".
Error measure: max |g - g64| / max |g64| per tensor; limits of tests/test_mim_train_gpu.py: gradients fp32 1e-4, bf16x3 1e-3,
bf16 5e-2; forward 2e-5, 2e-4, 5e-2."""
import functools
from functools import partial

import pytest
import torch
import torch.nn as nn

from oracle import vit_oracle as O
from tests import dino_ref as DR
from tests import drop_path_ref as R
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd import synth
from vit_ocm_wmsegmentation_amd.dino import utils as DU
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as V

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-4, "bf16x3": 1e-3, "bf16": 5e-2}
FWD_TOL = {"fp32": 2e-5, "bf16x3": 2e-4, "bf16": 5e-2}
PRECISIONS = ["fp32", "bf16x3", "bf16"]
DIM, HEADS, DEPTH, PATCH, SIDE, LOCAL, BATCH, RATE, SEED = 128, 2, 3, 8, 64, 32, 4, 0.5, 61
LOSS_BIAS_SHIFT = 10.0  # as tests/test_mim_train_gpu.py: no |x - x_rec| near zero, so the L1 signs are stable
HEAD = dict(in_dim=DIM, out_dim=96, hidden_dim=128, bottleneck_dim=64)
KW = dict(patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, mlp_ratio=4, qkv_bias=True,
          norm_layer=partial(nn.LayerNorm, eps=1e-6))
MAP_KW = dict(KW, img_size=[SIDE], interpolate_encoding=True)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _map_inputs():
    sd = synth.synth_state_dict(DIM, DEPTH, PATCH, seed=SEED, variant="sharp", img_size=224)
    wp = synth.synth_wrapper_params(DIM, PATCH, 3, seed=SEED)
    x = synth.synth_tiles(BATCH, SIDE, seed=SEED + 100)
    mask = synth.synth_patch_mask(BATCH, SIDE // PATCH, seed=SEED)
    return sd, wp, x, mask


@functools.lru_cache(maxsize=None)
def _dino_inputs():
    """Two 64^2 and two 32^2 crops of a batch of 2: four images per resolution group."""
    sd = synth.synth_state_dict(DIM, DEPTH, PATCH, seed=SEED + 1, variant="sharp", img_size=SIDE)
    head_sd = DR.fill_head(DR.TwinHead(**HEAD), seed=SEED + 10, g_spread=0.1)
    crops = [synth.synth_tiles(BATCH // 2, SIDE, seed=300 + i) for i in range(2)]
    crops += [synth.synth_tiles(BATCH // 2, LOCAL, seed=310 + i) for i in range(2)]
    return sd, head_sd, crops


def _upstream(shape, seed=5):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _finetune(dev, precision="bf16x3", rate=RATE, sd=None, depth=DEPTH):
    enc = M.VisionTransformerForFinetune(**dict(MAP_KW, depth=depth), drop_path_rate=rate)
    assert not enc.load_state_dict(sd or _map_inputs()[0], strict=True).missing_keys
    enc.set_precision(precision)
    return enc.enable_finetune().to(dev).train()


def _mim(dev, precision, rate=RATE):
    sd, wp, _, _ = _map_inputs()
    enc = M.VisionTransformerForSimMIM(**MAP_KW, drop_path_rate=rate)
    assert not enc.load_state_dict(dict(sd, mask_token=wp["mask_token"]), strict=True).missing_keys
    mim = M.MIM(enc, PATCH)
    mim.decoder[0].weight.data.copy_(wp["decoder.weight"])
    mim.decoder[0].bias.data.copy_(wp["decoder.bias"])
    enc.set_precision(precision)
    return mim.to(dev).train()


def _student(dev, precision, rate=RATE):
    sd, head_sd, _ = _dino_inputs()
    bb = V.VisionTransformer(img_size=[SIDE], drop_path_rate=rate, **KW)
    assert not bb.load_state_dict(sd, strict=True).missing_keys
    bb.set_precision(precision)
    head = V.DINOHead(**HEAD)
    head.load_state_dict(head_sd, strict=True)
    head.precision = precision
    return DU.MultiCropWrapper(bb.enable_training(), head).to(dev).train()


# ---- the scale tables the device forward draws, redrawn from the same seed ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drawn(batches):
    """(seed, [tables of draw 0, tables of draw 1, ...]) for a step that calls the encoder once per entry of `batches`: the first
    seed from 0 up for which, in some scaled branch, one image is dropped and one is kept. torch.manual_seed(seed) in front of the
    device forward then makes it draw these tables: both run draw_drop_path_scales on the device generator in the same order."""
    dev = torch.device("cuda:0")
    probe = V.VisionTransformer(img_size=[SIDE], drop_path_rate=RATE, **KW)
    for seed in range(16):
        torch.manual_seed(seed)
        draws = [[None if s is None else s.cpu() for s in V.draw_drop_path_scales(probe, b, dev)] for b in batches]
        if all(any(s is not None and bool((s == 0).any()) and bool((s > 0).any()) for s in tables) for tables in draws):
            return seed, draws
    raise AssertionError("no seed below 16 drops one image and keeps another in a scaled branch")


def _check_tables(tables):
    """Rates 0 / 0.25 / 0.5: block 0 unscaled, blocks 1 and 2 scaled by 0 or 1 / keep; a dropped and a kept image in some branch."""
    assert tables[0] is None and tables[1] is None and all(t is not None for t in tables[2:])
    for j, t in enumerate(tables[2:], start=2):
        keep = 1 - (0.25 if j < 4 else 0.5)
        assert all(v in (0.0, float(torch.tensor(1.0) / keep)) for v in t.tolist())
    assert any(bool((t == 0).any()) and bool((t > 0).any()) for t in tables[2:])


def _check_grads(named, ref, tol, what):
    errs = {n: R.rel(p.grad, ref[n]) for n, p in named if ref.get(n) is not None}
    missing = [n for n, p in named if p.grad is None and ref.get(n) is not None]
    assert not missing, missing
    worst = max(errs, key=errs.get)
    print(f"GPUTEST drop-path {what}: worst gradient {worst} {errs[worst]:.3e} (limit {tol:.0e})")
    assert errs[worst] <= tol, f"{what}: {worst}: {errs[worst]:.3e} > {tol:.0e}"


# ---- (a) SimMIM -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mim_reference(kind):
    sd, wp, x, mask = _map_inputs()
    _, (tables,) = _drawn((BATCH,))
    prm = {"encoder." + k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    prm["encoder.mask_token"] = wp["mask_token"].double().clone().requires_grad_(True)
    prm["decoder.0.weight"] = wp["decoder.weight"].double().clone().requires_grad_(True)
    prm["decoder.0.bias"] = (wp["decoder.bias"].double() + (LOSS_BIAS_SHIFT if kind == "loss" else 0.0)).requires_grad_(True)
    esd = {k[len("encoder."):]: v for k, v in prm.items() if k.startswith("encoder.") and k != "encoder.mask_token"}
    loss, rec = R.mim_forward(esd, O.make_cfg(esd, PATCH, HEADS), x.double(), mask, SIDE, prm["encoder.mask_token"],
                              prm["decoder.0.weight"], prm["decoder.0.bias"], PATCH, tables)
    if kind == "rec":
        rec.backward(_upstream(rec.shape))
    else:
        loss.backward()
    return rec.detach(), float(loss.detach()), {k: v.grad for k, v in prm.items()}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["rec", "loss"])
def test_mim_matches_float64(dev, kind, precision):
    _, _, x, mask = _map_inputs()
    seed, (tables,) = _drawn((BATCH,))
    _check_tables(tables)
    rec64, loss64, ref = _mim_reference(kind)
    mim = _mim(dev, precision)
    if kind == "loss":
        with torch.no_grad():
            mim.decoder[0].bias += LOSS_BIAS_SHIFT
    torch.manual_seed(seed)
    loss, rec, pm = mim(x.to(dev), mask)
    assert rec.grad_fn is not None and loss.grad_fn is not None
    e_rec = R.rel(rec, rec64)
    print(f"GPUTEST drop-path mim {kind} {precision}: x_rec {e_rec:.3e} (limit {FWD_TOL[precision]:.0e})")
    assert e_rec <= FWD_TOL[precision]
    if kind == "rec":
        rec.backward(_upstream(rec.shape).to(device=dev, dtype=torch.float32))
    else:
        bound = FWD_TOL[precision] * float(rec64.abs().max())
        gap = float((x.double() - rec64).abs()[pm.cpu().expand_as(rec64).bool()].min())
        assert gap > bound, f"an L1 sign is within the forward error ({gap:.2e} <= {bound:.2e})"
        assert abs(float(loss.detach()) - loss64) <= FWD_TOL[precision] * max(1.0, abs(loss64))
        loss.backward()
    _check_grads(list(mim.named_parameters()), ref, TOL[precision], f"mim {kind} {precision}")


# ---- (b) fine-tuning ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _finetune_reference():
    sd, _, x, _ = _map_inputs()
    _, (tables,) = _drawn((BATCH,))
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    z = R.encoder_fmap(prm, O.make_cfg(prm, PATCH, HEADS), x.double(), SIDE, tables)
    z.backward(_upstream(z.shape))
    return z.detach(), {k: v.grad for k, v in prm.items()}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_finetune_matches_float64(dev, precision):
    seed, _ = _drawn((BATCH,))
    z64, ref = _finetune_reference()
    enc = _finetune(dev, precision)
    torch.manual_seed(seed)
    z = enc(_map_inputs()[2].to(dev))
    assert z.grad_fn is not None and z.shape == z64.shape
    e = R.rel(z, z64)
    print(f"GPUTEST drop-path finetune {precision}: map {e:.3e} (limit {FWD_TOL[precision]:.0e})")
    assert e <= FWD_TOL[precision]
    z.backward(_upstream(z.shape).to(device=dev, dtype=torch.float32))
    _check_grads(list(enc.named_parameters()), ref, TOL[precision], f"finetune {precision}")


# ---- (c) a DINO student: two resolution groups, two draws per step ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dino_reference():
    sd, head_sd, crops = _dino_inputs()
    _, (t_global, t_local) = _drawn((BATCH, BATCH))
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    cfg = O.make_cfg(prm, PATCH, HEADS)
    head = DR.TwinHead(**HEAD)
    head.load_state_dict(head_sd)
    head = head.double()
    rows = [R.encoder_tokens(prm, cfg, torch.cat([c.double() for c in group]), tables)[:, 0]
            for group, tables in ((crops[:2], t_global), (crops[2:], t_local))]
    out = head(torch.cat(rows))
    out.backward(_upstream(out.shape))
    grads = {"backbone." + k: v.grad for k, v in prm.items()}
    grads.update({"head." + n: p.grad for n, p in head.named_parameters() if p.grad is not None})
    return out.detach(), grads


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dino_student_matches_float64(dev, precision):
    seed, (t_global, t_local) = _drawn((BATCH, BATCH))
    _check_tables(t_global)
    assert any(not torch.equal(a, b) for a, b in zip(t_global[2:], t_local[2:]))  # the second group drew its own tables
    out64, ref = _dino_reference()
    student = _student(dev, precision)
    torch.manual_seed(seed)
    out = student([c.to(dev) for c in _dino_inputs()[2]])
    assert out.grad_fn is not None and out.shape == out64.shape
    e = R.rel(out, out64)
    print(f"GPUTEST drop-path dino {precision}: logits {e:.3e} (limit {FWD_TOL[precision]:.0e})")
    assert e <= FWD_TOL[precision]
    out.backward(_upstream(out.shape).to(device=dev, dtype=torch.float32))
    _check_grads(list(student.named_parameters()), ref, TOL[precision], f"dino {precision}")


# ---- (d) exact checks with draw_drop_path_scales replaced ----------------------------------------------------------------------------
def _fixed(tables):
    """A draw_drop_path_scales that returns `tables` (a list of None / lists of floats) as device tensors."""
    def draw(model, batch, device):
        return [None if t is None else torch.tensor(t, dtype=torch.float32, device=device) for t in tables]
    return draw


def _run_map(enc, dev, seed=5):
    x = _map_inputs()[2].to(dev)
    z = enc(x)
    z.backward(_upstream(z.shape, seed).to(device=dev, dtype=torch.float32))
    torch.cuda.synchronize()
    return z.detach(), {n: p.grad for n, p in enc.named_parameters()}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_block_with_zero_tables_is_skipped_exactly(dev, monkeypatch, precision):
    """Block 1's two tables all zero: the tokens pass it unchanged — the output has the bits of the same model without that
    block — and every parameter of the block gets a gradient of exactly zero."""
    zeros = [0.0] * BATCH
    monkeypatch.setattr(V, "draw_drop_path_scales", _fixed([None, None, zeros, zeros, None, None]))
    z, grads = _run_map(_finetune(dev, precision), dev)
    for n, g in grads.items():
        if n.startswith("blocks.1."):
            assert g is not None and not bool(g.any()), n
        else:
            assert g is not None and bool(g.any()), n
    sd = _map_inputs()[0]
    sd2 = {k: v for k, v in sd.items() if not k.startswith("blocks.1.")}
    sd2 = {k.replace("blocks.2.", "blocks.1."): v for k, v in sd2.items()}
    monkeypatch.setattr(V, "draw_drop_path_scales", _fixed([None] * 4))
    z2, grads2 = _run_map(_finetune(dev, precision, sd=sd2, depth=2), dev)
    assert torch.equal(z, z2)
    for n, g in grads2.items():  # and the blocks around it see the same gradients
        assert torch.equal(g, grads[n.replace("blocks.1.", "blocks.2.")]), n


def test_tables_of_ones_agree_with_rate_zero(dev, monkeypatch):
    """All tables 1.0 against the drop_path_rate = 0 model in fp32 arithmetic: the same sums in another order of additions (the
    GEMM's residual epilogue adds resid + acc + bias, the drop-path kernel x + (acc + bias)): fp32 round-off, relative 1e-6."""
    z0, g0 = _run_map(_finetune(dev, "fp32", rate=0.0), dev)
    monkeypatch.setattr(V, "draw_drop_path_scales", _fixed([[1.0] * BATCH] * (2 * DEPTH)))
    z1, g1 = _run_map(_finetune(dev, "fp32"), dev)
    same = torch.equal(z0, z1) and all(torch.equal(g0[n], g1[n]) for n in g0)
    errs = {n: R.rel(g1[n], g0[n]) for n in g0}
    worst = max(errs, key=errs.get)
    print(f"GPUTEST drop-path tables of ones vs rate 0 (fp32): bit-equal {same}, map {R.rel(z1, z0):.3e}, worst gradient {worst} "
          f"{errs[worst]:.3e}")
    assert R.rel(z1, z0) <= 1e-6
    assert errs[worst] <= 1e-6, f"{worst}: {errs[worst]:.3e}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_image_dropped_everywhere_keeps_its_prepared_tokens(dev, monkeypatch, precision):
    """Image 2 dropped in all six branches: its rows of the output are norm(prepare_tokens) of that image, bit for bit."""
    table = [2.0, 2.0, 0.0, 2.0]
    monkeypatch.setattr(V, "draw_drop_path_scales", _fixed([table] * (2 * DEPTH)))
    enc = _finetune(dev, precision)
    x = _map_inputs()[2].to(dev)
    z = enc(x).detach()
    enc.eval()
    with torch.no_grad():
        want = M._tokens_to_fmap(enc.norm(enc.prepare_tokens(x)))
    assert torch.equal(z[2], want[2])
    assert not torch.equal(z[1], want[1])


# ---- (e) frozen blocks, accumulation, eval mode, the refusals ---------------------------------------------------------------------------
def test_frozen_lower_blocks_keep_the_remaining_gradients_bits(dev):
    seed, _ = _drawn((BATCH,))
    torch.manual_seed(seed)
    z_full, full = _run_map(_finetune(dev), dev)
    enc = _finetune(dev)
    below = ("cls_token", "pos_embed", "patch_embed.", "blocks.0.")
    for n, p in enc.named_parameters():
        if n.startswith(below):
            p.requires_grad_(False)
    assert M._first_block_to_train(enc, M._encoder_params(enc)) == 1
    torch.manual_seed(seed)
    z, part = _run_map(enc, dev)
    assert torch.equal(z, z_full)
    for n, g in part.items():
        if n.startswith(below):
            assert g is None, n
        else:
            assert torch.equal(g, full[n]), n


def test_two_backwards_accumulate(dev):
    seed, _ = _drawn((BATCH,))
    enc = _finetune(dev)
    torch.manual_seed(seed)
    _, first = _run_map(enc, dev)
    first = {n: g.clone() for n, g in first.items()}
    torch.manual_seed(seed)
    _run_map(enc, dev)
    for n, p in enc.named_parameters():
        assert torch.equal(p.grad, first[n] + first[n]), n


def test_eval_mode_ignores_the_rate_and_no_grad_training_is_refused(dev):
    x = _map_inputs()[2].to(dev)
    a, b = _finetune(dev, rate=0.1).eval(), _finetune(dev, rate=0.0).eval()
    assert torch.equal(a(x), b(x))
    a.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"\.eval\(\)"):
        a(x)
    a.enable_finetune(False)
    with pytest.raises(NotImplementedError, match="enable_finetune"):
        a(x)
    for p in a.enable_finetune().parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="trainable parameter"):
        a(x)
