"""Dropout on the ViT training path (model.py::_EncoderTrain, kernels_dropout.hip): outputs and every gradient of SimMIM (MIM loss
and x_rec), of VisionTransformerForFinetune and of a DINO student (MultiCropWrapper, two crop sizes: two draws per step) against a
float64 twin (tests/dropout_ref.py) whose masks come from the numpy restatement of csrc/philox.h and the seeds the device forward
drew, redrawn from the same torch seed; exact checks of the opt-in, reproducibility, precision independence of the draw, eval
mode, accumulation and frozen blocks. Needs an MI355X.

Encoder, inputs and limits are tests/test_drop_path_train_gpu.py's: D = 128, 2 heads of 64, depth 3, patch 8, 64^2 tiles (N = 65),
batch 4, synth "sharp". Configurations: (a) drop_rate 0.25 alone; (b) drop_rate 0.25 with drop_path_rate 0.5 (rates 0 / 0.25 /
0.5: an unscaled block, a dropped-and-scaled site behind a dropped-and-scaled site, the final norm behind such a branch). The twin
sees the same masks, so the error class is the drop-path test's: gradients fp32 1e-4, bf16x3 1e-3, bf16 5e-2 of each tensor's
maximum; forward 2e-5, 2e-4, 5e-2."""
import functools

import pytest
import torch

from oracle import vit_oracle as O
from tests import dino_ref as DR
from tests import dropout_ref as R
from tests import test_drop_path_train_gpu as DP
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.dino import utils as DU
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as V

pytestmark = pytest.mark.gpu

TOL, FWD_TOL, PRECISIONS = DP.TOL, DP.FWD_TOL, DP.PRECISIONS
DEPTH, PATCH, HEADS, SIDE, BATCH = DP.DEPTH, DP.PATCH, DP.HEADS, DP.SIDE, DP.BATCH
DROP = 0.25
CONFIGS = {"dropout": 0.0, "dropout+droppath": 0.5}  # name -> drop_path_rate
NSITES = 1 + 3 * DEPTH


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


# ---- models -------------------------------------------------------------------------------------------------------------------------
def _finetune(dev, precision="bf16x3", drop=DROP, path=0.0, enable=True):
    enc = M.VisionTransformerForFinetune(**DP.MAP_KW, drop_rate=drop, drop_path_rate=path)
    assert not enc.load_state_dict(DP._map_inputs()[0], strict=True).missing_keys
    enc.set_precision(precision)
    return enc.enable_finetune().enable_dropout(enable).to(dev).train()


def _mim(dev, precision, path):
    sd, wp, _, _ = DP._map_inputs()
    enc = M.VisionTransformerForSimMIM(**DP.MAP_KW, drop_rate=DROP, drop_path_rate=path)
    assert not enc.load_state_dict(dict(sd, mask_token=wp["mask_token"]), strict=True).missing_keys
    mim = M.MIM(enc.enable_dropout(), PATCH)
    mim.decoder[0].weight.data.copy_(wp["decoder.weight"])
    mim.decoder[0].bias.data.copy_(wp["decoder.bias"])
    enc.set_precision(precision)
    return mim.to(dev).train()


def _student(dev, precision, path):
    sd, head_sd, _ = DP._dino_inputs()
    bb = V.VisionTransformer(img_size=[SIDE], drop_rate=DROP, drop_path_rate=path, **DP.KW)
    assert not bb.load_state_dict(sd, strict=True).missing_keys
    bb.set_precision(precision)
    head = V.DINOHead(**DP.HEAD)
    head.load_state_dict(head_sd, strict=True)
    head.precision = precision
    return DU.MultiCropWrapper(bb.enable_training().enable_dropout(), head).to(dev).train()


# ---- what the device forward draws, redrawn from the same torch seed ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drawn(config, ncalls):
    """(torch seed, [(dropout seeds, drop-path tables) per encoder call]) of a step that calls the encoder `ncalls` times on BATCH
    images: the first seed from 0 up for which, with drop-path, some scaled branch of every call drops one image and keeps
    another. torch.manual_seed(seed) in front of the device forward then makes it draw the same: both sides call
    draw_dropout_seeds, then draw_drop_path_scales, on the device generator in the same order."""
    dev = torch.device("cuda:0")
    path = CONFIGS[config]
    probe = V.VisionTransformer(img_size=[SIDE], drop_rate=DROP, drop_path_rate=path, **DP.KW)
    for seed in range(16):
        torch.manual_seed(seed)
        draws = []
        for _ in range(ncalls):
            seeds = V.draw_dropout_seeds(probe, dev).cpu()
            tables = [None if s is None else s.cpu() for s in V.draw_drop_path_scales(probe, BATCH, dev)]
            draws.append((seeds, tables))
        if path == 0 or all(any(s is not None and bool((s == 0).any()) and bool((s > 0).any()) for s in t) for _, t in draws):
            return seed, draws
    raise AssertionError("no seed below 16 drops one image and keeps another in a scaled branch")


def _factors(seeds):
    assert seeds.shape == (NSITES,) and bool((seeds >= 0).all()) and bool((seeds < 2 ** 62).all())
    return R.SiteFactors(seeds.tolist(), R.site_rates(DEPTH, DROP))


def _check_draw(config, tables):
    if CONFIGS[config]:
        DP._check_tables(tables)
    else:
        assert tables == [None] * (2 * DEPTH)


def _check_grads(named, ref, tol, what):
    errs = {n: R.rel(p.grad, ref[n]) for n, p in named if ref.get(n) is not None}
    missing = [n for n, p in named if p.grad is None and ref.get(n) is not None]
    assert not missing, missing
    worst = max(errs, key=errs.get)
    print(f"GPUTEST dropout {what}: worst gradient {worst} {errs[worst]:.3e} (limit {tol:.0e})")
    assert errs[worst] <= tol, f"{what}: {worst}: {errs[worst]:.3e} > {tol:.0e}"


# ---- (a) SimMIM -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mim_reference(config, kind):
    sd, wp, x, mask = DP._map_inputs()
    _, ((seeds, tables),) = _drawn(config, 1)
    prm = {"encoder." + k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    prm["encoder.mask_token"] = wp["mask_token"].double().clone().requires_grad_(True)
    prm["decoder.0.weight"] = wp["decoder.weight"].double().clone().requires_grad_(True)
    prm["decoder.0.bias"] = (wp["decoder.bias"].double() + (DP.LOSS_BIAS_SHIFT if kind == "loss" else 0.0)).requires_grad_(True)
    esd = {k[len("encoder."):]: v for k, v in prm.items() if k.startswith("encoder.") and k != "encoder.mask_token"}
    loss, rec = R.mim_forward(esd, O.make_cfg(esd, PATCH, HEADS), x.double(), mask, SIDE, prm["encoder.mask_token"],
                              prm["decoder.0.weight"], prm["decoder.0.bias"], PATCH, tables, _factors(seeds))
    if kind == "rec":
        rec.backward(DP._upstream(rec.shape))
    else:
        loss.backward()
    return rec.detach(), float(loss.detach()), {k: v.grad for k, v in prm.items()}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["rec", "loss"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_mim_matches_float64(dev, config, kind, precision):
    _, _, x, mask = DP._map_inputs()
    seed, ((_, tables),) = _drawn(config, 1)
    _check_draw(config, tables)
    rec64, loss64, ref = _mim_reference(config, kind)
    mim = _mim(dev, precision, CONFIGS[config])
    if kind == "loss":
        with torch.no_grad():
            mim.decoder[0].bias += DP.LOSS_BIAS_SHIFT
    torch.manual_seed(seed)
    loss, rec, pm = mim(x.to(dev), mask)
    assert rec.grad_fn is not None and loss.grad_fn is not None
    e_rec = R.rel(rec, rec64)
    print(f"GPUTEST dropout mim {config} {kind} {precision}: x_rec {e_rec:.3e} (limit {FWD_TOL[precision]:.0e})")
    assert e_rec <= FWD_TOL[precision]
    if kind == "rec":
        rec.backward(DP._upstream(rec.shape).to(device=dev, dtype=torch.float32))
    else:
        bound = FWD_TOL[precision] * float(rec64.abs().max())
        gap = float((x.double() - rec64).abs()[pm.cpu().expand_as(rec64).bool()].min())
        assert gap > bound, f"an L1 sign is within the forward error ({gap:.2e} <= {bound:.2e})"
        assert abs(float(loss.detach()) - loss64) <= FWD_TOL[precision] * max(1.0, abs(loss64))
        loss.backward()
    _check_grads(list(mim.named_parameters()), ref, TOL[precision], f"mim {config} {kind} {precision}")


# ---- (b) fine-tuning ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _finetune_reference(config):
    sd, _, x, _ = DP._map_inputs()
    _, ((seeds, tables),) = _drawn(config, 1)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    z = R.encoder_fmap(prm, O.make_cfg(prm, PATCH, HEADS), x.double(), SIDE, tables, _factors(seeds))
    z.backward(DP._upstream(z.shape))
    return z.detach(), {k: v.grad for k, v in prm.items()}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_finetune_matches_float64(dev, config, precision):
    seed, _ = _drawn(config, 1)
    z64, ref = _finetune_reference(config)
    enc = _finetune(dev, precision, path=CONFIGS[config])
    torch.manual_seed(seed)
    z = enc(DP._map_inputs()[2].to(dev))
    assert z.grad_fn is not None and z.shape == z64.shape
    e = R.rel(z, z64)
    print(f"GPUTEST dropout finetune {config} {precision}: map {e:.3e} (limit {FWD_TOL[precision]:.0e})")
    assert e <= FWD_TOL[precision]
    z.backward(DP._upstream(z.shape).to(device=dev, dtype=torch.float32))
    _check_grads(list(enc.named_parameters()), ref, TOL[precision], f"finetune {config} {precision}")


# ---- (c) a DINO student: two resolution groups, two draws per step ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dino_reference(config):
    sd, head_sd, crops = DP._dino_inputs()
    _, (d_global, d_local) = _drawn(config, 2)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    cfg = O.make_cfg(prm, PATCH, HEADS)
    head = DR.TwinHead(**DP.HEAD)
    head.load_state_dict(head_sd)
    head = head.double()
    rows = [R.encoder_tokens(prm, cfg, torch.cat([c.double() for c in group]), tables, _factors(seeds))[:, 0]
            for group, (seeds, tables) in ((crops[:2], d_global), (crops[2:], d_local))]
    out = head(torch.cat(rows))
    out.backward(DP._upstream(out.shape))
    grads = {"backbone." + k: v.grad for k, v in prm.items()}
    grads.update({"head." + n: p.grad for n, p in head.named_parameters() if p.grad is not None})
    return out.detach(), grads


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_dino_student_matches_float64(dev, config, precision):
    seed, ((s_global, _), (s_local, _)) = _drawn(config, 2)
    assert not torch.equal(s_global, s_local)  # the second resolution group drew its own seeds
    out64, ref = _dino_reference(config)
    student = _student(dev, precision, CONFIGS[config])
    torch.manual_seed(seed)
    out = student([c.to(dev) for c in DP._dino_inputs()[2]])
    assert out.grad_fn is not None and out.shape == out64.shape
    e = R.rel(out, out64)
    print(f"GPUTEST dropout dino {config} {precision}: logits {e:.3e} (limit {FWD_TOL[precision]:.0e})")
    assert e <= FWD_TOL[precision]
    out.backward(DP._upstream(out.shape).to(device=dev, dtype=torch.float32))
    _check_grads(list(student.named_parameters()), ref, TOL[precision], f"dino {config} {precision}")


# ---- (d) exact checks ------------------------------------------------------------------------------------------------------------------
def _run_map(enc, dev, seed=None, upstream=5):
    if seed is not None:
        torch.manual_seed(seed)
    x = DP._map_inputs()[2].to(dev)
    z = enc(x)
    z.backward(DP._upstream(z.shape, upstream).to(device=dev, dtype=torch.float32))
    torch.cuda.synchronize()
    return z.detach(), {n: p.grad for n, p in enc.named_parameters()}


def _same(a, b):
    (za, ga), (zb, gb) = a, b
    return torch.equal(za, zb) and all((ga[n] is None and gb[n] is None) or torch.equal(ga[n], gb[n]) for n in ga)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rate_zero_with_the_flag_on_equals_the_flag_off(dev, precision):
    """drop_rate 0 with drop_path_rate 0.5: the flag changes no launch, so outputs and gradients keep their bits, and the
    generator is used alike (no seeds are drawn at rate 0)."""
    seed, _ = DP._drawn((BATCH,))
    off = _run_map(_finetune(dev, precision, drop=0.0, path=0.5, enable=False), dev, seed)
    after_off = torch.rand(3, device=dev)
    on = _run_map(_finetune(dev, precision, drop=0.0, path=0.5, enable=True), dev, seed)
    after_on = torch.rand(3, device=dev)
    assert _same(on, off) and torch.equal(after_on, after_off)


def test_the_same_seed_gives_the_same_bits_and_another_seed_other_masks(dev, monkeypatch):
    drawn = []
    draw = V.draw_dropout_seeds

    def recording(model, device):
        drawn.append(draw(model, device))
        return drawn[-1]

    monkeypatch.setattr(V, "draw_dropout_seeds", recording)
    enc = _finetune(dev, path=0.5)
    a = _run_map(enc, dev, 3)
    a = (a[0], {n: g.clone() for n, g in a[1].items()})
    enc.zero_grad(set_to_none=True)
    b = _run_map(enc, dev, 3)
    b = (b[0], {n: g.clone() for n, g in b[1].items()})
    enc.zero_grad(set_to_none=True)
    c = _run_map(enc, dev, 4)
    assert _same(a, b) and torch.equal(drawn[0], drawn[1])
    assert not torch.equal(drawn[0], drawn[2]) and not torch.equal(a[0], c[0])
    thresh = R.threshold(DROP)[0]
    masks = [R.keep_mask(int(s[0]), BATCH * 65 * 128, thresh) for s in (drawn[0].cpu(), drawn[2].cpu())]
    assert (masks[0] != masks[1]).any()


def test_the_three_precisions_draw_the_same_masks(dev, monkeypatch):
    drawn = {}
    draw = V.draw_dropout_seeds
    for precision in PRECISIONS:
        def recording(model, device, precision=precision):
            drawn[precision] = draw(model, device)
            return drawn[precision]

        monkeypatch.setattr(V, "draw_dropout_seeds", recording)
        torch.manual_seed(9)
        _finetune(dev, precision)(DP._map_inputs()[2].to(dev))
    torch.cuda.synchronize()
    assert torch.equal(drawn["fp32"], drawn["bf16"]) and torch.equal(drawn["fp32"], drawn["bf16x3"])
    assert drawn["fp32"].dtype == torch.int64 and drawn["fp32"].shape == (NSITES,) and drawn["fp32"].device.type == "cuda"


def test_pos_drop_alone_zeroes_what_the_mask_says(dev, monkeypatch):
    """Only pos_drop above 0, rate 0.5, and blocks made the identity (zero proj / fc2 weights and biases): the encoder output is
    norm(dropped tokens), so the final norm of the tokens masked by the numpy mask has to come out, bit for bit."""
    enc = _finetune(dev, "fp32", drop=0.0)
    enc.pos_drop.p = 0.5
    with torch.no_grad():
        for blk in enc.blocks:
            for lin in (blk.attn.proj, blk.mlp.fc2):
                lin.weight.zero_()
                lin.bias.zero_()
    seeds = torch.tensor([2 ** 40 + 7] + [0] * (NSITES - 1), dtype=torch.int64, device=dev)
    monkeypatch.setattr(V, "draw_dropout_seeds", lambda model, device: seeds)
    x = DP._map_inputs()[2].to(dev)
    z = enc(x).detach()
    enc.eval()
    with torch.no_grad():
        t = enc.prepare_tokens(x)
        f = torch.from_numpy(R.factors(2 ** 40 + 7, t.numel(), 0.5)).reshape(t.shape).to(dev)
        want = M._tokens_to_fmap(enc.norm(t * f))
    assert torch.equal(z, want)


# ---- (e) eval mode, accumulation, frozen blocks, the refusals ---------------------------------------------------------------------------
def test_eval_mode_equals_rate_zero_and_no_grad_training_is_refused(dev):
    x = DP._map_inputs()[2].to(dev)
    a, b = _finetune(dev, drop=DROP).eval(), _finetune(dev, drop=0.0, enable=False).eval()
    assert torch.equal(a(x), b(x))
    a.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"\.eval\(\)"):
        a(x)
    a.enable_finetune(False)
    with pytest.raises(NotImplementedError, match="enable_finetune"):
        a(x)
    a.enable_finetune().enable_dropout(False)
    with pytest.raises(NotImplementedError, match=r"enable_dropout\(\)"):
        a(x)
    a.enable_dropout()
    a.blocks[0].attn.attn_drop.p = 0.1
    with pytest.raises(NotImplementedError, match="attention dropout"):
        a(x)


def test_two_backwards_accumulate(dev):
    enc = _finetune(dev, path=0.5)
    _, first = _run_map(enc, dev, 2)
    first = {n: g.clone() for n, g in first.items()}
    _run_map(enc, dev, 2)
    for n, p in enc.named_parameters():
        assert torch.equal(p.grad, first[n] + first[n]), n


def test_frozen_lower_blocks_keep_the_remaining_gradients_bits(dev):
    z_full, full = _run_map(_finetune(dev, path=0.5), dev, 2)
    enc = _finetune(dev, path=0.5)
    below = ("cls_token", "pos_embed", "patch_embed.", "blocks.0.", "blocks.1.")
    for n, p in enc.named_parameters():
        if n.startswith(below):
            p.requires_grad_(False)
    assert M._first_block_to_train(enc, M._encoder_params(enc)) == 2
    z, part = _run_map(enc, dev, 2)
    assert torch.equal(z, z_full)
    for n, g in part.items():
        if n.startswith(below):
            assert g is None, n
        else:
            assert torch.equal(g, full[n]), n
