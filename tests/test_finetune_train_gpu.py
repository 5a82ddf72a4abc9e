"""Encoder fine-tuning on the HIP path (finetune.py --finetune True): LinearProbing over a trainable, opted-in
VisionTransformerForFinetune, with utils.DiceLoss. Needs an MI355X.

The float64 CPU twin is oracle.vit_oracle.encoder_fmap on requires_grad leaves, a deepcopy(...).double().train() of the decoder
nn.Sequential and the reference's Dice formula. Error measure: max |g - g64| / max |g64| per tensor.
  (a) decoder token gradient alone: test_linear_probing_train_gpu.py's cases, ladder (fp32 2e-5, bf16x3 2e-4, bf16 3e-2) and ReLU
      separation; the twin is fed the product's own tokens.
  (b) end to end: test_mim_train_gpu.py's limits (fp32 1e-4, bf16x3 1e-3, bf16 5e-2); the depth-12 case gets 3 x (the ladder is
      known at depth 4, accumulation over three times as many blocks is at worst linear).
Two-layer decoder end to end: the ReLU sits behind an encoder whose output differs from the twin's, so the thresholds are put in
gaps of the TWIN's normalised conv1 output that are at least MARGIN wide on each side (asserted on the CPU side): 4 x the measured
deviation of the product's normalised y1 from the twin's (Y1_DEVIATION, printed by every run of test_end_to_end). Single bf16
deviates by more than any gap these geometries have: its two-layer end-to-end cases assert finite gradients only."""
import copy
import functools
import gc
from functools import partial

import pytest
import torch
import torch.nn as nn

from oracle import vit_oracle as O
from tests import test_linear_probing_train_gpu as LPT
from tests.golden_cases import WRAPPER_CASES
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd import synth
from vit_ocm_wmsegmentation_amd import utils as U

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-4, "bf16x3": 1e-3, "bf16": 5e-2}  # tests/test_mim_train_gpu.py
FWD_TOL = LPT.TOL  # tests/test_wrappers.py's ladder
GEOMS = {
    "wrap_p8_64": WRAPPER_CASES["wrap_p8_64"],
    "ft384": dict(LPT.FT, batch=2),  # depth 2, N = 2305
    # build_finetune_model's head layout (12 blocks, 6 x 64-wide heads) at 96^2, finetune.py's batch
    "ft96_d12": dict(dim=384, depth=12, heads=6, patch=8, img_size=96, batch=3, seed=51, variant="full"),
    # partial fine-tuning's memory check (no twin): three blocks at 384^2
    "ft384_d3": dict(dim=384, depth=3, heads=6, patch=8, img_size=384, batch=2, seed=52, variant="full"),
}
DEPTH_FACTOR = {"wrap_p8_64": 1, "ft384": 1, "ft96_d12": 3}
# max |y1n - y1n64| of the product's normalised conv1 output (training-mode encoder) per precision, at or above the worst measured
# over the three geometries: fp32 1.7e-5 (ft96_d12), bf16x3 1.15e-4 (ft96_d12; ft384 9.9e-5), bf16 6.4e-2 (ft96_d12)
Y1_DEVIATION = {"fp32": 2.5e-5, "bf16x3": 1.5e-4, "bf16": 7e-2}
MARGIN = {k: 4 * v for k, v in Y1_DEVIATION.items()}
# (geometry, precision) pairs whose widest gaps hold MARGIN (the CPU-side assertion of _separated_bias passes), fixed here: the
# smallest half-gaps are 6.4e-2 (wrap_p8_64), 5.5e-3 (ft384) and 3.3e-2 (ft96_d12) against 1e-4 / 6e-4 / 0.28
LAYER2_CLAIMED = [("wrap_p8_64", "fp32"), ("wrap_p8_64", "bf16x3"), ("ft384", "fp32"), ("ft384", "bf16x3"),
                  ("ft96_d12", "fp32"), ("ft96_d12", "bf16x3")]
LAYER2_FINITE_ONLY = [("wrap_p8_64", "bf16"), ("ft96_d12", "bf16")]


def _inputs(name):
    c = GEOMS[name]
    sd = synth.synth_state_dict(c["dim"], c["depth"], c["patch"], seed=c["seed"], variant=c["variant"], img_size=224)
    x = synth.synth_tiles(c["batch"], c["img_size"], seed=c["seed"] + 100)
    return c, sd, x


def _decoder_state(name, layer_num):
    c = GEOMS[name]
    if layer_num == 2:
        return dict(synth.synth_two_layer_decoder_params(c["dim"], c["patch"], seed=c["seed"]))
    wp1 = synth.synth_wrapper_params(c["dim"], c["patch"], 1, seed=c["seed"])
    return {"0.weight": wp1["decoder.weight"], "0.bias": wp1["decoder.bias"]}


def _decoder_of(lp):
    return lp.two_layer_decoder if lp.layer_num == 2 else lp.one_layer_decoder


def _fresh_decoder(name, layer_num, bn_bias=None):
    c = GEOMS[name]
    feats, s2 = c["dim"], c["patch"] ** 2
    if layer_num == 2:
        dec = nn.Sequential(nn.Conv2d(feats, 4 * s2, kernel_size=3, padding=1), nn.BatchNorm2d(4 * s2), nn.ReLU(inplace=True),
                            nn.Conv2d(4 * s2, s2, kernel_size=3, padding=1), nn.PixelShuffle(c["patch"]))
    else:
        dec = nn.Sequential(nn.Conv2d(feats, s2, kernel_size=1), nn.PixelShuffle(c["patch"]))
    dec.load_state_dict(_decoder_state(name, layer_num), strict=False)
    if bn_bias is not None:
        with torch.no_grad():
            dec[1].bias.copy_(bn_bias)
    return dec


def _model(name, layer_num, precision, dev, separated=True, flag=True):
    """LinearProbing over a fully trainable encoder that has opted in, in training mode, and its input."""
    c, sd, x = _inputs(name)
    enc = M.VisionTransformerForFinetune(patch_size=c["patch"], embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"],
                                         mlp_ratio=4, img_size=[c["img_size"]], qkv_bias=True,
                                         norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)
    assert not enc.load_state_dict(sd, strict=True).missing_keys
    enc.enable_finetune(flag)
    lp = M.LinearProbing(enc, c["patch"], layer_num=layer_num)
    bias = _separated_bias(name)[0] if (layer_num == 2 and separated) else None
    _decoder_of(lp).load_state_dict(_fresh_decoder(name, layer_num, bias).state_dict())
    enc.set_precision(precision)
    return lp.to(dev).train(), x.to(dev)


@functools.lru_cache(maxsize=None)
def _twin_fmap(name):
    c, sd, x = _inputs(name)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        return O.encoder_fmap(sd64, O.make_cfg(sd64, c["patch"], c["heads"]), x.double(), c["img_size"])


def _normalised_y1(dec, fmap):
    conv1, bn = dec[0], dec[1]
    y1 = nn.functional.conv2d(fmap, conv1.weight.double().cpu(), conv1.bias.double().cpu(), padding=1)
    y1 = y1.transpose(0, 1).reshape(y1.shape[1], -1)
    mu, var = y1.mean(1, keepdim=True), y1.var(1, unbiased=False, keepdim=True)
    return (y1 - mu) / torch.sqrt(var + bn.eps)


@functools.lru_cache(maxsize=None)
def _separated_bias(name):
    """LPT._separate_relu on the twin's own map: (BatchNorm bias that puts every channel's ReLU threshold in the middle of the widest
    gap of its normalised values between the 2 % and 98 % quantiles, the smallest half-gap in units of the normalised y1)."""
    dec = _fresh_decoder(name, 2)
    with torch.no_grad():
        xh, _ = _normalised_y1(dec, _twin_fmap(name)).sort(1)
        n = xh.shape[1]
        inner = xh[:, n // 50: n - n // 50]
        gaps = inner[:, 1:] - inner[:, :-1]
        gap, i = gaps.max(1)
        q = inner.gather(1, i[:, None])[:, 0] + gap / 2
        gamma = dec[1].weight.double()
        return (-gamma * q).float(), float((gap / 2).min())


@functools.lru_cache(maxsize=None)
def _reference(name, layer_num):
    """The twin: (out64, loss64, {kind: {lp parameter name: grad64}}, normalised y1 or None, dy1 of the dice backward or None)."""
    c, sd, x = _inputs(name)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    dec = _fresh_decoder(name, layer_num, _separated_bias(name)[0] if layer_num == 2 else None).double().train()
    z = O.encoder_fmap(prm, O.make_cfg(prm, c["patch"], c["heads"]), x.double(), c["img_size"])
    y1_grads = []

    def keep_y1_grad(mod, inp, o):  # conv1's output gradient (mid, M) of every backward, for the conv1-bias bound
        o.register_hook(lambda g: y1_grads.append(g.transpose(0, 1).reshape(g.shape[1], -1)))

    if layer_num == 2:
        dec[0].register_forward_hook(keep_y1_grad)
    out = dec(z)
    loss = LPT.dice_loss(out, LPT._target(x).double())
    prefix = "two_layer_decoder." if layer_num == 2 else "one_layer_decoder."
    leaves = {"encoder." + k: v for k, v in prm.items()}
    leaves.update({prefix + k: v for k, v in dec.named_parameters()})
    grads = {}
    for kind, root, seed in (("dice", loss, None), ("upstream", out, _upstream(out.shape))):
        g = torch.autograd.grad(root, list(leaves.values()), seed, retain_graph=True)
        grads[kind] = dict(zip(leaves, g))
    with torch.no_grad():
        y1n = _normalised_y1(dec, z.detach()) if layer_num == 2 else None
    return out.detach(), float(loss.detach()), grads, y1n, y1_grads


def _upstream(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)


def _rel(a, ref):
    return float((a.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _errors(lp, ref, tol, y1_grad=None):
    """Every parameter of the wrapper: the unused decoder has no gradient, every other one is within tol of the twin's."""
    unused = "one_layer_decoder." if lp.layer_num == 2 else "two_layer_decoder."
    errs = {}
    for n, p in lp.named_parameters():
        if n.startswith(unused):
            assert p.grad is None, n
            continue
        assert p.grad is not None, n
        if n == "two_layer_decoder.0.bias":
            # conv1's bias gradient sum_m dy1 is zero in exact arithmetic (BatchNorm removes the channel mean): what is left is
            # rounding, at most M * tol * max |dy1| (test_linear_probing_train_gpu.py's bound)
            bound = tol * y1_grad[0].numel() * float(y1_grad.abs().max())
            assert float(p.grad.abs().max()) <= bound, f"{n}: {float(p.grad.abs().max()):.3e} > {bound:.3e}"
            continue
        errs[n] = _rel(p.grad, ref[n])
    return errs


def _assert_errors(errs, tol, what):
    worst = max(errs, key=errs.get)
    print(f"GPUTEST finetune {what}: worst gradient {worst} {errs[worst]:.3e} (limit {tol:.0e})")
    assert errs[worst] <= tol, f"{what}: {worst}: {errs[worst]:.3e} > {tol:.0e}"


# ---- (a) the decoder's token gradient alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("layer_num", [1, 2])
@pytest.mark.parametrize("name,batch,precision", LPT.TRAIN_CASES)
def test_decoder_token_gradient(dev, name, batch, layer_num, precision):
    lp, x, fmap = LPT._setup(name, batch, layer_num, precision, dev)  # frozen encoder; fmap: the product's own tokens in float64
    if layer_num == 2:
        LPT._separate_relu(lp, fmap, precision)
    twin = LPT._twin(lp)
    tol = LPT.TOL[precision]
    with torch.no_grad():
        tokens = lp.encoder._encode(x, tokens=True)
    B, N, D = tokens.shape
    y = LPT._target(x)
    for what in ("dice", "random upstream"):
        lp.zero_grad(set_to_none=True)
        twin.zero_grad(set_to_none=True)
        tok = tokens.clone().requires_grad_(True)
        f64 = fmap.clone().requires_grad_(True)
        out, want = M._train_forward(lp, tok), twin(f64)
        assert out.grad_fn is not None and _rel(out, want) <= tol
        if what == "dice":
            U.DiceLoss()(out, y).backward()
            LPT.dice_loss(want, y.double().cpu()).backward()
        else:
            G = _upstream(out.shape)
            out.backward(G.float().to(dev))
            want.backward(G)
        assert tok.grad.shape == tokens.shape and tok.grad.dtype == torch.float32
        assert not bool(tok.grad[:, 0].any()), "the CLS row of the token gradient is not exactly zero"
        want_tok = f64.grad.reshape(B, D, N - 1).transpose(1, 2)  # (B, P, D)
        err = _rel(tok.grad[:, 1:], want_tok)
        print(f"GPUTEST finetune token gradient {name} b{batch} layer {layer_num} {precision} {what}: {err:.3e}")
        assert err <= tol, f"{what}: token gradient {err:.3e} > {tol:.0e}"
        LPT._check_grads(lp, twin, precision, what)  # the parameter gradients of the same backward are what they were


# ---- (b) end to end -------------------------------------------------------------------------------------------------------
def _end_to_end(dev, name, precision, layer_num, claimed=True):
    lp, x = _model(name, layer_num, precision, dev)
    out64, loss64, ref, y1n64, y1_grads = _reference(name, layer_num)
    tol = TOL[precision] * DEPTH_FACTOR[name]
    y = LPT._target(x)
    out = lp(x)
    assert out.grad_fn is not None and out.shape == out64.shape
    if layer_num == 2:
        with torch.no_grad():  # how far the product's normalised y1 is from the twin's: what MARGIN is four times of
            fmap = lp.encoder.train()(x)
            dev_y1 = float((_normalised_y1(copy.deepcopy(lp.two_layer_decoder).cpu().double(), fmap.double().cpu()) - y1n64)
                           .abs().max())
        print(f"GPUTEST finetune y1 deviation {name} {precision}: {dev_y1:.3e} (margin {MARGIN[precision]:.1e}, "
              f"half-gap {_separated_bias(name)[1]:.3e})")
    if not claimed:
        U.DiceLoss()(out, y).backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in lp.parameters() if p.grad is not None)
        assert bool(torch.isfinite(out).all()) and lp.encoder.pos_embed.grad is not None
        return
    if layer_num == 2:
        assert _separated_bias(name)[1] >= MARGIN[precision], "the ReLU thresholds are not MARGIN away from every value"
        assert dev_y1 <= Y1_DEVIATION[precision], f"y1 deviates by {dev_y1:.3e}: Y1_DEVIATION is out of date"
    fwd = _rel(out, out64)
    print(f"GPUTEST finetune forward {name} {precision} layer {layer_num}: {fwd:.3e}")
    assert fwd <= FWD_TOL[precision] * DEPTH_FACTOR[name]
    loss = U.DiceLoss()(out, y)
    assert abs(float(loss) - loss64) <= FWD_TOL[precision] * DEPTH_FACTOR[name] * max(1.0, abs(loss64))
    loss.backward()
    _assert_errors(_errors(lp, ref["dice"], tol, y1_grads[0] if y1_grads else None), tol,
                   f"{name} {precision} layer {layer_num} dice")
    lp.zero_grad(set_to_none=True)
    lp(x).backward(_upstream(out.shape).float().to(dev))
    _assert_errors(_errors(lp, ref["upstream"], tol, y1_grads[1] if y1_grads else None), tol,
                   f"{name} {precision} layer {layer_num} upstream")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["wrap_p8_64", "ft384", "ft96_d12"])
def test_end_to_end_one_layer(dev, name, precision):
    _end_to_end(dev, name, precision, 1)


@pytest.mark.parametrize("name,precision", LAYER2_CLAIMED)
def test_end_to_end_two_layer(dev, name, precision):
    _end_to_end(dev, name, precision, 2)


@pytest.mark.parametrize("name,precision", LAYER2_FINITE_ONLY)
def test_end_to_end_two_layer_bf16_stays_finite(dev, name, precision):
    _end_to_end(dev, name, precision, 2, claimed=False)


# ---- (c) the training-mode forward against the eval-mode forward --------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", ["wrap_p8_64", "ft384"])
def test_training_forward_matches_eval_forward(dev, name, precision):
    lp, x = _model(name, 1, precision, dev)
    fmap_t, out_t = lp.encoder(x), lp(x)
    assert fmap_t.grad_fn is not None and out_t.grad_fn is not None
    lp.eval()
    fmap_e, out_e = lp.encoder(x), lp(x)
    assert fmap_e.grad_fn is None and out_e.grad_fn is None and fmap_e.shape == fmap_t.shape
    tol = FWD_TOL[precision]
    d_map, d_out = float((fmap_t - fmap_e).abs().max()), float((out_t - out_e).abs().max())
    print(f"GPUTEST finetune train vs eval {name} {precision}: map {d_map:.3e}, output {d_out:.3e}")
    assert d_map <= tol and d_out <= tol


# ---- (d) partial fine-tuning ----------------------------------------------------------------------------------------------------
def _step(lp, x, y, first):
    """One forward + backward after a warm-up step (operand caches built); (gradients, peak bytes above the resting level).
    The resting level is read after a garbage collection: device memory that earlier tests left to the cycle collector would
    count as resting, and a collection that happened to run inside the measured step would free it below that level."""
    enc = lp.encoder
    for n, p in enc.named_parameters():
        p.requires_grad_(n.startswith("norm.") or (n.startswith("blocks.") and int(n.split(".")[1]) >= first))
    peak = None
    for _ in range(2):
        lp.zero_grad(set_to_none=True)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        rest = torch.cuda.memory_allocated()
        U.DiceLoss()(lp(x), y).backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - rest
    return {n: p.grad.clone() if p.grad is not None else None for n, p in lp.named_parameters()}, peak


@pytest.mark.parametrize("name", ["ft384_d3", "ft96_d12"])
def test_partial_finetuning_same_bits_and_less_memory(dev, name):
    c = GEOMS[name]
    lp, x = _model(name, 1, "bf16x3", dev)
    y = LPT._target(x)
    full, peak_full = _step(lp, x, y, 0)
    N, D, B = (c["img_size"] // c["patch"]) ** 2 + 1, c["dim"], c["batch"]
    per_block = (5 + 4) * N * D * 4 + N * D * 4  # (5 + mlp_ratio) N D fp32 + the context (split pairs: 4 bytes)
    for j in (1, c["depth"] - 1):
        part, peak = _step(lp, x, y, j)
        for n, g in part.items():
            below = n.startswith("encoder.") and not n.startswith("encoder.norm.") and not (
                n.startswith("encoder.blocks.") and int(n.split(".")[2]) >= j)
            if below or n.startswith("two_layer_decoder."):
                assert g is None, n
            else:
                assert_same_bits(g, full[n], f"{n} with blocks below {j} frozen")
        saved = peak_full - peak
        print(f"GPUTEST finetune partial {name} j={j}: peak {peak / 2**20:.1f} MiB vs {peak_full / 2**20:.1f} MiB, saved "
              f"{saved / 2**20:.1f} MiB, per block and batch {B * per_block / 2**20:.1f} MiB")
        if name == "ft384_d3":  # activations dominate the step's memory there (35 MB per block and image)
            assert saved >= 0.8 * j * B * per_block


# ---- (e) opt-in -------------------------------------------------------------------------------------------------------------------
def test_without_the_flag_todays_behaviour_holds(dev):
    lp, x = _model("wrap_p8_64", 2, "bf16x3", dev, flag=False)
    with pytest.raises(NotImplementedError):
        lp(x)
    lp1, x1 = _model("wrap_p8_64", 1, "bf16x3", dev, flag=False)
    assert lp1(x1).grad_fn is None
    assert lp1.encoder(x1).grad_fn is None
    enc = lp1.encoder.enable_finetune()
    z = enc(x1)
    assert z.grad_fn is not None and z.shape == (2, 128, 8, 8)
    z.sum().backward()
    assert all(p.grad is not None for p in enc.parameters())
    with torch.no_grad():
        assert enc(x1).grad_fn is None
    assert enc.eval()(x1).grad_fn is None


def test_training_mode_without_a_graph(dev):
    """finetune.py's evaluate() may run the wrapper under no_grad: the decoder normalises with batch statistics, no graph."""
    lp, x = _model("wrap_p8_64", 2, "bf16x3", dev)
    with torch.no_grad():
        out = lp(x)
    assert out.grad_fn is None and int(lp.two_layer_decoder[1].num_batches_tracked) == 1
    assert _rel(out, _reference("wrap_p8_64", 2)[0]) <= FWD_TOL["bf16x3"]


# ---- (f) optimizer steps, accumulation, autograd's rules ---------------------------------------------------------------------
def test_adam_steps_lower_the_loss_and_track_the_twin(dev):
    """Three Adam steps (finetune.py: Adam on every parameter, lr 1e-4) on wrap_p8_64 in split-bf16, two-layer decoder. Adam's eps
    is 1e-6, above the gradient error (test_mim_train_gpu.py: an element at round-off level would otherwise move by +-lr with a
    sign that is noise). Afterwards the product's state goes into the twin and the eval-mode outputs are compared, as
    test_linear_probing_train_gpu.py does."""
    name, precision = "wrap_p8_64", "bf16x3"
    c, sd, x64 = _inputs(name)
    lp, x = _model(name, 2, precision, dev)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    dec = _fresh_decoder(name, 2, _separated_bias(name)[0]).double().train()
    cfg = O.make_cfg(prm, c["patch"], c["heads"])
    opt = torch.optim.Adam(lp.parameters(), lr=1e-4, eps=1e-6)
    opt64 = torch.optim.Adam(list(prm.values()) + list(dec.parameters()), lr=1e-4, eps=1e-6)
    y, loss_fn = LPT._target(x), U.DiceLoss()
    track = []
    for step in range(3):
        opt.zero_grad()
        opt64.zero_grad()
        loss = loss_fn(lp(x), y)
        loss64 = LPT.dice_loss(dec(O.encoder_fmap(prm, cfg, x64.double(), c["img_size"])), y.double().cpu())
        loss.backward()
        loss64.backward()
        opt.step()
        opt64.step()
        track.append((float(loss), float(loss64)))
        print(f"GPUTEST finetune adam step {step}: loss {track[-1][0]:.6f}, twin {track[-1][1]:.6f}")
        assert abs(track[-1][0] - track[-1][1]) <= 1e-3 * abs(track[-1][1])
    with torch.no_grad():
        after = float(loss_fn(lp(x), y))
    print(f"GPUTEST finetune adam after step 2: loss {after:.6f}")
    assert after < track[2][0] < track[0][0] and track[1][0] < track[0][0]
    dec.load_state_dict({k: v.double().cpu() if v.is_floating_point() else v.cpu()
                         for k, v in lp.two_layer_decoder.state_dict().items()})
    sd_now = {k: v.detach().double().cpu() for k, v in lp.encoder.state_dict().items()}
    lp.eval()
    dec.eval()
    with torch.no_grad():
        out = lp(x)
        want = dec(O.encoder_fmap(sd_now, cfg, x64.double(), c["img_size"]))
    assert _rel(out, want) <= FWD_TOL[precision]


def test_accumulation_second_backward_and_repeated_steps(dev):
    lp, x = _model("wrap_p8_64", 2, "bf16x3", dev)
    y, loss_fn = LPT._target(x), U.DiceLoss()
    loss = loss_fn(lp(x), y)
    loss.backward()
    first = {n: p.grad.clone() for n, p in lp.named_parameters() if p.grad is not None}
    assert any(n.startswith("encoder.blocks.0.") for n in first) and "encoder.pos_embed" in first
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        loss.backward()
    loss_fn(lp(x), y).backward()  # accumulates: the same bits twice, the sum is exactly 2 g
    for n, g in first.items():
        assert torch.equal(dict(lp.named_parameters())[n].grad, g + g), n
    for rep in range(2):  # repeated identical steps: the same bits
        lp.zero_grad(set_to_none=True)
        loss_fn(lp(x), y).backward()
        for n, g in first.items():
            assert_same_bits(dict(lp.named_parameters())[n].grad, g, f"grad {n}, repeat {rep + 1}")
