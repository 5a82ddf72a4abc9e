"""Replaced modules and parameters whose memory the allocator hands to their successors (engine.SourceCache): every model of
the package, several rounds in a row. The old instance is dropped before the replacement is built, the replacement is built the
way the model was (the same in-place steps, so the version counters agree), and the result is compared with torch.equal against
a freshly constructed model carrying the same state dict: same kernels, same order, same bits. Needs an MI355X."""
import gc
from functools import partial

import pytest
import torch
import torch.nn as nn

import vit_ocm_wmsegmentation_amd.dino.vision_transformer as vits
from tests.golden_cases import SWIN_GEOMETRIES, WRAPPER_CASES
from tests.unet_twin import make_case
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd import swin as SW
from vit_ocm_wmsegmentation_amd import synth
from vit_ocm_wmsegmentation_amd.dino.utils import trunc_normal_

pytestmark = pytest.mark.gpu

ROUNDS = 4
WRAP = WRAPPER_CASES["wrap_p8_64"]
SWIN = dict(synth.SWIN_TINY, **SWIN_GEOMETRIES["C"]["cfg"])
# the gradient limits of the paths' own training tests (test_mim_train_gpu.py, test_swin_train_gpu.py), split-bf16
MIM_TOL, SWIN_TOL = 1e-3, 3e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _values(shape, round_, scale=0.05):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + round_)) * scale


def _versions(module):
    return [p._version for p in module.parameters()]


def _loaded(module, state, dev, init=None):
    """A module built the way the models here are: constructed (and initialised by `init`), load_state_dict, .to(device)."""
    if init is not None:
        init(module)
    msg = module.load_state_dict(state, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    return module.to(dev)


def _swap(parent, name, build):
    """Drop parent.<name> (a sub-module or a parameter), collect, then put build() in its place. Returns the new child after
    checking that it is where the old one was in everything but its memory: the same version counters."""
    old = getattr(parent, name)
    versions = _versions(old) if isinstance(old, nn.Module) else [old._version]
    del old
    setattr(parent, name, None)
    gc.collect()
    new = build()
    setattr(parent, name, new)
    assert (_versions(new) if isinstance(new, nn.Module) else [new._version]) == versions
    return new


# ---- VisionTransformer: the engine's parameter upload, with and without the automatic graph replay ----
def _vit(state, dev, auto_graph):
    model = _loaded(vits.vit_tiny(patch_size=16, num_classes=0), state, dev).eval().requires_grad_(False)
    model.auto_graph = auto_graph
    return model


@pytest.mark.parametrize("what", ["module", "parameter"])
@pytest.mark.parametrize("auto_graph", [True, False])
def test_vit_follows_a_replaced_qkv(dev, auto_graph, what):
    model = _vit(synth.synth_arch_state_dict("vit_tiny", 16, seed=3, variant="full"), dev, auto_graph)
    x = synth.synth_tiles(1, 224, seed=5).to(dev)
    attn = model.blocks[1].attn
    seen = [model.get_last_selfattention(x) for _ in range(3)]
    for r in range(8):
        def linear():
            lin = _loaded(nn.Linear(192, 576), {"weight": _values((576, 192), r), "bias": _values((576,), r, 0.1)}, dev,
                          init=model._init_weights)
            return lin.requires_grad_(False)
        if what == "module":
            _swap(attn, "qkv", linear)
        else:
            _swap(attn.qkv, "weight", lambda: linear().weight)
        got = [model.get_last_selfattention(x) for _ in range(3)]  # with auto_graph: launches, a capture, a replay
        want = _vit(model.state_dict(), dev, False).get_last_selfattention(x)
        for g in got:
            assert torch.equal(g, want), f"round {r}"
        assert not torch.equal(want, seen[-1])
        seen.append(want)


# ---- free-standing Mlp and Attention: one operand copy per weight ----
def test_free_standing_mlp_follows_a_replaced_fc1(dev):
    x = torch.randn(2, 37, 128, generator=torch.Generator().manual_seed(1)).to(dev)
    mlp = vits.Mlp(128, 512).to(dev).eval()
    last = mlp(x)
    for r in range(ROUNDS):
        _swap(mlp, "fc1", lambda: nn.Linear(128, 512).to(dev))
        got = mlp(x)
        assert torch.equal(got, _loaded(vits.Mlp(128, 512), mlp.state_dict(), dev).eval()(x)), f"round {r}"
        assert not torch.equal(got, last)
        last = got


def test_free_standing_attention_follows_a_replaced_qkv(dev):
    x = torch.randn(2, 37, 128, generator=torch.Generator().manual_seed(2)).to(dev)
    att = vits.Attention(128, num_heads=2, qkv_bias=True).to(dev).eval()
    last = att(x)
    for r in range(ROUNDS):
        _swap(att, "qkv", lambda: nn.Linear(128, 384).to(dev))
        got = att(x)
        want = _loaded(vits.Attention(128, num_heads=2, qkv_bias=True), att.state_dict(), dev).eval()(x)
        for g, w in zip(got, want):
            assert torch.equal(g, w), f"round {r}"
        assert not torch.equal(got[0], last[0])
        last = got


# ---- the wrappers of model.py in eval mode: the head's operand, the folded two-layer decoder ----
def _encoder_kw():
    c = WRAP
    return dict(patch_size=c["patch"], embed_dim=c["dim"], depth=c["depth"], num_heads=c["heads"], mlp_ratio=4,
                img_size=[c["img_size"]], qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)


def _wrap_inputs(dev):
    c = WRAP
    x = synth.synth_tiles(c["batch"], c["img_size"], seed=c["seed"] + 100).to(dev)
    return x, synth.synth_patch_mask(c["batch"], c["img_size"] // c["patch"], seed=c["seed"])


def _encoder_state():
    c = WRAP
    return synth.synth_state_dict(c["dim"], c["depth"], c["patch"], seed=c["seed"], variant=c["variant"], img_size=224)


def _probe(state, layer_num, dev):
    lp = M.LinearProbing(M.VisionTransformerForFinetune(**_encoder_kw()), WRAP["patch"], layer_num=layer_num)
    if state is not None:
        _loaded(lp, state, dev)
    else:
        assert not lp.encoder.load_state_dict(_encoder_state(), strict=True).missing_keys
    return lp.to(dev).eval()


@pytest.mark.parametrize("layer_num,decoder,index,conv", [
    (1, "one_layer_decoder", "0", lambda D, s: nn.Conv2d(D, s * s, kernel_size=1)),
    (2, "two_layer_decoder", "0", lambda D, s: nn.Conv2d(D, 4 * s * s, kernel_size=3, padding=1)),
    (2, "two_layer_decoder", "3", lambda D, s: nn.Conv2d(4 * s * s, s * s, kernel_size=3, padding=1))])
def test_linear_probing_follows_a_replaced_conv(dev, layer_num, decoder, index, conv):
    x, _ = _wrap_inputs(dev)
    lp = _probe(None, layer_num, dev)
    last = lp(x)
    for r in range(ROUNDS):
        _swap(getattr(lp, decoder), index, lambda: conv(WRAP["dim"], WRAP["patch"]).to(dev))
        got = lp(x)
        assert torch.equal(got, _probe(lp.state_dict(), layer_num, dev)(x)), f"round {r}"
        assert not torch.equal(got, last)
        last = got


def _mim(state, dev):
    mim = M.MIM(M.VisionTransformerForSimMIM(**_encoder_kw()), WRAP["patch"])
    mim.patch_size = WRAP["patch"]
    return _loaded(mim, state, dev)


def _mim_state():
    wp = synth.synth_wrapper_params(WRAP["dim"], WRAP["patch"], 3, seed=WRAP["seed"])
    state = {"encoder." + k: v for k, v in _encoder_state().items()}
    state.update({"encoder.mask_token": wp["mask_token"], "decoder.0.weight": wp["decoder.weight"],
                  "decoder.0.bias": wp["decoder.bias"]})
    return state


def test_mim_eval_follows_a_replaced_conv(dev):
    x, mask = _wrap_inputs(dev)
    mim = _mim(_mim_state(), dev).eval()
    last = mim(x, mask)[1]
    out = 3 * WRAP["patch"] ** 2
    for r in range(ROUNDS):
        state = {"weight": _values((out, WRAP["dim"], 1, 1), r), "bias": _values((out,), r)}
        _swap(mim.decoder, "0", lambda: _loaded(nn.Conv2d(WRAP["dim"], out, kernel_size=1), state, dev))
        got = mim(x, mask)[1]
        assert torch.equal(got, _mim(mim.state_dict(), dev).eval()(x, mask)[1]), f"round {r}"
        assert not torch.equal(got, last)
        last = got


# ---- build_unet: the folded operands of one convolution ----
def test_unet_follows_a_replaced_conv(dev):
    x64 = torch.randn(3, 3, 16, 16, generator=torch.Generator().manual_seed(21), dtype=torch.float64)
    state = {k: v.float() if v.is_floating_point() else v for k, v in make_case(21, x64).state_dict().items()}
    net = _loaded(M.build_unet(), state, dev).eval()
    x = x64.float().to(dev)
    last = net(x)
    for r in range(ROUNDS):
        conv = {"weight": _values((128, 64, 3, 3), r), "bias": _values((128,), r)}
        _swap(net.e2.conv, "conv1", lambda: _loaded(nn.Conv2d(64, 128, kernel_size=3, padding=1), conv, dev))
        got = net(x)
        assert torch.equal(got, _loaded(M.build_unet(), net.state_dict(), dev).eval()(x)), f"round {r}"
        assert not torch.equal(got, last)
        last = got


# ---- Swin: the engine's parameter upload ----
SWIN_FLAT = "swin__encoder__layers__0__blocks__1__mlp__fc1__weight"


def _swin(state, dev, precision="bf16x3"):
    cfg = SW.SwinConfig(**{k: v for k, v in SWIN.items() if k != "patch_size"}, drop_path_rate=0.0)
    return _loaded(SW.SwinForImageClassification(cfg), state, dev).set_precision(precision)


def _swin_inputs(dev):
    c = SWIN_GEOMETRIES["C"]
    x = synth.synth_tiles(c["batch"], SWIN["image_size"], seed=c["seed"] + 50, channels=SWIN["num_channels"])
    labels = torch.randint(0, SWIN["num_labels"], (c["batch"],), generator=torch.Generator().manual_seed(c["seed"]))
    return synth.synth_swin_state_dict(SWIN, seed=c["seed"], qk_gain=c["qk_gain"]), x.to(dev), labels.to(dev)


def _swin_parameter(shape, round_, dev, requires_grad):
    """A flat parameter as SwinForImageClassification makes and loads one: zeros, trunc_normal_, copy_, .to(device)."""
    p = nn.Parameter(torch.zeros(shape), requires_grad=False)
    trunc_normal_(p, std=.02)
    with torch.no_grad():
        p.copy_(_values(shape, round_))
    p.data = p.data.to(dev)
    return p.requires_grad_(requires_grad)


def test_swin_follows_a_replaced_parameter(dev):
    state, x, _ = _swin_inputs(dev)
    model = _swin(state, dev).eval()
    last = model(pixel_values=x).logits
    shape = getattr(model, SWIN_FLAT).shape
    for r in range(ROUNDS):
        _swap(model, SWIN_FLAT, lambda: _swin_parameter(shape, r, dev, False))
        got = model(pixel_values=x).logits
        assert torch.equal(got, _swin(model.state_dict(), dev).eval()(pixel_values=x).logits), f"round {r}"
        assert not torch.equal(got, last)
        last = got


# ---- training: the operand copies and transposes of _EncoderTrain and _SwinTrain. Gradients are compared as the paths' own
# training tests compare them, max |g - g_ref| / max |g_ref| per tensor at their split-bf16 limit, against a fresh model ----
def _grad_errors(model, fresh, scale_of=lambda name: name):
    ref = {n: p.grad for n, p in fresh.named_parameters()}
    errs = {}
    for n, p in model.named_parameters():
        assert p.grad is not None and ref[n] is not None, n
        errs[n] = float((p.grad - ref[n]).abs().max() / ref[scale_of(n)].abs().max().clamp_min(1e-30))
    return errs


def test_mim_training_follows_a_replaced_weight(dev):
    x, mask = _wrap_inputs(dev)
    mim = _mim(_mim_state(), dev).train()
    mim(x, mask)[0].backward()
    first = mim.encoder.blocks[0].mlp.fc2.weight.grad.clone()
    mim.zero_grad(set_to_none=True)
    fc1 = mim.encoder.blocks[0].mlp.fc1
    state = {"weight": _values(fc1.weight.shape, 0), "bias": _values(fc1.bias.shape, 0)}
    _swap(fc1, "weight", lambda: _loaded(nn.Linear(128, 512), state, dev, init=mim.encoder._init_weights).weight)
    mim(x, mask)[0].backward()
    fresh = _mim(mim.state_dict(), dev).train()
    fresh(x, mask)[0].backward()
    errs = _grad_errors(mim, fresh)
    worst = max(errs, key=errs.get)
    assert errs[worst] <= MIM_TOL, f"{worst}: {errs[worst]:.3e}"
    assert not torch.equal(mim.encoder.blocks[0].mlp.fc2.weight.grad, first)


def test_swin_training_follows_a_replaced_weight(dev):
    state, x, labels = _swin_inputs(dev)
    model = _swin(state, dev).train().requires_grad_(True)
    model(pixel_values=x, labels=labels).loss.backward()
    first = getattr(model, SWIN_FLAT.replace("fc1", "fc2")).grad.clone()
    model.zero_grad(set_to_none=True)
    shape = getattr(model, SWIN_FLAT).shape
    _swap(model, SWIN_FLAT, lambda: _swin_parameter(shape, 0, dev, True))
    model(pixel_values=x, labels=labels).loss.backward()
    fresh = _swin(model.state_dict(), dev).train().requires_grad_(True)
    fresh(pixel_values=x, labels=labels).loss.backward()
    # (k_proj.bias is measured against its weight's gradient, as in test_swin_train_gpu.py: its exact gradient is zero)
    errs = _grad_errors(model, fresh, lambda n: n[:-len("bias")] + "weight" if n.endswith("k_proj__bias") else n)
    worst = max(errs, key=errs.get)
    assert errs[worst] <= SWIN_TOL, f"{worst}: {errs[worst]:.3e}"
    assert not torch.equal(getattr(model, SWIN_FLAT.replace("fc1", "fc2")).grad, first)
