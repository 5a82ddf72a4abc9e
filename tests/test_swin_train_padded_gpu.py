"""SwinForImageClassification.enable_padded_training on the HIP path: training on the geometries that need transformers' padding
paths (a stage grid that is not a multiple of the window, an odd grid before a patch merging). Every parameter's gradient and
the training-forward logits against the float64 CPU twin (oracle.swin_oracle under torch autograd, which walks both padding
paths; with stochastic depth, the layer restated below with the masks the module drew), a frozen subset, accumulation,
determinism, no drift on the unpadded geometries and the eval-mode forward after AdamW steps. Needs an MI355X.

Error measure and limits are those of tests/test_swin_train_gpu.py (max |g - g64| / max |g64| per tensor).
Measured worst per precision and case: DESIGN.md 3.34."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import swin_oracle as SO
from tests.golden_cases import SWIN_CASES, SWIN_GEOMETRIES
from tests.test_swin_train_gpu import TOL, _check, _grads, _loss, _rel
from vit_ocm_wmsegmentation_amd import synth
from vit_ocm_wmsegmentation_amd import swin as SW

pytestmark = pytest.mark.gpu

CASES = {k: dict(cfg=dict(synth.SWIN_TINY, **SWIN_GEOMETRIES[k]["cfg"]), batch=SWIN_GEOMETRIES[k]["batch"],
                 seed=SWIN_GEOMETRIES[k]["seed"], qk_gain=SWIN_GEOMETRIES[k]["qk_gain"]) for k in "ADGH"}  # H: no padding
CASES["pad120"] = dict(cfg=dict(synth.SWIN_TINY, **SWIN_CASES["pad120"]["cfg"]), batch=SWIN_CASES["pad120"]["batch"],
                       seed=SWIN_CASES["pad120"]["seed"], qk_gain=SWIN_CASES["pad120"]["qk_gain"])
# grids 24 -> 12 padded to 28 / 14: the last two stage geometries of Swin-T on a 384^2 tile, no odd merge
CASES["tile96"] = dict(cfg=dict(synth.SWIN_TINY, image_size=96, depths=(2, 2), num_heads=(3, 6), window_size=7, num_labels=5),
                       batch=2, seed=81, qk_gain=4.0)
CASES["swin_t"] = dict(cfg=dict(synth.SWIN_TINY), batch=2, seed=71, qk_gain=4.0)  # 224^2: no padding
PADDED = ("A", "D", "G", "pad120", "tile96")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = CASES[name]
    cfg = c["cfg"]
    sd = synth.synth_swin_state_dict(cfg, seed=c["seed"], qk_gain=c["qk_gain"])
    x = synth.synth_tiles(c["batch"], cfg["image_size"], seed=c["seed"] + 50, channels=cfg["num_channels"])
    labels = torch.randint(0, cfg["num_labels"], (c["batch"],), generator=torch.Generator().manual_seed(c["seed"]))
    return cfg, sd, x, labels


def _model(name, precision, dev, rate=0.0, padded=True):
    cfg, sd, x, labels = _inputs(name)
    m = SW.SwinForImageClassification(SW.SwinConfig(**{k: v for k, v in cfg.items() if k != "patch_size"}, drop_path_rate=rate))
    assert not m.load_state_dict(sd, strict=True).missing_keys
    m = m.to(dev).set_precision(precision).train().requires_grad_(True)
    return (m.enable_padded_training() if padded else m), x.to(dev), labels.to(dev)


def _layer(sd, pre, x, H, heads, ws, shift, eps, scale):
    """SO.swin_layer with the attention branch scaled per image (SwinDropPath: branch / keep * mask): zero rows after
    layernorm_before up to the window multiple, the shift mask of the padded grid, the padded positions' outputs dropped."""
    B, L, C = x.shape
    a = pre + "attention."
    Hp = -(-H // ws) * ws
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_before.weight"], sd[pre + "layernorm_before.bias"], eps).view(B, H, H, C)
    y = F.pad(y, (0, 0, 0, Hp - H, 0, Hp - H))
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(y, ws).view(-1, ws * ws, C)
    q, k, v = [F.linear(win, sd[a + n + "_proj.weight"], sd[a + n + "_proj.bias"]).view(-1, ws * ws, heads, 32).transpose(1, 2)
               for n in "qkv"]
    table = sd[a + "relative_position_bias.relative_position_bias_table"]
    bias = table[SO.relative_position_index(ws).view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1).unsqueeze(0)
    mask = SO.shift_mask(Hp, Hp, ws, shift, x.dtype)
    if mask is not None:
        nW = mask.shape[0]
        bias = bias + mask.unsqueeze(1).unsqueeze(0).expand(win.shape[0] // nW, -1, -1, -1, -1).reshape(-1, 1, ws * ws, ws * ws)
    p = F.softmax(q @ k.transpose(2, 3) * 32 ** -0.5 + bias, dim=-1)
    o = F.linear((p @ v).transpose(1, 2).reshape(-1, ws * ws, C), sd[a + "o_proj.weight"], sd[a + "o_proj.bias"])
    o = SO.window_reverse(o.view(-1, ws, ws, C), ws, Hp, Hp)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    o = o[:, :H, :H, :].reshape(B, L, C)
    if scale is not None:
        keep, m = scale
        o = o.div(keep) * m.view(B, 1, 1)
    x = x + o
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_after.weight"], sd[pre + "layernorm_after.bias"], eps)
    return x + F.linear(F.gelu(F.linear(y, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])), sd[pre + "mlp.fc2.weight"],
                        sd[pre + "mlp.fc2.bias"])


def _twin_logits(sd, cfg, x, masks):
    """The float64 twin: oracle.swin_forward itself without stochastic depth, else its restatement with the module's masks."""
    if all(m is None for m in masks):
        return SO.swin_forward.__wrapped__(sd, cfg, x)["logits"]
    e, eps, ws = "swin.embeddings.", cfg["layer_norm_eps"], cfg["window_size"]
    t = F.conv2d(x, sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"], stride=4)
    H = t.shape[-1]
    t = F.layer_norm(t.flatten(2).transpose(1, 2), (t.shape[1],), sd[e + "norm.weight"], sd[e + "norm.bias"], 1e-5)
    li = 0
    for s, (depth, heads) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
        for b in range(depth):
            shift = ws // 2 if b % 2 and H > ws else 0
            sc = None if masks[li] is None else (masks[li][0], masks[li][1].double().cpu())
            t = _layer(sd, f"swin.encoder.layers.{s}.blocks.{b}.", t, H, heads, ws, shift, eps, sc)
            li += 1
        if s + 1 < len(cfg["depths"]):
            t = SO.patch_merging(sd, f"swin.encoder.layers.{s}.downsample.", t, H, H)
            H = (H + 1) // 2
    seq = F.layer_norm(t, (t.shape[-1],), sd["swin.layernorm.weight"], sd["swin.layernorm.bias"], eps)
    return F.linear(seq.mean(1), sd["classifier.weight"], sd["classifier.bias"])


def _twin(name, masks):
    """(gradients, logits) of the float64 twin."""
    cfg, sd, x, labels = _inputs(name)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    logits = _twin_logits(prm, cfg, x.double(), masks)
    F.cross_entropy(logits, labels).backward()
    return {k: v.grad for k, v in prm.items()}, logits.detach()


@functools.lru_cache(maxsize=None)
def _reference(name):
    return _twin(name, [None] * sum(CASES[name]["cfg"]["depths"]))


def test_twin_restatement_is_the_oracle():
    """The restated layer (used with stochastic depth) gives the oracle's logits when every mask keeps every image."""
    for name in ("G", "tile96"):
        cfg, sd, x, labels = _inputs(name)
        sd64 = {k: v.double() for k, v in sd.items()}
        ones = [(1.0, torch.ones(x.shape[0]))] * sum(cfg["depths"])
        want = SO.swin_forward.__wrapped__(sd64, cfg, x.double())["logits"]
        assert float((_twin_logits(sd64, cfg, x.double(), ones) - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", PADDED)
def test_grads_and_logits_match_float64(dev, name, precision):
    """Drop-path rate 0: the training-forward logits and every parameter's gradient on the padded geometries."""
    m, x, labels = _model(name, precision, dev)
    out = m(pixel_values=x, labels=labels)
    out.loss.backward()
    ref, logits64 = _reference(name)
    e = _rel(out.logits, logits64)
    print(f"GPUTEST swin padded train {name} {precision}: logits {e:.3e}")
    errs = _check(m, ref, TOL[precision], f"padded {name} {precision}")
    for kind in ("q_proj.bias", "v_proj.bias", "layernorm_before.weight", "q_proj.weight"):
        worst = max(v for k, v in errs.items() if k.endswith(kind))
        print(f"GPUTEST swin padded train {name} {precision}: worst {kind} {worst:.3e}")
    assert e <= TOL[precision], f"{name} {precision}: logits {e:.3e} > {TOL[precision]:.0e}"


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["G", "tile96"])
def test_grads_match_float64_with_drop_path(dev, name, precision):
    """drop_path_rate 0.2, applied after the crop: the masks the module drew, redrawn from the same seed, go to the twin."""
    m, x, labels = _model(name, precision, dev, rate=0.2)
    seed = 7
    torch.manual_seed(seed)
    out = m(pixel_values=x, labels=labels)
    out.loss.backward()
    torch.manual_seed(seed)
    masks = SW.draw_drop_path_masks(m.config, x.shape[0], dev)
    assert masks[0] is None and all(mk is not None for mk in masks[1:])
    print(f"GPUTEST swin padded train {name} drop path masks: {[None if mk is None else mk[1].tolist() for mk in masks]}")
    ref, logits64 = _twin(name, masks)
    e = _rel(out.logits, logits64)
    _check(m, ref, TOL[precision], f"padded {name} drop path 0.2 {precision}")
    assert e <= TOL[precision], f"{name} {precision}: logits {e:.3e}"


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_frozen_subset_determinism_and_accumulation(dev, precision):
    """tile96. The same step twice gives the same gradient bits; with the embeddings and stage 0 frozen the frozen parameters get
    None and the others the full run's bits; two micro-batches accumulated into .grad are the sum of their gradients within
    the rounding of one fp32 addition."""
    m, x, labels = _model("tile96", precision, dev)
    _loss(m, x, labels, None).backward()
    full = {k: g.clone() for k, g in _grads(m).items()}
    m.zero_grad(set_to_none=True)
    _loss(m, x, labels, None).backward()
    for k, g in _grads(m).items():
        assert torch.equal(g, full[k]), k

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
    m.requires_grad_(True)

    x2, l2 = x.flip(0) * 0.5, labels.roll(1)  # a second micro-batch
    m.zero_grad(set_to_none=True)
    _loss(m, x2, l2, None).backward()
    second = {k: g.clone() for k, g in _grads(m).items()}
    m.zero_grad(set_to_none=True)
    _loss(m, x, labels, None).backward()
    _loss(m, x2, l2, None).backward()
    for k, g in _grads(m).items():
        exact = full[k].double() + second[k].double()
        assert bool(((g.double() - exact).abs() <= exact.abs() * 2.0 ** -24).all()), k


@pytest.mark.parametrize("name", ["H", "swin_t"])
def test_opt_in_changes_nothing_without_padding(dev, name):
    """Geometry H and Swin-T at 224^2 (batch 2) need no padding: the opt-in's gradients are the default's, bit for bit."""
    got = []
    for padded in (False, True):
        m, x, labels = _model(name, "bf16x3", dev, padded=padded)
        out = m(pixel_values=x, labels=labels)
        out.loss.backward()
        got.append((out.logits.detach().clone(), _grads(m), m.__dict__["_train_kept_bytes"]))
    assert torch.equal(got[0][0], got[1][0]) and got[0][2] == got[1][2]
    for k, g in got[0][1].items():
        assert torch.equal(g, got[1][1][k]), k


def test_refused_without_the_opt_in_and_hidden_state_with_it(dev):
    m, x, labels = _model("tile96", "bf16x3", dev, padded=False)
    with pytest.raises(NotImplementedError, match="padding"):
        m(pixel_values=x, labels=labels)
    out = m.enable_padded_training()(pixel_values=x, labels=labels, output_hidden_states=True)
    assert out.last_hidden_state.shape == (2, 144, 192) and out.hidden_states is None  # 12 x 12 tokens, not the padded 14 x 14
    assert m.__dict__["_train_kept_bytes"] > 0
    out.loss.backward()


def test_eval_after_adamw_steps_matches_a_fresh_module(dev):
    """Three AdamW steps on tile96, then eval(): the engine (which pads on its own) sees the trained weights — the logits of a
    fresh module loaded with the trained state_dict, bit for bit."""
    m, x, labels = _model("tile96", "bf16x3", dev)
    before = m.eval()(pixel_values=x).logits.clone()
    m.train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(3):
        loss = m(pixel_values=x, labels=labels).loss
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0]
    got = m.eval()(pixel_values=x).logits
    assert not torch.equal(got, before)
    fresh = SW.SwinForImageClassification(m.config)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev).set_precision("bf16x3").eval()
    assert torch.equal(got, fresh(pixel_values=x).logits)
