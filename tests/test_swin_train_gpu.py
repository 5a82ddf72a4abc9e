"""SwinForImageClassification in training mode on the HIP path (Allen_data_Backbone/train.py fine-tunes it with the HF Trainer):
every parameter's gradient against a float64 CPU twin (oracle.swin_oracle under torch autograd; with stochastic depth, the
layer restated below with the masks the module drew), frozen subsets, accumulation, refusals, a train.py-shaped AdamW loop and
the eval-mode forward afterwards. Needs an MI355X.

Error measure: max |g - g64| / max |g64| per tensor. Limits (TOL) from MI355X measurements with headroom."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import swin_oracle as SO
from tests.golden_cases import SWIN_GEOMETRIES
from vit_ocm_wmsegmentation_amd import _lib, synth
from vit_ocm_wmsegmentation_amd import swin as SW

pytestmark = pytest.mark.gpu

# measured worst (MI355X): fp32 2.9e-5, bf16x3 9.4e-5, bf16 5.3e-2 (geometry F, 1000 labels); limits about 3x that
TOL = {"fp32": 1e-4, "bf16x3": 3e-4, "bf16": 1.5e-1}
# Swin-T at 224^2 with train.py's 5 labels and per-device batch 8, and the unpadded geometries of tests/golden_cases.py
CASES = {"swin_t": dict(cfg=dict(synth.SWIN_TINY), batch=8, seed=71, qk_gain=4.0),
         # q / k projections x8 and the relative-position table x200: peaked windows. Single bf16 is not claimed there (README)
         "swin_t_peaked": dict(cfg=dict(synth.SWIN_TINY), batch=8, seed=71, qk_gain=8.0)}
CASES.update({f"geom_{k}": dict(cfg=dict(synth.SWIN_TINY, **SWIN_GEOMETRIES[k]["cfg"]), batch=SWIN_GEOMETRIES[k]["batch"],
                                seed=SWIN_GEOMETRIES[k]["seed"], qk_gain=SWIN_GEOMETRIES[k]["qk_gain"]) for k in "BCEFH"})


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


def _inputs(name):
    c = CASES[name]
    cfg = c["cfg"]
    sd = synth.synth_swin_state_dict(cfg, seed=c["seed"], qk_gain=c["qk_gain"])
    x = synth.synth_tiles(c["batch"], cfg["image_size"], seed=c["seed"] + 50, channels=cfg["num_channels"])
    g = torch.Generator().manual_seed(c["seed"])
    labels = torch.randint(0, max(cfg["num_labels"], 1), (c["batch"],), generator=g)
    up = torch.randn(c["batch"], cfg["num_labels"], generator=g, dtype=torch.float64)  # upstream gradient when num_labels < 2
    return cfg, sd, x, labels, up


def _model(name, precision, dev, rate=0.0):
    cfg, sd, x, labels, up = _inputs(name)
    hf = SW.SwinConfig(**{k: v for k, v in cfg.items() if k != "patch_size"}, drop_path_rate=rate)
    m = SW.SwinForImageClassification(hf)
    assert not m.load_state_dict(sd, strict=True).missing_keys
    return m.to(dev).set_precision(precision).train().requires_grad_(True), x.to(dev), labels.to(dev), up


def _loss(m, x, labels, up):
    if m.config.num_labels >= 2:
        return m(pixel_values=x, labels=labels).loss
    return (m(pixel_values=x).logits.double() * up.to(x.device)).sum()


def _layer(sd, pre, x, H, heads, ws, shift, eps, scale):
    """SO.swin_layer on an unpadded grid with the attention branch scaled per image (SwinDropPath: branch / keep * mask)."""
    B, L, C = x.shape
    a = pre + "attention."
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_before.weight"], sd[pre + "layernorm_before.bias"], eps).view(B, H, H, C)
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(y, ws).view(-1, ws * ws, C)
    q, k, v = [F.linear(win, sd[a + n + "_proj.weight"], sd[a + n + "_proj.bias"]).view(-1, ws * ws, heads, 32).transpose(1, 2)
               for n in "qkv"]
    table = sd[a + "relative_position_bias.relative_position_bias_table"]
    bias = table[SO.relative_position_index(ws).view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1).unsqueeze(0)
    mask = SO.shift_mask(H, H, ws, shift, x.dtype)
    if mask is not None:
        nW = mask.shape[0]
        bias = bias + mask.unsqueeze(1).unsqueeze(0).expand(win.shape[0] // nW, -1, -1, -1, -1).reshape(-1, 1, ws * ws, ws * ws)
    p = F.softmax(q @ k.transpose(2, 3) * 32 ** -0.5 + bias, dim=-1)
    o = F.linear((p @ v).transpose(1, 2).reshape(-1, ws * ws, C), sd[a + "o_proj.weight"], sd[a + "o_proj.bias"])
    o = SO.window_reverse(o.view(-1, ws, ws, C), ws, H, H)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    o = o.reshape(B, L, C)
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
            H //= 2
    seq = F.layer_norm(t, (t.shape[-1],), sd["swin.layernorm.weight"], sd["swin.layernorm.bias"], eps)
    return F.linear(seq.mean(1), sd["classifier.weight"], sd["classifier.bias"])


def _twin_grads(name, masks):
    cfg, sd, x, labels, up = _inputs(name)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    logits = _twin_logits(prm, cfg, x.double(), masks)
    loss = F.cross_entropy(logits, labels) if cfg["num_labels"] >= 2 else (logits * up).sum()
    loss.backward()
    return {k: v.grad for k, v in prm.items()}


@functools.lru_cache(maxsize=None)
def _reference(name):
    return _twin_grads(name, [None] * sum(CASES[name]["cfg"]["depths"]))


def _rel(a, ref):
    return float((a.detach().double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _check(m, ref, tol, what):
    """k_proj.bias is measured against the largest k_proj.weight gradient: its exact gradient is zero (adding a constant to
    every key adds q . b to a whole row of scores, which the softmax ignores), so the float64 value is round-off."""
    errs = {}
    for flat, p in m.named_parameters():
        key = m._names[flat]
        assert p.grad is not None, key
        if key.endswith("k_proj.bias"):
            wref = ref[key[:-len("bias")] + "weight"]
            errs[key] = float((p.grad.detach().double().cpu() - ref[key]).abs().max() / wref.abs().max())
        else:
            errs[key] = _rel(p.grad, ref[key])
    worst = max(errs, key=errs.get)
    print(f"GPUTEST swin train {what}: worst {worst} {errs[worst]:.3e}")
    assert errs[worst] <= tol, f"{what}: {worst}: {errs[worst]:.3e} > {tol:.0e}"
    return errs


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_grads_match_float64(dev, name, precision):
    """Drop-path rate 0: loss.backward() fills every parameter's .grad, relative-position tables and classifier included."""
    m, x, labels, up = _model(name, precision, dev)
    _loss(m, x, labels, up).backward()
    if name == "swin_t_peaked" and precision == "bf16":  # printed, finite
        _check(m, _reference(name), float("inf"), f"{name} {precision} (not claimed)")
        assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        return
    _check(m, _reference(name), TOL[precision], f"{name} {precision}")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_grads_match_float64_with_drop_path(dev, precision):
    """drop_path_rate 0.1 (transformers' default): the masks the module drew, redrawn from the same seed, go to the twin."""
    m, x, labels, up = _model("swin_t", precision, dev, rate=0.1)
    torch.manual_seed(123)
    _loss(m, x, labels, up).backward()
    torch.manual_seed(123)
    masks = SW.draw_drop_path_masks(m.config, x.shape[0], dev)
    assert masks[0] is None and all(mk is not None for mk in masks[1:])
    assert any(float(mk[1].min()) == 0 for mk in masks[1:])  # some image's branch is dropped somewhere
    _check(m, _twin_grads("swin_t", masks), TOL[precision], f"swin_t drop path 0.1 {precision}")


def _grads(m):
    return {m._names[n]: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_frozen_subsets_and_accumulation(dev, precision):
    """Frozen parameters get .grad None and the others the full run's bits; a second loss.backward() from a second forward
    doubles every gradient exactly (the reruns give the same bits)."""
    name = "geom_E"  # four stages
    m, x, labels, up = _model(name, precision, dev)
    _loss(m, x, labels, up).backward()
    full = {k: g.clone() for k, g in _grads(m).items()}
    _loss(m, x, labels, up).backward()
    for k, g in _grads(m).items():
        assert torch.equal(g, 2 * full[k]), k
    for frozen in (lambda k: not k.startswith("classifier."),
                   lambda k: k.startswith("swin.embeddings.") or k.startswith("swin.encoder.layers.0.")
                   or k.startswith("swin.encoder.layers.1.")):
        m.zero_grad(set_to_none=True)
        for n, p in m.named_parameters():
            p.requires_grad_(not frozen(m._names[n]))
        _loss(m, x, labels, up).backward()
        for k, g in _grads(m).items():
            if frozen(k):
                assert g is None, k
            else:
                assert torch.equal(g, full[k]), k
        m.requires_grad_(True)


def test_second_backward_and_inplace_edit_refused(dev):
    m, x, labels, up = _model("geom_H", "bf16x3", dev)
    loss = _loss(m, x, labels, up)
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    loss = _loss(m, x, labels, up)
    with torch.no_grad():
        m.classifier__weight.add_(1.0)
    with pytest.raises(RuntimeError, match="inplace"):
        loss.backward()


def test_frozen_and_eval_keep_inference(dev):
    """A fresh module in training mode (every parameter frozen), eval mode and no_grad run inference: no graph, and the
    logits of the engine."""
    m, x, labels, up = _model("geom_H", "bf16x3", dev)
    m.requires_grad_(False)
    a = m(pixel_values=x, labels=labels)
    assert a.loss.grad_fn is None and not a.logits.requires_grad
    m.requires_grad_(True)
    with torch.no_grad():
        b = m(pixel_values=x)
    c = m.eval()(pixel_values=x)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.logits, c.logits) and c.logits.grad_fn is None


def test_output_answers_trainer_indexing(dev):
    m, x, labels, up = _model("geom_H", "fp32", dev)
    out = m(pixel_values=x, labels=labels)
    assert out["loss"] is out.loss and out[0] is out.loss and out[1] is out.logits
    assert out.loss.requires_grad and out.logits.requires_grad
    assert m(pixel_values=x)[0] is not None


def test_refusals_raise_before_any_launch(dev, monkeypatch):
    """Every refusal raises its own error before the library is touched (the patched loader would raise instead)."""
    m, x, labels, up = _model("geom_H", "bf16x3", dev)
    c = m.config

    def no_launch():
        raise AssertionError("the library was called before the refusal")

    monkeypatch.setattr(_lib, "load", no_launch)
    with pytest.raises(NotImplementedError, match="gradient of the input"):
        m(pixel_values=x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="int64"):
        m(pixel_values=x, labels=labels.float())
    c.hidden_dropout_prob = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        m(pixel_values=x)
    c.hidden_dropout_prob, c.attention_probs_dropout_prob = 0.0, 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        m(pixel_values=x)
    c.attention_probs_dropout_prob = 0.0
    for k in "ADG":  # transformers' padding paths
        gcfg = dict(synth.SWIN_TINY, **SWIN_GEOMETRIES[k]["cfg"])
        g = SW.SwinForImageClassification(SW.SwinConfig(**{a: v for a, v in gcfg.items() if a != "patch_size"}))
        g = g.to(dev).train().requires_grad_(True)
        xg = torch.zeros(1, gcfg["num_channels"], gcfg["image_size"], gcfg["image_size"], device=dev)
        with pytest.raises(NotImplementedError, match="padding"):
            g(pixel_values=xg)
    one = SW.SwinForImageClassification(SW.SwinConfig(image_size=64, embed_dim=32, depths=(2, 2, 1), num_heads=(1, 2, 4),
                                                      window_size=4, num_labels=1)).to(dev).train().requires_grad_(True)
    with pytest.raises(ValueError, match="num_labels"):
        one(pixel_values=torch.zeros(2, 3, 64, 64, device=dev), labels=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="HIP"):
        m(pixel_values=x.cpu(), labels=labels)


def test_trainpy_loop_tracks_float64_twin(dev):
    """train.py's loop: AdamW lr 5e-5, 4 accumulation steps, clip_grad_norm_(1.0), linear warmup (then linear decay), on the
    HIP module and on the float64 twin; afterwards the eval-mode logits equal those of a fresh module loaded with the trained
    state_dict."""
    name, precision, steps, accum, warmup = "geom_H", "fp32", 3, 4, 2
    cfg, sd, x, labels, up = _inputs(name)
    m, xd, ld, _ = _model(name, precision, dev)
    prm = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    sched_fn = lambda s: (s + 1) / warmup if s < warmup else max(0.0, (steps - s) / steps)  # noqa: E731
    opt = torch.optim.AdamW(m.parameters(), lr=5e-5)
    opt64 = torch.optim.AdamW(list(prm.values()), lr=5e-5)
    sched, sched64 = torch.optim.lr_scheduler.LambdaLR(opt, sched_fn), torch.optim.lr_scheduler.LambdaLR(opt64, sched_fn)
    for _ in range(steps):
        for micro in range(accum):
            xs, ls = xd.roll(micro, 0), ld.roll(micro, 0)
            (m(pixel_values=xs, labels=ls).loss / accum).backward()
            logits64 = _twin_logits(prm, cfg, xs.double().cpu(), [None] * sum(cfg["depths"]))
            (F.cross_entropy(logits64, ls.cpu()) / accum).backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        torch.nn.utils.clip_grad_norm_(list(prm.values()), 1.0)
        for o, sc in ((opt, sched), (opt64, sched64)):
            o.step()
            sc.step()
            o.zero_grad()
    errs = {m._names[n]: _rel(p, prm[m._names[n]].detach()) for n, p in m.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"GPUTEST swin train.py loop {name} {precision}: worst parameter {worst} {errs[worst]:.3e}")
    assert errs[worst] <= TOL[precision]
    m.eval()
    got = m(pixel_values=xd).logits
    fresh = SW.SwinForImageClassification(m.config)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev).set_precision(precision).eval()
    assert torch.equal(got, fresh(pixel_values=xd).logits)


def test_kept_activation_memory(dev):
    """Record the activations the training forward keeps for the backward, per image, Swin-T at 224^2."""
    m, x, labels, up = _model("swin_t", "bf16", dev, rate=0.1)
    out = m(pixel_values=x, labels=labels)
    per = m.__dict__["_train_kept_bytes"] / x.shape[0]
    print(f"GPUTEST swin train kept activations: {per / 2 ** 20:.1f} MiB per image (bf16, Swin-T 224^2)")
    assert 20 * 2 ** 20 < per < 120 * 2 ** 20
    out.loss.backward()
