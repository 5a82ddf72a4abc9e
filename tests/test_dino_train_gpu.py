"""One DINO training step on the HIP path against a float64 twin: student and teacher MultiCropWrapper(VisionTransformer,
DINOHead), two global 32^2 crops (N = 17) and three local 16^2 crops (N = 5) of a batch of 2, DINOLoss at epoch 0 with a non-zero
centre, clip_gradients, cancel_gradients_last_layer, optimizer.AdamW, ema_update. Needs an MI355X.

Backbone: D = 128, depth 2, 2 heads of 64, patch 8, a 4 x 4 position grid (the local crops resample it to 2 x 2, and pos_embed's
gradient goes back through that resampling). Head (128, 128, 64, 96). The twin is tests/dino_ref.py: the oracle's encoder on
requires_grad leaves, TwinHead, dino_loss. Error measure: max |g - g64| / max |g64| per tensor; limits of
tests/test_mim_train_gpu.py: fp32 1e-4, bf16x3 1e-3, bf16 5e-2 (forward: 2e-5, 2e-4, 5e-2).

The two map encoders (VisionTransformerForFinetune, VisionTransformerForSimMIM) share the generalised _encode_train: their training
outputs and gradients are compared with fingerprints recorded by running the parent commit once
(tests/golden/dino_parent_fingerprints.json)."""
import functools
import json
import os
from functools import partial

import pytest
import torch
import torch.nn as nn

from oracle import vit_oracle as O
from tests import dino_ref as R
from vit_ocm_wmsegmentation_amd import optimizer as OPT
from vit_ocm_wmsegmentation_amd import synth
from vit_ocm_wmsegmentation_amd.dino import utils as DU
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as VT

pytestmark = pytest.mark.gpu

TOL = {"fp32": 1e-4, "bf16x3": 1e-3, "bf16": 5e-2}
FWD_TOL = {"fp32": 2e-5, "bf16x3": 2e-4, "bf16": 5e-2}
DIM, DEPTH, HEADS, PATCH, SIDE, LOCAL, BATCH, NCROPS = 128, 2, 2, 8, 32, 16, 2, 5
HEAD = dict(in_dim=DIM, out_dim=96, hidden_dim=128, bottleneck_dim=64)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dino_parent_fingerprints.json")


def _backbone():
    return VT.VisionTransformer(img_size=[SIDE], patch_size=PATCH, embed_dim=DIM, depth=DEPTH, num_heads=HEADS, mlp_ratio=4,
                                qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6))


@functools.lru_cache(maxsize=None)
def _states():
    """((student backbone, student head), (teacher backbone, teacher head)) state dicts, the crops, the centre."""
    out = []
    for seed in (31, 32):
        sd = synth.synth_state_dict(DIM, DEPTH, PATCH, seed=seed, variant="full", img_size=SIDE)
        out.append((sd, R.fill_head(R.TwinHead(**HEAD), seed=seed + 10, g_spread=0.1)))
    crops = [synth.synth_tiles(BATCH, SIDE, seed=200 + i) for i in range(2)]
    crops += [synth.synth_tiles(BATCH, LOCAL, seed=210 + i) for i in range(NCROPS - 2)]
    center = 0.2 * torch.randn(1, HEAD["out_dim"], generator=torch.Generator().manual_seed(40))
    return out[0], out[1], crops, center


def _wrapper(state, precision, dev, train):
    sd, head_sd = state
    bb = _backbone()
    assert not bb.load_state_dict(sd, strict=True).missing_keys
    bb.set_precision(precision)
    head = VT.DINOHead(**HEAD)
    head.load_state_dict(head_sd, strict=True)
    head.precision = precision
    if train:
        bb.enable_training()
    return DU.MultiCropWrapper(bb, head).to(dev).train()


def _twin_forward(sd, head, crops):
    """MultiCropWrapper in float64: the encoder per run of equally sized crops, the head on all rows."""
    cfg = O.make_cfg(sd, PATCH, HEADS)
    rows = [R.encoder_cls(sd, cfg, torch.cat([c.double() for c in group])) for group in (crops[:2], crops[2:]) if group]
    return head(torch.cat(rows))


@functools.lru_cache(maxsize=None)
def _reference():
    """(loss64, {student parameter name: grad64}, updated centre64, teacher logits64)."""
    student, teacher, crops, center = _states()
    prm = {k: v.double().clone().requires_grad_(True) for k, v in student[0].items()}
    head = R.TwinHead(**HEAD)
    head.load_state_dict(student[1])
    head = head.double()
    out = _twin_forward(prm, head, crops)
    with torch.no_grad():
        thead = R.TwinHead(**HEAD)
        thead.load_state_dict(teacher[1])
        tout = _twin_forward({k: v.double() for k, v in teacher[0].items()}, thead.double(), crops[:2])
    loss = R.dino_loss(out, tout, center.double().reshape(-1), 0.1, 0.04, NCROPS)
    loss.backward()
    grads = {"backbone." + k: v.grad for k, v in prm.items()}
    grads.update({"head." + n: p.grad for n, p in head.named_parameters() if p.grad is not None})
    new_center = R.center_update(center.double(), tout.sum(0, keepdim=True), tout.shape[0], 0.9)
    return float(loss.detach()), grads, new_center, tout


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_one_step_matches_float64(dev, precision):
    student_sd, teacher_sd, crops, center = _states()
    loss64, grads64, center64, tout64 = _reference()
    student = _wrapper(student_sd, precision, dev, train=True)
    teacher = _wrapper(teacher_sd, precision, dev, train=False)
    for p in teacher.parameters():
        p.requires_grad = False
    criterion = DU.DINOLoss(HEAD["out_dim"], NCROPS, 0.04, 0.07, 3, 10).to(dev)
    criterion.center.copy_(center)
    images = [c.to(dev) for c in crops]
    with torch.no_grad():
        tout = teacher(images[:2])
    assert tout.grad_fn is None and R.rel(tout, tout64) <= FWD_TOL[precision]
    out = student(images)
    assert out.shape == (NCROPS * BATCH, HEAD["out_dim"]) and out.grad_fn is not None
    loss = criterion(out, tout, 0)
    assert abs(float(loss.detach()) - loss64) <= TOL[precision] * abs(loss64)
    assert R.rel(criterion.center, center64) <= TOL[precision]
    loss.backward()
    named = dict(student.named_parameters())
    assert {n for n, p in named.items() if p.grad is not None} == set(grads64)  # (the frozen weight_g has none)
    errs = {n: R.rel(named[n].grad, g64) for n, g64 in grads64.items()}
    print(precision, "loss", float(loss.detach()), loss64, {k: f"{v:.2e}" for k, v in errs.items()})
    worst = max(errs, key=errs.get)
    assert errs[worst] <= TOL[precision], f"{worst}: {errs[worst]:.3e} > {TOL[precision]:.0e}"
    with pytest.raises(RuntimeError, match="backward through the graph a second time"):
        loss.backward()

    # the rest of the step: clip, cancel the last layer's gradients, AdamW, the teacher's EMA
    norms = DU.clip_gradients(student, 3.0)
    assert len(norms) == len(grads64) and all(n > 0 for n in norms)
    DU.cancel_gradients_last_layer(0, student, 1)
    assert student.head.last_layer.weight_v.grad is None
    before = {n: p.detach().clone() for n, p in student.named_parameters()}
    opt = OPT.AdamW(DU.get_params_groups(student), lr=1e-3, weight_decay=0.04)
    opt.step()
    assert all(not torch.equal(before[n], p) for n, p in student.named_parameters() if p.grad is not None)
    assert torch.equal(before["head.last_layer.weight_v"], student.head.last_layer.weight_v)
    want = {n: (t.detach().double() * 0.9 + s.detach().double() * 0.1).cpu()
            for (n, t), s in zip(teacher.named_parameters(), student.parameters())}
    DU.ema_update(list(teacher.parameters()), list(student.parameters()), 0.9)
    for n, p in teacher.named_parameters():
        assert R.rel(p, want[n]) <= 2e-7, n
    # the teacher's next forward runs on the moved weights (its engine and operand copies are rebuilt)
    with torch.no_grad():
        tout2 = teacher(images[:2])
        thead = R.TwinHead(**HEAD)
        thead.load_state_dict({k: v.cpu() for k, v in teacher.head.state_dict().items()})
        sd2 = {k: v.cpu().double() for k, v in teacher.backbone.state_dict().items()}
        tout2_64 = _twin_forward(sd2, thead.double(), crops[:2])
    assert R.rel(tout2, tout2_64) <= FWD_TOL[precision]
    assert R.rel(tout, tout2_64) > 10 * FWD_TOL["bf16x3"]  # (the move is visible at all)


def test_without_the_opt_in_nothing_builds_a_graph(dev):
    student_sd, _, crops, _ = _states()
    bb = _backbone()
    bb.load_state_dict(student_sd[0])
    bb = bb.to(dev).train()
    x = crops[0].to(dev)
    plain = bb(x)
    assert plain.grad_fn is None and bb.training_backward is False and "training_backward" not in bb.state_dict()
    assert bb.enable_training() is bb
    trained = bb(x)
    assert trained.grad_fn is not None and R.rel(trained, plain) <= FWD_TOL["bf16x3"]
    with torch.no_grad():
        assert bb(x).grad_fn is None
    assert bb.eval()(x).grad_fn is None
    bb.train().enable_training(False)
    assert bb(x).grad_fn is None
    bb.enable_training()
    with pytest.raises(NotImplementedError, match="gradient of the input"):
        bb(x.clone().requires_grad_(True))
    narrow = VT.VisionTransformer(img_size=[SIDE], patch_size=PATCH, embed_dim=96, depth=1, num_heads=3).to(dev).train()
    with pytest.raises(NotImplementedError, match="64- or 128-wide heads"):
        narrow.enable_training()(x)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_map_encoders_keep_the_parent_commits_bits(dev, precision):
    """VisionTransformerForFinetune / ForSimMIM, training mode: output and every gradient bit-equal to what the parent commit gave
    (recorded by running it once on an MI355X)."""
    with open(GOLDEN) as f:
        parent = json.load(f)[precision]
    now = R.encoder_fingerprints(dev, precision)
    for kind in ("finetune", "simmim"):
        assert set(now[kind]) == set(parent[kind])
        changed = sorted(k for k in parent[kind] if now[kind][k] != parent[kind][k])
        assert not changed, f"{kind} ({precision}): bits changed in {changed}"
