"""Stochastic depth's module surface (dino/vision_transformer.py), without a GPU: where DropPath sits and with which rates, the
state_dict, draw_drop_path_scales on the CPU generator, drop_path() itself, and the training-mode refusals of _engine (which
come before anything touches a device)."""
from functools import partial

import pytest
import torch
import torch.nn as nn

from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as V

DEPTH, RATE = 5, 0.3
KW = dict(patch_size=8, embed_dim=128, depth=DEPTH, num_heads=2, mlp_ratio=4, qkv_bias=True, img_size=[32],
          norm_layer=partial(nn.LayerNorm, eps=1e-6))


def _vit(cls=V.VisionTransformer, **over):
    kw = dict(KW, **over)
    if cls is not V.VisionTransformer:
        kw["img_size"] = 32
    return cls(**kw)


@pytest.mark.parametrize("cls", [V.VisionTransformer, M.VisionTransformerForSimMIM, M.VisionTransformerForFinetune])
def test_droppath_sits_where_the_reference_has_it(cls):
    m = _vit(cls, drop_path_rate=RATE)
    rates = torch.linspace(0, RATE, DEPTH).tolist()
    assert rates[0] == 0.0
    for blk, r in zip(m.blocks, rates):
        if r > 0:
            assert type(blk.drop_path) is V.DropPath and blk.drop_path.drop_prob == r
            assert not list(blk.drop_path.parameters()) and not list(blk.drop_path.buffers())
        else:
            assert type(blk.drop_path) is nn.Identity
    plain = _vit(cls)
    assert all(type(b.drop_path) is nn.Identity for b in plain.blocks)
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())
    assert "(drop_path): DropPath()" in repr(m)
    # the only DropPath / Identity children are the blocks' drop_path (and the head)
    named = [n for n, mod in m.named_modules() if isinstance(mod, V.DropPath)]
    assert named == [f"blocks.{i}.drop_path" for i in range(1, DEPTH)]


def test_draw_scales_order_values_and_generator_use():
    m = _vit(drop_path_rate=RATE)
    B = 6
    torch.manual_seed(1234)
    scales = V.draw_drop_path_scales(m, B, torch.device("cpu"))
    after = torch.rand(3)
    assert len(scales) == 2 * DEPTH
    torch.manual_seed(1234)
    seen = set()
    for i, blk in enumerate(m.blocks):
        for j in (2 * i, 2 * i + 1):
            if i == 0:
                assert scales[j] is None  # rate 0: an Identity, nothing drawn
                continue
            keep = 1 - blk.drop_path.drop_prob
            want = torch.floor(keep + torch.rand((B, 1, 1), dtype=torch.float32)).reshape(B) / keep  # restated
            assert scales[j].dtype == torch.float32 and scales[j].shape == (B,)
            assert torch.equal(scales[j], want)
            one = torch.tensor(1.0) / keep
            assert all(v in (0.0, float(one)) for v in scales[j].tolist())
            seen.update(v > 0 for v in scales[j].tolist())
    assert torch.equal(after, torch.rand(3))  # exactly 2 (depth - 1) draws of (B, 1, 1) were consumed
    assert seen == {True, False}
    assert V.draw_drop_path_scales(_vit(), B, torch.device("cpu")) == [None] * (2 * DEPTH)


def test_drop_path_function_and_module():
    x = torch.randn(4, 3, 8)
    assert V.drop_path(x, 0.5, training=False) is x
    assert V.drop_path(x, 0.0, training=True) is x
    mod = V.DropPath(0.5)
    assert mod.eval()(x) is x
    torch.manual_seed(3)
    y = mod.train()(x)
    torch.manual_seed(3)
    mask = torch.floor(0.5 + torch.rand(4, 1, 1))
    assert torch.equal(y, x.div(0.5) * mask)
    assert V.drop_path(torch.randn(5, 7), 0.25, True).shape == (5, 7)


@pytest.mark.parametrize("kw", [dict(drop_rate=0.1), dict(attn_drop_rate=0.1), dict(drop_rate=0.1, drop_path_rate=0.1)])
def test_dropout_in_training_mode_is_still_refused(kw):
    m = _vit(**kw).train()
    with pytest.raises(NotImplementedError, match="dropout"):
        m._engine(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="dropout"):
        m._engine(torch.device("cpu"), training_path=True)


def test_drop_path_in_training_mode_is_refused_on_the_engine_path_only():
    m = _vit(drop_path_rate=0.1).train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"\.eval\(\).*enable_training\(\).*enable_finetune\(\)"):
        m._engine(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="drop-path"):
        m._engine(torch.device("cpu"))
    # a free-standing Block applies the reference's formula through its DropPath module
    assert isinstance(m.blocks[-1].drop_path, V.DropPath)
