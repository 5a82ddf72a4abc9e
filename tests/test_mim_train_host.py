"""The SimMIM training path's refusals, which happen before anything is launched (no GPU needed)."""
from functools import partial

import pytest
import torch
import torch.nn as nn

from vit_ocm_wmsegmentation_amd import model as M


def _mim(dim, heads):
    enc = M.VisionTransformerForSimMIM(patch_size=8, embed_dim=dim, depth=1, num_heads=heads, mlp_ratio=4, img_size=[32],
                                       qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)
    return M.MIM(enc, 8).train()


def _inputs(requires_grad=False):
    x = torch.zeros(1, 3, 32, 32, requires_grad=requires_grad)
    return x, torch.zeros(1, 4, 4, dtype=torch.int64)


def test_head_width_48_is_refused():
    mim = _mim(192, 4)  # 48-wide heads
    with pytest.raises(NotImplementedError, match="64- or 128-wide heads"):
        mim(*_inputs())
    with pytest.raises(NotImplementedError, match="64- or 128-wide heads"):
        mim.encoder(*_inputs())


def test_input_gradient_is_refused():
    mim = _mim(128, 2)
    with pytest.raises(NotImplementedError, match="gradient of the input"):
        mim(*_inputs(requires_grad=True))


def test_frozen_encoder_with_unsupported_heads_is_not_refused_for_its_width():
    """A frozen encoder is not differentiated: its head width does not matter (the decoder alone trains)."""
    mim = _mim(192, 4)
    for p in mim.encoder.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="HIP device"):
        mim(*_inputs())


@pytest.mark.parametrize("side", [2, 8])
def test_mask_of_the_wrong_size_is_refused(side):
    """The kernels read one mask entry per patch of every image: a mask for another grid is refused as the eval path refuses it."""
    mim = _mim(128, 2)
    x, _ = _inputs()
    bad = torch.zeros(1, side, side, dtype=torch.int64)
    with pytest.raises(ValueError, match="entries per image, expected 16"):
        mim(x, bad)
    with pytest.raises(ValueError, match="entries per image, expected 16"):
        mim.encoder(x, bad)
