"""The Swin accuracy bounds of tests/test_swin_geometry_gpu.py can see the bugs they exist for (CPU only).

Each case plants one plausible Swin mistake into the float64 oracle (by patching one of its helpers, or by a changed config
or weights: the oracle itself is not copied) and asserts that it moves last_hidden_state by at least five times the
split-bf16 hidden bound. A kernel with that mistake would then fail the GPU test however its rounding fell.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from oracle import swin_oracle as SO
from tests.test_swin_geometry_gpu import BOUNDS, geometry_case


class _Proxy:
    """A module whose attributes are the wrapped module's, except those given."""

    def __init__(self, module, **overrides):
        self._module, self._overrides = module, overrides

    def __getattr__(self, name):
        return self._overrides[name] if name in self._overrides else getattr(self._module, name)


@contextlib.contextmanager
def _patched(name, value):
    old = getattr(SO, name)
    setattr(SO, name, value)
    try:
        yield
    finally:
        setattr(SO, name, old)


def _no_shift_mask():
    return _patched("shift_mask", lambda *a, **k: None)


def _transposed_relative_position_index():
    rpi = SO.relative_position_index
    return _patched("relative_position_index", lambda ws: rpi(ws).t().contiguous())


def _fixed_eps_from_config(cfg):
    """Embedding and patch-merging LayerNorms take the config eps instead of transformers' fixed 1e-5."""
    eps = cfg["layer_norm_eps"]
    assert eps != 1e-5
    return _patched("F", _Proxy(F, layer_norm=lambda x, shape, w, b, e: F.layer_norm(x, shape, w, b, eps if e == 1e-5 else e)))


def _pad_before_layernorm():
    """SwinLayer.maybe_pad applied to x before layernorm_before: the padded positions hold LayerNorm(0) = beta, not 0."""
    layer = SO.swin_layer

    def swin_layer(sd, pre, x, H, W, *args):
        beta = sd[pre + "layernorm_before.bias"]

        def pad(y, p):
            y = F.pad(y, p)
            y[:, H:, :, :] = beta
            y[:, :, W:, :] = beta
            return y

        with _patched("F", _Proxy(F, pad=pad)):
            return layer(sd, pre, x, H, W, *args)

    return _patched("swin_layer", swin_layer)


def _merge_order_permuted():
    """Patch merging concatenates x0 | x2 | x1 | x3 (rows and columns of the 2 x 2 neighbourhood swapped)."""
    def cat(ts, dim=0):
        return torch.cat([ts[i] for i in (0, 2, 1, 3)] if len(ts) == 4 else ts, dim=dim)

    return _patched("torch", _Proxy(torch, cat=cat))


def _tanh_gelu():
    return _patched("F", _Proxy(F, gelu=lambda x: F.gelu(x, approximate="tanh")))


# name: (geometry, how the planted run differs). Geometry A: padded grids, shifted windows, one patch merging and config eps
# 1e-3. tanh-GELU differs from erf-GELU by < 2e-4 on the pre-activations of the synthetic weights (|x| < 1): on D with
# fc1 and fc2 weights x4 (pre-activations of a few units) it moves the hidden state by 1.5e-3.
PLANTED = {
    "shift_mask_dropped": ("A", "patch", _no_shift_mask),
    "relative_position_index_transposed": ("A", "patch", _transposed_relative_position_index),
    "config_eps_replaced_by_1e-5": ("A", "cfg", None),
    "fixed_1e-5_replaced_by_config_eps": ("A", "patch_cfg", _fixed_eps_from_config),
    "padding_before_layernorm_before": ("A", "patch", _pad_before_layernorm),
    "patch_merging_concat_permuted": ("A", "patch", _merge_order_permuted),
    "tanh_gelu": ("D", "mlp_gain", _tanh_gelu),
}


@pytest.mark.parametrize("planted", sorted(PLANTED))
def test_split_bf16_hidden_bound_sees_planted_change(planted):
    name, kind, make = PLANTED[planted]
    cfg, sd, x = geometry_case(name, torch.float64)
    if kind == "mlp_gain":
        sd = {k: v * 4 if k.endswith(("mlp.fc1.weight", "mlp.fc2.weight")) else v for k, v in sd.items()}
    want = SO.swin_forward(sd, cfg, x)["last_hidden_state"]
    if kind == "cfg":
        got = SO.swin_forward(sd, dict(cfg, layer_norm_eps=1e-5), x)["last_hidden_state"]
    else:
        with make(cfg) if kind == "patch_cfg" else make():
            got = SO.swin_forward(sd, cfg, x)["last_hidden_state"]
    moved = (got - want).abs().max().item()
    bound = BOUNDS["bf16x3"][2]
    print(f"planted {planted} on {name}: last_hidden_state moves {moved:.2e} (split-bf16 bound {bound:.1e})")
    assert moved >= 5 * bound
    # the planted change is gone again: the helpers are restored
    assert torch.equal(SO.swin_forward(sd, cfg, x)["last_hidden_state"], want)
