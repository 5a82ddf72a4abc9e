"""The Swin forward on every geometry class ocm_swin_create accepts (tests/golden_cases.py SWIN_GEOMETRIES: embed_dim 32 .. 128,
windows 2 .. 7, 1 .. 4 stages, one and three channels, mlp_ratio 1 .. 4, ln_eps 1e-6 .. 1e-3, 1 .. 1000 labels), in every
precision and, for split-bf16, with the fused kernels on and off (OCM_SWIN_OPT_FUSE_MLP), against the float64 oracle
(oracle/swin_oracle.py, pinned to transformers by tests/test_swin.py) on the same synthetic weights.

Logits, pooler_output and the WHOLE last_hidden_state (every token and channel) are compared: a dropped shift mask or a
wrong eps moves the logits by less than the split-bf16 logit bar of tests/test_swin.py but the hidden state by 1e-2 and more
(tests/test_swin_sensitivity.py holds the bounds below against such planted changes). fp32 and split-bf16 bounds are set from
measurement with up to ~4x headroom. Single bf16 rounds every GEMM operand to 8 bits of mantissa: its bounds are a sanity
check (finite, the right magnitude, no layout error), not an accuracy claim.
"""
import pytest
import torch

from oracle import swin_oracle as SO
from tests.golden_cases import SWIN_GEOMETRIES
from vit_ocm_wmsegmentation_amd import _lib, synth
from vit_ocm_wmsegmentation_amd import swin as SW

# max |GPU - float64 oracle| per mode: (logits, pooler_output, last_hidden_state). Largest measured on MI355X over the eight
# geometries (and both fuse settings): fp32 2.1e-6 / 3.7e-6 / 7.3e-6, split-bf16 1.7e-5 / 2.7e-5 / 5.4e-5, bf16 1.0e-2 / 1.8e-2 /
# 2.7e-2, each at F (1024 channels, 1000 labels) but the split-bf16 hidden state (F 5.4e-5, E 4.9e-5); DESIGN §3.7 lists them all.
BOUNDS = {
    "fp32": (6e-6, 1e-5, 2e-5),
    "bf16x3": (5e-5, 8e-5, 1.5e-4),
    "bf16": (3e-2, 5e-2, 8e-2),  # sanity only
}

_ORACLE = {}


def geometry_case(name, dtype=torch.float32):
    """(cfg, state_dict, pixel_values) of a SWIN_GEOMETRIES entry, weights and tiles in `dtype`."""
    c = SWIN_GEOMETRIES[name]
    cfg = dict(synth.SWIN_TINY, **c["cfg"])
    sd = {k: v.to(dtype) for k, v in synth.synth_swin_state_dict(cfg, seed=c["seed"], qk_gain=c["qk_gain"]).items()}
    x = synth.synth_tiles(c["batch"], cfg["image_size"], seed=c["seed"] + 50, channels=cfg["num_channels"]).to(dtype)
    return cfg, sd, x


def _oracle(name):
    """The float64 oracle's outputs for a geometry, computed once per module run."""
    if name not in _ORACLE:
        cfg, sd, x = geometry_case(name, torch.float64)
        o = SO.swin_forward(sd, cfg, x)
        _ORACLE[name] = {k: o[k] for k in ("logits", "pooled", "last_hidden_state")}
    return _ORACLE[name]


@pytest.mark.gpu
@pytest.mark.parametrize("precision,fuse", [("fp32", None), ("bf16x3", 1), ("bf16x3", 0), ("bf16", None)])
@pytest.mark.parametrize("name", sorted(SWIN_GEOMETRIES))
def test_swin_geometry_vs_float64_oracle(lib, dev, name, precision, fuse):
    cfg, sd, x = geometry_case(name)
    want = _oracle(name)
    hf = SW.SwinConfig(image_size=cfg["image_size"], num_channels=cfg["num_channels"], embed_dim=cfg["embed_dim"],
                       depths=cfg["depths"], num_heads=cfg["num_heads"], window_size=cfg["window_size"],
                       mlp_ratio=cfg["mlp_ratio"], layer_norm_eps=cfg["layer_norm_eps"], num_labels=cfg["num_labels"])
    model = SW.SwinForImageClassification(hf)
    msg = model.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    model = model.to(dev).eval().set_precision(precision)
    if fuse is not None:
        _lib.check(lib.ocm_swin_set_option(model._get_engine(dev)["h"], _lib.OCM_SWIN_OPT_FUSE_MLP, fuse))
    out = model(pixel_values=x.to(dev), output_hidden_states=True)
    got = {"logits": out.logits, "pooled": out.pooler_output, "last_hidden_state": out.last_hidden_state}
    err = {}
    for k, t in got.items():
        assert tuple(t.shape) == tuple(want[k].shape), k
        t = t.cpu().double()
        assert torch.isfinite(t).all(), k
        err[k] = (t - want[k]).abs().max().item()
    tag = precision + ("" if fuse is None else f" fuse{fuse}")
    print(f"GPUTEST swin geometry {name} {tag}: logits {err['logits']:.2e}, pooled {err['pooled']:.2e}, "
          f"hidden {err['last_hidden_state']:.2e}")
    bl, bp, bh = BOUNDS[precision]
    assert err["logits"] <= bl and err["pooled"] <= bp and err["last_hidden_state"] <= bh, err
