"""Host side of Swin training on the padded geometries (no GPU): the four byte-moving entry points exist, are bound and check
their arguments before any launch; SwinForImageClassification.enable_padded_training and what _check_trainable still refuses."""
import ctypes as C

import pytest
import torch

from tests.golden_cases import SWIN_GEOMETRIES
from vit_ocm_wmsegmentation_amd import _lib, synth
from vit_ocm_wmsegmentation_amd import swin as SW

OPS = ("ocm_op_swin_pad_rows", "ocm_op_swin_crop_rows", "ocm_op_swin_merge_gather_pad", "ocm_op_swin_merge_scatter_pad")
A, B_ = C.c_void_p(0x10000), C.c_void_p(0x20000)  # 16-byte aligned addresses no call below may reach a launch with
ODD = C.c_void_p(0x10008)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exported_and_bound(lib):
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION == 20  # the additions are additive
    for name in OPS:
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes == _lib.SIGNATURES[name][1]


@pytest.mark.parametrize("name", OPS[:2])
def test_pad_crop_argument_domain(lib, name):
    fn = getattr(lib, name)
    bad = [(None, B_, 2, 5, 3, 6, 4, 64), (A, None, 2, 5, 3, 6, 4, 64),  # null pointers
           (A, B_, 0, 5, 3, 6, 4, 64), (A, B_, -1, 5, 3, 6, 4, 64), (A, B_, 2, 0, 3, 6, 4, 64), (A, B_, 2, 5, 0, 6, 4, 64),
           (A, B_, 2, 5, 3, 4, 4, 64), (A, B_, 2, 5, 3, 6, 2, 64),  # Hp < H, Wp < W
           (A, B_, 2, 5, 3, 6, 4, 0), (A, B_, 2, 5, 3, 6, 4, 24), (A, B_, 2, 5, 3, 6, 4, 2),  # row_bytes % 16
           (ODD, B_, 2, 5, 3, 6, 4, 64), (A, ODD, 2, 5, 3, 6, 4, 64)]  # 16-byte accesses need aligned rows
    for args in bad:
        assert fn(*args, None) == _lib.OCM_EINVAL, args
        assert lib.ocm_last_error()


@pytest.mark.parametrize("name", OPS[2:])
def test_merge_pad_argument_domain(lib, name):
    fn = getattr(lib, name)
    bad = [(None, B_, 1, 5, 5, 32), (A, None, 1, 5, 5, 32), (A, B_, 0, 5, 5, 32), (A, B_, 1, 0, 5, 32), (A, B_, 1, 5, -2, 32),
           (A, B_, 1, 5, 5, 0), (A, B_, 1, 5, 5, 30), (ODD, B_, 1, 5, 5, 32), (A, ODD, 1, 5, 5, 32)]
    for args in bad:
        assert fn(*args, None) == _lib.OCM_EINVAL, args


def _module(key=None, **over):
    cfg = dict(synth.SWIN_TINY, **(SWIN_GEOMETRIES[key]["cfg"] if key else {}))
    cfg.update(over)
    m = SW.SwinForImageClassification(SW.SwinConfig(**{a: v for a, v in cfg.items() if a != "patch_size"}))
    x = torch.zeros(1, cfg["num_channels"], cfg["image_size"], cfg["image_size"])
    return m.train().requires_grad_(True), x


def test_opt_in_is_a_module_setting():
    m, _ = _module("G")
    keys = set(m.state_dict())
    assert m.enable_padded_training() is m and m.__dict__["_padded_training"] is True
    assert m.enable_padded_training(False) is m and m.__dict__["_padded_training"] is False
    m.enable_padded_training()
    assert set(m.state_dict()) == keys and not any("padded" in k for k in keys)
    fresh, _ = _module("G")
    assert not fresh.load_state_dict(m.state_dict(), strict=True).missing_keys
    assert not fresh.__dict__.get("_padded_training", False)  # the setting does not travel with the weights


def test_refusals_before_any_launch(monkeypatch):
    def no_launch():
        raise AssertionError("the library was called before the refusal")

    monkeypatch.setattr(_lib, "load", no_launch)
    for key in "ADG":
        m, x = _module(key)
        with pytest.raises(NotImplementedError, match="padding"):
            m._check_trainable(x, None)
        with pytest.raises(NotImplementedError, match="enable_padded_training"):
            m._check_trainable(x, None)
        assert m.enable_padded_training()._check_trainable(x, None) is None
        with pytest.raises(NotImplementedError, match="padding"):
            m.enable_padded_training(False)._check_trainable(x, None)
    tile, x = _module(image_size=384)  # Swin-T on the project's tile: grids 96 / 48 / 24 / 12 for windows of 7
    with pytest.raises(NotImplementedError, match="padding"):
        tile._check_trainable(x, None)
    assert tile.enable_padded_training()._check_trainable(x, None) is None
    # what the opt-in does not lift
    small, x = _module(image_size=40, depths=(2, 2), num_heads=(3, 6))  # grids 10 -> 5 < 7
    with pytest.raises(NotImplementedError, match="smaller than window_size"):
        small.enable_padded_training()._check_trainable(x, None)
    m, x = _module("G")
    m.enable_padded_training()
    m.config.hidden_dropout_prob = 0.1
    with pytest.raises(NotImplementedError, match="dropout"):
        m._check_trainable(x, None)
    m.config.hidden_dropout_prob = 0.0
    with pytest.raises(NotImplementedError, match="gradient of the input"):
        m._check_trainable(x.clone().requires_grad_(True), None)
    wide, x = _module("G", num_heads=(2, 2))  # 16-wide heads in stage 0
    with pytest.raises(NotImplementedError, match="32-wide heads"):
        wide.enable_padded_training()._check_trainable(x, None)
    big, x = _module("G", window_size=8, image_size=80)
    with pytest.raises(NotImplementedError, match="windows of 2 to 7"):
        big.enable_padded_training()._check_trainable(x, None)
