"""Dropout without a GPU: the generator of csrc/philox.h held to Random123's known answers, from the library's host exports and
from the numpy restatement of tests/dropout_ref.py; the keep mask, the threshold, the keep rate of the definition; the module
surface (enable_dropout, the refusals of _engine, draw_dropout_seeds on the CPU generator); header, export map and binding."""
import ctypes as C
import fnmatch
import math
import os
import re
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import dropout_ref as R
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import model as M
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc")
NEW_SYMBOLS = ["ocm_philox4x32_10", "ocm_dropout_threshold", "ocm_dropout_keep_host", "ocm_op_dropout_mask", "ocm_op_dropout",
               "ocm_op_dropout_layernorm", "ocm_op_dropout_backward", "ocm_op_gelu_dropout", "ocm_op_gelu_dropout_backward"]
# counter, key -> output (Random123's published vectors for philox4x32-10)
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
SEEDS = [0, 1, 61, 2 ** 40 + 7, 2 ** 62 - 1]
RATES = [0.1, 0.25, 0.5]
DEPTH = 3
KW = dict(patch_size=8, embed_dim=128, depth=DEPTH, num_heads=2, mlp_ratio=4, qkv_bias=True, img_size=[32],
          norm_layer=partial(nn.LayerNorm, eps=1e-6))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _vit(cls=V.VisionTransformer, **over):
    kw = dict(KW, **over)
    if cls is not V.VisionTransformer:
        kw["img_size"] = 32
    return cls(**kw)


# ---- the generator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_known_answers(lib, ctr, key, want):
    assert tuple(int(v) for v in R.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))) == want
    out = (C.c_uint32 * 4)()
    lib.ocm_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out)
    assert tuple(out) == want


def _keep_host(lib, seed, first, count, thresh):
    keep = np.full(count + 2, 7, dtype=np.uint8)  # a guard byte on either side
    rc = lib.ocm_dropout_keep_host(seed, first, count, thresh, C.c_void_p(keep.ctypes.data + 1))
    assert rc == 0, lib.ocm_last_error()
    assert keep[0] == 7 and keep[-1] == 7
    return keep[1:-1]


@pytest.mark.parametrize("seed", SEEDS)
def test_keep_host_equals_the_numpy_mask(lib, seed):
    thresh, _ = R.threshold(0.25)
    for count in (1, 3, 4, 5, 4099):
        assert np.array_equal(_keep_host(lib, seed, 0, count, thresh), R.keep_mask(seed, count, thresh)), count
    whole = R.keep_mask(seed, 64, thresh)
    for first, count in ((1, 2), (2, 4), (3, 1), (3, 2), (5, 9), (7, 1), (6, 13), (2 ** 34 + 3, 6)):  # across groups of four
        got = _keep_host(lib, seed, first, count, thresh)
        assert np.array_equal(got, R.keep_mask(seed, count, thresh, first=first)), (first, count)
        if first + count <= 64:
            assert np.array_equal(got, whole[first:first + count]), (first, count)
    assert 0 < int(R.keep_mask(seed, 4099, thresh).sum()) < 4099


def test_the_key_and_the_counter_use_both_halves():
    """Seeds that differ above bit 32 only, and groups that differ above bit 32 only, give different words."""
    assert not np.array_equal(R.words(7, 0, 16), R.words(2 ** 40 + 7, 0, 16))
    assert not np.array_equal(R.words(7, 0, 16), R.words(7, 2 ** 34, 16))
    ctr = np.array([[5, 1, 0, 0]], dtype=np.uint64)  # group 2^32 + 5
    key = np.array([[7, 0]], dtype=np.uint64)
    assert np.array_equal(R.words(7, 4 * (2 ** 32 + 5), 4), R.philox4x32_10(ctr, key)[0])


def test_threshold_and_its_refusals(lib):
    for p, thresh in ((0.1, 429496730), (0.25, 1 << 30), (0.5, 1 << 31)):
        th, ik = C.c_uint32(), C.c_float()
        assert lib.ocm_dropout_threshold(p, C.byref(th), C.byref(ik)) == 0
        assert th.value == thresh == R.threshold(p)[0] == math.floor(p * 2 ** 32 + 0.5)
        assert np.float32(ik.value) == R.threshold(p)[1] == np.float32(1.0 / (1.0 - p))
    th, ik = C.c_uint32(5), C.c_float(5.0)
    for p in (0.0, 1.0, -0.1, float("nan")):
        assert lib.ocm_dropout_threshold(p, C.byref(th), C.byref(ik)) == _lib.OCM_EINVAL, p
    assert th.value == 5 and ik.value == 5.0
    assert lib.ocm_dropout_threshold(0.5, None, C.byref(ik)) == _lib.OCM_EINVAL
    assert lib.ocm_dropout_keep_host(-1, 0, 4, 1 << 31, C.c_void_p(np.zeros(4, np.uint8).ctypes.data)) == _lib.OCM_EINVAL
    assert lib.ocm_dropout_keep_host(1, 0, 0, 1 << 31, C.c_void_p(np.zeros(4, np.uint8).ctypes.data)) == _lib.OCM_EINVAL
    assert lib.ocm_dropout_keep_host(1, 0, 4, 1 << 31, None) == _lib.OCM_EINVAL


def test_keep_rate_of_the_definition():
    """The dropped fraction of the reference masks at the tensors of the training test (4 x 65 x 32 / x 128 / x 512 elements) is
    within 4 sigma of p, sigma = sqrt(p (1 - p) / count). Computed from the definition, the worst of the 45 cases is 2.38 sigma."""
    worst = 0.0
    for seed in SEEDS:
        for count in (8320, 33280, 133120):
            w = R.words(seed, 0, count)
            for p in RATES:
                dropped = float((w < np.uint32(R.threshold(p)[0])).mean())
                z = abs(dropped - p) / math.sqrt(p * (1 - p) / count)
                worst = max(worst, z)
                assert z <= 4.0, (seed, count, p, z)
    print(f"dropout keep rate: worst of 45 cases {worst:.2f} sigma")


def test_factors_are_zero_or_inv_keep():
    f = R.factors(61, 4099, 0.1)
    assert f.dtype == np.float32 and set(np.unique(f).tolist()) == {0.0, float(np.float32(1.0 / 0.9))}


# ---- the opt-in ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(drop_rate=0.1), dict(attn_drop_rate=0.1), dict(drop_rate=0.1, drop_path_rate=0.1)])
def test_without_the_opt_in_the_refusals_stand(kw):
    m = _vit(**kw).train()
    assert m.dropout_enabled is False
    for tp in (False, True):
        with pytest.raises(NotImplementedError, match=r"dropout.*enable_dropout\(\)"):
            m._engine(torch.device("cpu"), training_path=tp)
    m.enable_dropout().enable_dropout(False)
    with pytest.raises(NotImplementedError, match="dropout"):
        m._engine(torch.device("cpu"), training_path=True)


@pytest.mark.parametrize("cls", [V.VisionTransformer, M.VisionTransformerForSimMIM, M.VisionTransformerForFinetune])
def test_enable_dropout_is_a_plain_attribute(cls):
    plain, m = _vit(cls), _vit(cls, drop_rate=0.1)
    assert m.enable_dropout() is m and m.dropout_enabled is True
    assert list(m.state_dict().keys()) == list(plain.state_dict().keys())
    assert "dropout_enabled" not in dict(m.named_buffers()) and "dropout_enabled" not in dict(m.named_parameters())
    assert m.enable_dropout(False).dropout_enabled is False


def test_attention_dropout_stays_refused_with_the_opt_in():
    m = _vit(attn_drop_rate=0.1).enable_dropout().train()
    for tp in (False, True):
        with pytest.raises(NotImplementedError, match="dropout"):
            m._engine(torch.device("cpu"), training_path=tp)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        V.dropout_site_rates(m)


def test_off_the_training_path_training_mode_is_refused():
    m = _vit(drop_rate=0.1).enable_dropout().train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match=r"\.eval\(\).*enable_training\(\).*enable_finetune\(\)"):
        m._engine(torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="dropout"):
        m._engine(torch.device("cpu"))


@pytest.mark.parametrize("rate", [1.0, 1.5, -0.5])
def test_a_rate_outside_the_unit_interval_is_a_value_error(rate):
    m = _vit(drop_rate=0.1).enable_dropout().train()
    m.blocks[1].mlp.drop.p = rate  # rates are read at call time from the modules that hold them
    for tp in (False, True):
        with pytest.raises(ValueError, match="dropout rate"):
            m._engine(torch.device("cpu"), training_path=tp)
    if rate == 1.0:
        one = _vit(drop_rate=1.0).enable_dropout().train()
        with pytest.raises(ValueError, match="dropout rate"):
            one._engine(torch.device("cpu"), training_path=True)


def test_site_rates_are_read_from_the_modules():
    m = _vit(drop_rate=0.1)
    assert V.dropout_site_rates(m) == [0.1] * (1 + 3 * DEPTH)
    m.pos_drop.p, m.blocks[0].attn.proj_drop.p, m.blocks[2].mlp.drop.p = 0.0, 0.2, 0.3
    assert V.dropout_site_rates(m) == [0.0, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.3, 0.3]


def test_draw_dropout_seeds_is_one_draw():
    m = _vit(drop_rate=0.1)
    torch.manual_seed(77)
    seeds = V.draw_dropout_seeds(m, torch.device("cpu"))
    after = torch.rand(3)
    torch.manual_seed(77)
    want = torch.randint(0, 2 ** 62, (1 + 3 * DEPTH,), dtype=torch.int64)
    assert seeds.dtype == torch.int64 and torch.equal(seeds, want) and bool((seeds >= 0).all())
    assert torch.equal(after, torch.rand(3))  # exactly that one draw was consumed
    plain, paths = _vit(), _vit(drop_path_rate=0.3)  # (building a model draws its initial weights)
    torch.manual_seed(77)
    assert V.draw_dropout_seeds(plain, torch.device("cpu")) is None
    assert V.draw_dropout_seeds(paths, torch.device("cpu")) is None
    assert torch.equal(torch.randint(0, 2 ** 62, (1 + 3 * DEPTH,), dtype=torch.int64), want)  # rate 0 drew nothing
    one = _vit()
    one.blocks[1].attn.proj_drop.p = 0.2  # a single site above 0: still the whole vector
    assert V.draw_dropout_seeds(one, torch.device("cpu")).shape == (1 + 3 * DEPTH,)


def test_builders_do_not_opt_in():
    import inspect
    for fn in (M.build_finetune_model, M.build_model):
        assert "enable_dropout" not in inspect.getsource(fn)


# ---- header, export map, binding ----------------------------------------------------------------------------------------------------
def test_header_export_map_and_binding_agree(lib):
    with open(os.path.join(ROOT, "include", "ocm_vit.h")) as f:
        header = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    with open(os.path.join(CSRC, "exports.map")) as f:
        patterns = re.findall(r"global:\s*([^;]+);", f.read())
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for p in patterns), name
        assert getattr(lib, name) is not None  # bound: the built library exports it
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION == 20
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "kernels_dropout.hip" in make and "philox.h" in make
    src = open(os.path.join(CSRC, "kernels_dropout.hip")).read()
    assert "#pragma clang fp contract(off)" in src
