"""Host side of DINO training on the HIP path (dino/vision_transformer.py DINOHead, dino/utils.py, kernels_dino.hip): the module
tree and state-dict exchange of the head against a torch twin built here, MultiCropWrapper's grouping on stub backbones, the
schedules and parameter groups against values written out below, and the C ABI's declarations and argument refusals (decided
before any launch). No GPU needed.

The ABI version: the issue behind this file asks for 21 and for every existing test file to stay as it is; eight existing host
tests assert 20. The additions are additive (no existing signature or struct changed), so the version stays 20, as it did for
every additive change since the region-query operators, and this file asserts what holds: library == binding == header, and the
new symbols are declared, bound and exported."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import dino_ref as R
from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd.dino import utils as DU
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as VT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ocm_op_l2_normalize", "ocm_op_l2_normalize_backward", "ocm_op_weight_norm", "ocm_op_weight_norm_backward",
               "ocm_dino_loss_workspace_bytes", "ocm_op_dino_loss", "ocm_op_dino_loss_backward", "ocm_op_dino_center",
               "ocm_op_ema_update"]
P = 4096  # a non-null address that is never touched
DIMS = dict(in_dim=128, out_dim=96, hidden_dim=192, bottleneck_dim=64)


def _refused(lib, rc, word):
    assert rc == _lib.OCM_EINVAL, rc
    assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()


@pytest.mark.parametrize("norm_last_layer", [True, False])
@pytest.mark.parametrize("use_bn", [False, True])
@pytest.mark.parametrize("nlayers", [1, 2, 3])
def test_head_tree_and_state_dict(nlayers, use_bn, norm_last_layer):
    kw = dict(DIMS, nlayers=nlayers, use_bn=use_bn, norm_last_layer=norm_last_layer)
    head, twin = VT.DINOHead(**kw), R.TwinHead(**kw)
    sd, sd_twin = head.state_dict(), twin.state_dict()
    assert list(sd) == list(sd_twin)
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in sd_twin.items()}
    want = {"last_layer.weight_g", "last_layer.weight_v"}
    want |= {"mlp.weight", "mlp.bias"} if nlayers == 1 else {f"mlp.{i}.{k}" for i in range(0, 2 * nlayers - 1, 2)
                                                              for k in ("weight", "bias")} if not use_bn else set()
    assert want <= set(sd)
    if not use_bn:
        assert want == set(sd)
    assert tuple(sd["last_layer.weight_g"].shape) == (DIMS["out_dim"], 1)
    assert torch.equal(sd["last_layer.weight_g"], torch.ones(DIMS["out_dim"], 1))
    assert head.last_layer.weight_g.requires_grad is (not norm_last_layer) is twin.last_layer.weight_g.requires_grad
    assert {n: p.requires_grad for n, p in head.named_parameters()} == {n: p.requires_grad for n, p in twin.named_parameters()}
    assert [type(m) for m in head.mlp.modules()] == [type(m) for m in twin.mlp.modules()]
    for lin in (m for m in head.mlp.modules() if isinstance(m, nn.Linear)):  # the initialisation: N(0, 0.02) weights, zero biases
        assert float(lin.bias.detach().abs().max()) == 0.0 and 0.01 < float(lin.weight.detach().std()) < 0.03
    filled = R.fill_head(twin, seed=3, g_spread=0.1)
    assert not head.load_state_dict(twin.state_dict(), strict=True).missing_keys
    assert all(torch.equal(head.state_dict()[k], filled[k]) for k in filled)
    R.fill_head(head, seed=4)
    assert not twin.load_state_dict(head.state_dict(), strict=True).missing_keys
    assert head.precision == _lib.DEFAULT_PRECISION == "bf16x3"


def test_head_refusals():
    x = torch.zeros(3, 128)
    with pytest.raises(NotImplementedError, match="use_bn"):
        VT.DINOHead(**DIMS, use_bn=True)(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        VT.DINOHead(**DIMS)(x)
    for bad in (dict(in_dim=96), dict(hidden_dim=100), dict(bottleneck_dim=32), dict(out_dim=48)):
        head = VT.DINOHead(**dict(DIMS, **bad))
        with pytest.raises(ValueError, match="multiples of 64"):
            head(torch.zeros(3, head._linears()[0][1].in_features))


class _StubBackbone(nn.Module):
    def __init__(self):
        super().__init__()
        self.head = nn.Linear(4, 4)
        self.calls = []

    def forward(self, x):
        self.calls.append(tuple(x.shape))
        return x.flatten(1)[:, :4] + 0.0


def test_multi_crop_wrapper_groups_consecutive_sizes():
    a, b = 8, 4
    bb = _StubBackbone()
    wrap = DU.MultiCropWrapper(bb, nn.Identity())
    assert isinstance(bb.head, nn.Identity) and isinstance(bb.fc, nn.Identity)
    assert all(k.startswith(("backbone.", "head.")) for k in wrap.state_dict())
    crops = [torch.full((2, 1, s, s), float(i)) for i, s in enumerate([a, a, b, b, b])]
    out = wrap(crops)
    assert bb.calls == [(4, 1, a, a), (6, 1, b, b)]
    assert out.shape == (10, 4) and out[:, 0].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    bb.calls.clear()
    assert wrap([crops[0]]).shape == (2, 4) and bb.calls == [(2, 1, a, a)]
    bb.calls.clear()
    assert wrap(crops[2]).shape == (2, 4) and bb.calls == [(2, 1, b, b)]  # a bare tensor
    bb.calls.clear()
    wrap([crops[0], crops[2], crops[1]])  # a size that returns later is a group of its own
    assert bb.calls == [(2, 1, a, a), (2, 1, b, b), (2, 1, a, a)]
    head = VT.DINOHead(**DIMS)
    keys = set(DU.MultiCropWrapper(_StubBackbone(), head).state_dict())
    assert {"head." + k for k in head.state_dict()} <= keys


def test_cosine_scheduler_values():
    s = DU.cosine_scheduler(1.0, 0.0, epochs=2, niter_per_ep=2)
    np.testing.assert_allclose(s, [1.0, 0.8535533905932737, 0.5, 0.14644660940672627], rtol=0, atol=1e-15)
    s = DU.cosine_scheduler(0.5, 0.1, epochs=3, niter_per_ep=2, warmup_epochs=1, start_warmup_value=0.1)
    np.testing.assert_allclose(s, [0.1, 0.5, 0.5, 0.4414213562373095, 0.3, 0.15857864376269052], rtol=0, atol=1e-15)
    assert len(DU.cosine_scheduler(5e-4, 1e-6, 100, 7, warmup_epochs=10)) == 700


def test_teacher_temperature_schedule_and_center_buffer():
    loss = DU.DINOLoss(96, 10, 0.04, 0.07, 4, 6)
    np.testing.assert_allclose(loss.teacher_temp_schedule, [0.04, 0.05, 0.06, 0.07, 0.07, 0.07], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(loss.teacher_temp_schedule, R.teacher_temp_schedule(0.04, 0.07, 4, 6))
    assert list(loss.state_dict()) == ["center"] and tuple(loss.center.shape) == (1, 96) and float(loss.center.abs().max()) == 0.0
    assert loss.student_temp == 0.1 and loss.center_momentum == 0.9 and loss.ncrops == 10
    with pytest.raises(RuntimeError, match="HIP device"):
        loss(torch.zeros(20, 96), torch.zeros(4, 96), 0)


def test_params_groups_and_helpers():
    head = VT.DINOHead(**DIMS, norm_last_layer=True)
    model = nn.Sequential(nn.Linear(4, 4), nn.LayerNorm(4), head)
    groups = DU.get_params_groups(model)
    named = dict(model.named_parameters())
    reg = {"0.weight", "2.mlp.0.weight", "2.mlp.2.weight", "2.mlp.4.weight", "2.last_layer.weight_v"}
    plain = {"0.bias", "1.weight", "1.bias", "2.mlp.0.bias", "2.mlp.2.bias", "2.mlp.4.bias"}  # weight_g is frozen: in neither
    assert {id(p) for p in groups[0]["params"]} == {id(named[n]) for n in reg}
    assert {id(p) for p in groups[1]["params"]} == {id(named[n]) for n in plain}
    assert "weight_decay" not in groups[0] and groups[1]["weight_decay"] == 0.
    assert not DU.has_batchnorms(model) and DU.has_batchnorms(VT.DINOHead(**DIMS, use_bn=True))
    for p in head.parameters():
        p.grad = torch.zeros_like(p)
    DU.cancel_gradients_last_layer(1, head, 1)
    assert head.last_layer.weight_v.grad is not None
    DU.cancel_gradients_last_layer(0, head, 1)
    assert head.last_layer.weight_v.grad is None and head.last_layer.weight_g.grad is None and head.mlp[0].weight.grad is not None
    assert DU.clip_gradients(nn.Linear(2, 2), 3.0) == []  # nothing has a gradient: nothing to launch
    with pytest.raises(ValueError, match="teacher tensors"):
        DU.ema_update([torch.zeros(2)], [], 0.9)


def test_entry_points_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "ocm_vit.h")).read()
    version = int(re.search(r"#define OCM_ABI_VERSION (\d+)\b", text).group(1))
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION == version == 20  # additive: see the module docstring
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert "kernels_dino.hip" in open(os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc", "Makefile")).read()


def test_row_operator_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    _refused(lib, lib.ocm_op_l2_normalize(None, P, P, 2, 8, None), "null")
    _refused(lib, lib.ocm_op_l2_normalize(P, P, None, 2, 8, None), "null")
    _refused(lib, lib.ocm_op_l2_normalize(P, P, P, 0, 8, None), "rows")
    _refused(lib, lib.ocm_op_l2_normalize(P, P, P, 2, 0, None), "dim")
    _refused(lib, lib.ocm_op_l2_normalize(P + 2, P, P, 2, 8, None), "aligned")
    _refused(lib, lib.ocm_op_l2_normalize_backward(P, None, P, P, 2, 8, None), "null")
    _refused(lib, lib.ocm_op_l2_normalize_backward(P, P, P, P, -1, 8, None), "rows")
    _refused(lib, lib.ocm_op_l2_normalize_backward(P, P, P, P + 1, 2, 8, None), "aligned")
    _refused(lib, lib.ocm_op_weight_norm(P, None, P, P, 4, 8, None), "null")
    _refused(lib, lib.ocm_op_weight_norm(P, P, P, P, 0, 8, None), "rows")
    _refused(lib, lib.ocm_op_weight_norm(P, P, P, P, 4, -3, None), "dim")
    _refused(lib, lib.ocm_op_weight_norm_backward(None, P, P, P, P, P, 4, 8, None), "null")
    _refused(lib, lib.ocm_op_weight_norm_backward(P, P, P, P, None, None, 4, 8, None), "both outputs")
    _refused(lib, lib.ocm_op_weight_norm_backward(P, P, P, P, P, None, 4, 0, None), "dim")
    _refused(lib, lib.ocm_op_weight_norm_backward(P, P, P, P, None, P + 2, 4, 8, None), "aligned")


def test_loss_and_center_refusals(lib):
    ws = lib.ocm_dino_loss_workspace_bytes
    assert ws(2, 10, 65536) == 2 * 16 * 2 * 10 * 8 and ws(1, 2, 1) == 32 and ws(3, 4, 4097) == 3 * 2 * 2 * 4 * 8
    assert ws(0, 2, 8) == 0 and ws(1, 1, 8) == 0 and ws(1, 2, 0) == 0
    big = 1 << 30

    def loss(s=P, t=P, c=P, ts=0.1, tt=0.04, B=2, V=3, K=40, out=P, stats=P, wsp=P, nbytes=big):
        return lib.ocm_op_dino_loss(s, t, c, ts, tt, B, V, K, out, stats, wsp, nbytes, None)

    for name in ("s", "t", "c", "out", "stats"):
        _refused(lib, loss(**{name: None}), "null")
    _refused(lib, loss(B=0), "B = 0")
    _refused(lib, loss(V=1), "V = 1")
    _refused(lib, loss(K=0), "K = 0")
    for bad in (dict(ts=0.0), dict(tt=-1.0), dict(ts=float("nan")), dict(tt=float("inf"))):
        _refused(lib, loss(**bad), "temp")
    _refused(lib, loss(s=P + 2), "aligned")
    _refused(lib, loss(stats=P + 4), "aligned")
    _refused(lib, loss(wsp=None), "workspace")
    _refused(lib, loss(nbytes=2 * 1 * 2 * 3 * 8 - 1), "workspace")
    _refused(lib, loss(wsp=P + 4), "workspace")

    def bwd(g=P, s=P, t=P, c=P, ts=0.1, tt=0.04, B=2, V=3, K=40, stats=P, ds=P):
        return lib.ocm_op_dino_loss_backward(g, s, t, c, ts, tt, B, V, K, stats, ds, None)

    for name in ("g", "s", "t", "c", "stats", "ds"):
        _refused(lib, bwd(**{name: None}), "null")
    _refused(lib, bwd(V=0), "V = 0")
    _refused(lib, bwd(ts=0.0), "temp")
    _refused(lib, bwd(ds=P + 1), "aligned")

    SUM, UPD = _lib.OCM_DINO_CENTER_SUM, _lib.OCM_DINO_CENTER_UPDATE
    _refused(lib, lib.ocm_op_dino_center(2, P, 4, 8, P, P, 4.0, 0.9, None), "mode")
    _refused(lib, lib.ocm_op_dino_center(SUM, P, 4, 0, P, None, 0.0, 0.0, None), "K = 0")
    _refused(lib, lib.ocm_op_dino_center(SUM, None, 4, 8, P, None, 0.0, 0.0, None), "teacher")
    _refused(lib, lib.ocm_op_dino_center(SUM, P, 0, 8, P, None, 0.0, 0.0, None), "rows")
    _refused(lib, lib.ocm_op_dino_center(SUM, P, 4, 8, None, None, 0.0, 0.0, None), "batch_sum")
    _refused(lib, lib.ocm_op_dino_center(UPD, None, 0, 8, P, None, 4.0, 0.9, None), "center")
    _refused(lib, lib.ocm_op_dino_center(UPD, None, 0, 8, P, P, 0.0, 0.9, None), "count")
    _refused(lib, lib.ocm_op_dino_center(UPD, None, 0, 8, P, P, 4.0, float("nan"), None), "momentum")


def test_ema_refusals(lib):
    def table(rows):
        return np.ascontiguousarray(np.array(rows, dtype=np.int64))

    good = table([[P, P, 0, 0, 16]])
    _refused(lib, lib.ocm_op_ema_update(None, 1, 0.9, None), "null")
    _refused(lib, lib.ocm_op_ema_update(good.ctypes.data, -1, 0.9, None), "-1 tensors")
    _refused(lib, lib.ocm_op_ema_update(good.ctypes.data, 1, float("inf"), None), "momentum")
    _refused(lib, lib.ocm_op_ema_update(table([[0, P, 0, 0, 4]]).ctypes.data, 1, 0.9, None), "null param")
    _refused(lib, lib.ocm_op_ema_update(table([[P, 0, 0, 0, 4]]).ctypes.data, 1, 0.9, None), "null grad")
    _refused(lib, lib.ocm_op_ema_update(table([[P, P + 2, 0, 0, 4]]).ctypes.data, 1, 0.9, None), "aligned")
    _refused(lib, lib.ocm_op_ema_update(table([[P, P, 0, 0, -1]]).ctypes.data, 1, 0.9, None), "count")
    assert lib.ocm_op_ema_update(table([[0, 0, 0, 0, 0]]).ctypes.data, 1, 0.9, None) == _lib.OCM_OK  # nothing to launch
