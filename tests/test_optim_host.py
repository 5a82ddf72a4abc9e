"""Host side of the optimizer path (kernels_optim.hip, optimizer.py, utils.clip_grad_norm_ / grad_norm / get_grad_norm): the C
ABI's declarations, limits and argument refusals (decided before any device call), the constructors' and step()'s refusals, the
state-dict exchange with torch.optim on CPU parameters and the parameter groups of the training scripts. No GPU needed."""
import ctypes as C
import logging
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from vit_ocm_wmsegmentation_amd import _lib
from vit_ocm_wmsegmentation_amd import optimizer as OPT
from vit_ocm_wmsegmentation_amd import utils as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ocm_optim_limits", "ocm_op_optim_step", "ocm_grad_norm_workspace_bytes", "ocm_op_grad_norm", "ocm_op_grad_scale"]
P = 4096  # a non-null address that is never touched


def _table(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.int64))


def _hyper(**kw):
    base = dict(rule=_lib.OCM_OPTIM_ADAMW, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step_size=1e-2,
                bias_correction2_sqrt=0.03, momentum=0.9, dampening=0.0)
    base.update(kw)
    return _lib.OcmOptimHyper(**base)


def _refused(lib, rc, word):
    assert rc == _lib.OCM_EINVAL, rc
    assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()


def test_entry_points_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "ocm_vit.h")).read()
    assert re.search(r"#define OCM_ABI_VERSION 20\b", text)  # the additions are additive
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert "kernels_optim.hip" in open(os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc", "Makefile")).read()
    assert C.sizeof(_lib.OcmOptimTensor) == 40 and C.sizeof(_lib.OcmOptimHyper) == 16 + 9 * 8


def test_limits(lib):
    T, chunk = OPT.optim_limits()
    assert T >= 1 and chunk >= 4 and chunk % 4 == 0
    lib.ocm_optim_limits(None, None)  # either pointer may be null


def test_step_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    good = _table([[P, P, P, P, 16]])
    h = _hyper()
    _refused(lib, lib.ocm_op_optim_step(None, 1, C.byref(h), None), "null")
    _refused(lib, lib.ocm_op_optim_step(good.ctypes.data, 1, None, None), "null")
    _refused(lib, lib.ocm_op_optim_step(good.ctypes.data, -1, C.byref(h), None), "-1 tensors")
    for rule in (-1, 3, 7):
        _refused(lib, lib.ocm_op_optim_step(good.ctypes.data, 1, C.byref(_hyper(rule=rule)), None), "rule")
    for col, word in ((0, "null param"), (1, "null grad"), (2, "null m"), (3, "null v")):
        row = [P, P, P, P, 16]
        row[col] = 0
        t = _table([[P, P, P, P, 4], row])
        _refused(lib, lib.ocm_op_optim_step(t.ctypes.data, 2, C.byref(h), None), "tensor 1: " + word)
    sgd = _hyper(rule=_lib.OCM_OPTIM_SGD)
    _refused(lib, lib.ocm_op_optim_step(_table([[0, P, P, 0, 8]]).ctypes.data, 1, C.byref(sgd), None), "null param")
    _refused(lib, lib.ocm_op_optim_step(_table([[P, P, 0, 0, 8]]).ctypes.data, 1, C.byref(sgd), None), "null m")
    for count in (-1, (1 << 36) + 1):
        _refused(lib, lib.ocm_op_optim_step(_table([[P, P, P, P, count]]).ctypes.data, 1, C.byref(h), None), "count")
    _refused(lib, lib.ocm_op_optim_step(_table([[P + 2, P, P, P, 8]]).ctypes.data, 1, C.byref(h), None), "aligned")
    for bad in (dict(lr=float("nan")), dict(step_size=float("inf")), dict(bias_correction2_sqrt=0.0)):
        assert lib.ocm_op_optim_step(good.ctypes.data, 1, C.byref(_hyper(**bad)), None) == _lib.OCM_EINVAL, bad
    with pytest.raises(ValueError):
        _lib.check(lib.ocm_op_optim_step(good.ctypes.data, 1, C.byref(_hyper(rule=9)), None))


def test_norm_and_scale_refusals(lib):
    T, chunk = OPT.optim_limits()
    good = _table([[0, P, 0, 0, chunk + 1], [0, 0, 0, 0, 0], [0, P, 0, 0, 3]])
    ws = lib.ocm_grad_norm_workspace_bytes
    assert ws(good.ctypes.data, 3) == 8 * 3 and ws(good.ctypes.data, 0) == 8
    assert ws(None, 1) == 0 and ws(good.ctypes.data, -1) == 0 and ws(_table([[0, P, 0, 0, -1]]).ctypes.data, 1) == 0
    big = 1 << 30

    def norm(tab=good, n=3, sumsq=P, out=P, coef=P, wsp=P, nbytes=big):
        return lib.ocm_op_grad_norm(tab.ctypes.data if tab is not None else None, n, 1.0, sumsq, out, coef, wsp, nbytes, None)

    _refused(lib, norm(tab=None), "null")
    _refused(lib, norm(n=-1), "-1 tensors")
    _refused(lib, norm(tab=_table([[0, 0, 0, 0, 5]]), n=1), "null grad")
    for name in ("sumsq", "out", "coef"):
        _refused(lib, norm(**{name: None}), "null output")
    _refused(lib, norm(nbytes=8 * 3 - 1), "workspace")
    _refused(lib, norm(wsp=None), "workspace")
    _refused(lib, norm(wsp=P + 4), "workspace")
    _refused(lib, lib.ocm_op_grad_scale(None, 1, P, None), "null")
    _refused(lib, lib.ocm_op_grad_scale(good.ctypes.data, -1, P, None), "-1 tensors")
    _refused(lib, lib.ocm_op_grad_scale(good.ctypes.data, 3, None, None), "null coefficient")
    _refused(lib, lib.ocm_op_grad_scale(_table([[P, 0, P, P, 5]]).ctypes.data, 1, P, None), "null grad")


def test_constructor_and_step_refusals():
    ps = [nn.Parameter(torch.randn(3, 4))]
    for cls in (OPT.AdamW, OPT.Adam):
        for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
            with pytest.raises(NotImplementedError):
                cls(ps, **{flag: True})
        with pytest.raises(NotImplementedError):
            cls(ps, lr=torch.tensor(1e-3))
        cls(ps, foreach=True), cls(ps, fused=True), cls(ps, foreach=False, fused=False)  # accepted and ignored
    for flag in ("maximize", "differentiable"):
        with pytest.raises(NotImplementedError):
            OPT.SGD(ps, **{flag: True})
    with pytest.raises(NotImplementedError):
        OPT.SGD(ps, lr=torch.tensor(1e-3))
    OPT.SGD(ps, foreach=True), OPT.SGD(ps, fused=True)
    for cls, tcls in ((OPT.AdamW, torch.optim.AdamW), (OPT.Adam, torch.optim.Adam), (OPT.SGD, torch.optim.SGD)):
        assert issubclass(cls, torch.optim.Optimizer) and cls(ps).defaults == tcls(ps).defaults
        ps[0].grad = torch.randn(3, 4)
        opt = cls(ps)
        with pytest.raises(TypeError):  # CPU parameters: there is no host fall-back
            opt.step()
        assert len(opt.state) == 0
    ps[0].grad = None
    OPT.AdamW(ps).step()  # nothing to step: no device is needed
    with pytest.raises(ValueError):
        OPT.AdamW(ps, lr=-1.0)  # torch's own argument checks still apply
    for fn in (lambda: U.clip_grad_norm_(ps, 1.0, norm_type=1), lambda: U.grad_norm(ps, norm_type=3),
               lambda: U.get_grad_norm(ps, norm_type=1)):
        with pytest.raises(ValueError):
            fn()
    assert float(U.clip_grad_norm_(ps, 1.0)) == 0.0 and U.get_grad_norm(ps) == 0.0  # no gradients
    ps[0].grad = torch.randn(3, 4)
    with pytest.raises(TypeError):
        U.clip_grad_norm_(ps, 1.0)
    with pytest.raises(TypeError):
        U.get_grad_norm(ps)


def _assert_same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys()
        for name, v in a["state"][k].items():
            w = b["state"][k][name]
            assert v.dtype == w.dtype and v.device == w.device and torch.equal(v, w), (k, name)


@pytest.mark.parametrize("name", ["AdamW", "Adam", "SGD"])
def test_state_dict_exchange_on_cpu(name):
    """A torch.optim state dict loads into ours and back, on CPU parameters, with equal keys and values."""
    tcls, ours = getattr(torch.optim, name), getattr(OPT, name)
    kwargs = dict(lr=1e-2, momentum=0.9) if name == "SGD" else dict(lr=1e-2, weight_decay=0.03)
    torch.manual_seed(0)
    ps = [nn.Parameter(torch.randn(3, 4)), nn.Parameter(torch.randn(5))]
    t = tcls(ps, **kwargs)
    for _ in range(2):
        for p in ps:
            p.grad = torch.randn_like(p)
        t.step()
    sd = t.state_dict()
    o = ours([nn.Parameter(p.detach().clone()) for p in ps], **kwargs)
    _assert_same_state_dict(ours(ps, **kwargs).state_dict(), tcls(ps, **kwargs).state_dict())  # fresh: the same groups
    o.load_state_dict(sd)
    _assert_same_state_dict(o.state_dict(), sd)
    if name != "SGD":
        st = o.state_dict()["state"][0]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 2.0
    back = tcls([nn.Parameter(p.detach().clone()) for p in ps], **kwargs)
    back.load_state_dict(o.state_dict())
    _assert_same_state_dict(back.state_dict(), sd)


class _Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.pos_embed = nn.Parameter(torch.zeros(1, 5, 8))
        self.cls_token = nn.Parameter(torch.zeros(1, 1, 8))
        self.fc = nn.Linear(8, 8)
        self.norm = nn.LayerNorm(8)
        self.rel = nn.ModuleDict({"relative_position_bias_table": nn.Linear(8, 2, bias=False)})
        self.frozen = nn.Linear(8, 8)
        self.frozen.requires_grad_(False)

    def no_weight_decay(self):
        return {"pos_embed"}

    def no_weight_decay_keywords(self):
        return {"relative_position_bias_table"}


def _names(model, group):
    by_id = {id(p): n for n, p in model.named_parameters()}
    return sorted(by_id[id(p)] for p in group["params"])


def test_param_groups():
    m, logger = _Toy(), logging.getLogger("test_optim_host")
    assert OPT.check_keywords_in_name("a.bias_table.b", ("x", "bias_table")) and not OPT.check_keywords_in_name("a", ("b",))
    assert not OPT.check_keywords_in_name("a", ())
    decay, plain = OPT.get_pretrain_param_groups(m, logger, m.no_weight_decay(), m.no_weight_decay_keywords())
    assert "weight_decay" not in decay and plain["weight_decay"] == 0.0
    assert _names(m, decay) == ["cls_token", "fc.weight"]
    assert _names(m, plain) == ["fc.bias", "norm.bias", "norm.weight", "pos_embed", "rel.relative_position_bias_table.weight"]
    decay, plain = OPT.get_pretrain_param_groups(m, logger)
    assert _names(m, decay) == ["cls_token", "fc.weight", "pos_embed", "rel.relative_position_bias_table.weight"]
    reg, not_reg = OPT.get_params_groups(m)
    assert _names(m, reg) == ["cls_token", "fc.weight", "pos_embed", "rel.relative_position_bias_table.weight"]
    assert _names(m, not_reg) == ["fc.bias", "norm.bias", "norm.weight"] and not_reg["weight_decay"] == 0.0


@pytest.mark.parametrize("name", ["adamw", "AdamW", "sgd", "lamb"])
def test_build_pretrain_optimizer(name):
    cfg = types.SimpleNamespace(TRAIN=types.SimpleNamespace(
        BASE_LR=3e-4, WEIGHT_DECAY=0.04, OPTIMIZER=types.SimpleNamespace(NAME=name, EPS=1e-7, BETAS=(0.85, 0.98), MOMENTUM=0.8)))
    m = _Toy()
    opt = OPT.build_pretrain_optimizer(cfg, m, logging.getLogger("test_optim_host"))
    if name == "lamb":
        assert opt is None  # as the reference: an unknown name builds nothing
        return
    decay, plain = opt.param_groups
    assert _names(m, decay) == ["cls_token", "fc.weight"] and len(plain["params"]) == 5
    assert decay["lr"] == plain["lr"] == 3e-4 and decay["weight_decay"] == 0.04 and plain["weight_decay"] == 0.0
    if name == "sgd":
        assert type(opt) is OPT.SGD and decay["nesterov"] is True and decay["momentum"] == 0.8 and decay["dampening"] == 0
    else:
        assert type(opt) is OPT.AdamW and decay["eps"] == 1e-7 and decay["betas"] == (0.85, 0.98)
