"""The reference's optimizer.py on the HIP path: the parameter groups of its training scripts and AdamW / Adam / SGD whose step()
is one multi-tensor launch of kernels_optim.hip per (param group, step count) instead of torch.optim's pass per tensor.

  check_keywords_in_name, get_pretrain_param_groups, get_params_groups, build_pretrain_optimizer
                      reference optimizer.py:6-78 (mim.py's SimMIM groups, DINO's groups, the optimizer TRAIN.OPTIMIZER names)
  AdamW, Adam, SGD    torch.optim's classes of the same names (their constructors, defaults, param_groups and state: `step` a CPU
                      float32 scalar, `exp_avg`, `exp_avg_sq`, `momentum_buffer`, so a state_dict() moves between the two in both
                      directions), with step() on the device: torch's single-tensor rules, the scalar factors formed in Python
                      floats as torch forms them. fp32 parameters on one HIP device only; there is no CPU or eager fall-back.

step() launches on the current stream of the parameters' device, allocates nothing after the first step, never reads the device
back, and afterwards raises every stepped parameter's version counter: the operand caches and engines of this package (engine.SourceCache)
compare (data_ptr, _version), and a raw kernel write is invisible to autograd's own counting. The `step` entries of the state are 0-dim
views of CPU tensors shared by many parameters (read and raised in one operation each); a loaded state's own `step` tensors are
replaced by such views of the same value at the first step() after load_state_dict().
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import _stream

__all__ = ["AdamW", "Adam", "SGD", "check_keywords_in_name", "get_pretrain_param_groups", "get_params_groups",
           "build_pretrain_optimizer", "optim_limits"]


def optim_limits():
    """(T, C): the tensors one launch takes and the elements one workgroup takes (ocm_optim_limits)."""
    t, c = C.c_int32(0), C.c_int32(0)
    _lib.load().ocm_optim_limits(C.byref(t), C.byref(c))
    return t.value, c.value


def _check_tensor(t, what, device):
    """The refusals shared by step() and the gradient norm; returns the one device every tensor of a call lives on."""
    if t.is_sparse:
        raise TypeError(f"{what} is sparse: the HIP optimizer path takes dense gradients only")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} is {t.dtype}: the HIP optimizer path takes float32 only")
    if not t.is_cuda:
        raise TypeError(f"{what} lives on {t.device}: the HIP optimizer path runs on a HIP device only (no CPU fall-back)")
    if device is not None and t.device != device:
        raise TypeError(f"{what} lives on {t.device}, others on {device}: one device per call")
    return t.device


def _table(columns):
    """The OcmOptimTensor array of a call, (N, 5) int64 rows of (param, grad, m, v, count), from per-column lists."""
    return np.ascontiguousarray(np.array(columns, dtype=np.int64).T)


STEP_BLOCK = 256  # step counts per shared CPU tensor


class _Entry:
    """What step() knows about one parameter between calls: its state dict and state tensors (held, so their addresses stay
    valid), their addresses, and for the Adam rules the slot of its `step` count."""
    __slots__ = ("p", "state", "m", "v", "m_ptr", "v_ptr", "numel", "device", "step_t", "block", "slot", "first")


class _StepCache:
    """Per optimizer, dropped whenever `optimizer.state` is replaced (load_state_dict does that)."""

    def __init__(self, state):
        self.state = state
        self.entries = {}  # id(p) -> _Entry
        self.tables = {}   # (group, bucket ordinal) -> (key, (N, 5) int64 array): rebuilt only when an address or a count changed
        # The `step` entries of the state are 0-dim views of shared CPU float32 tensors, STEP_BLOCK counts each: one tolist()
        # reads every count of a step() and one add_ raises them, instead of an .item() and an add per parameter. Each view is a
        # CPU float32 scalar tensor as torch's own `step` is, and torch's optimizers step it as they step their own.
        self.blocks, self.used, self.hits, self.values = [], 0, [], []

    def table(self, slot, columns):
        key = tuple(map(tuple, columns))
        hit = self.tables.get(slot)
        if hit is None or hit[0] != key:
            hit = self.tables[slot] = (key, _table(columns))
        return hit[1]

    def new_step(self, value):
        """A 0-dim view holding `value` -> (view, block index, slot)."""
        if not self.blocks or self.used == STEP_BLOCK:
            self.blocks.append(torch.zeros(STEP_BLOCK, dtype=torch.float32))
            self.values.append([0.0] * STEP_BLOCK)
            self.hits.append(None)
            self.used = 0
        bi, slot = len(self.blocks) - 1, self.used
        self.used += 1
        self.blocks[bi][slot] = value
        self.values[bi][slot] = value
        return self.blocks[bi][slot], bi, slot


_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


def _refuse_unsupported(name, lr, flags):
    for flag, value in flags.items():
        if value:
            raise NotImplementedError(f"{name}({flag}=True) is not implemented on the HIP path")
    if isinstance(lr, torch.Tensor):
        raise NotImplementedError(f"{name}: a tensor lr is not implemented on the HIP path (pass a float)")


def _check_state_tensor(t, what, p):
    _check_tensor(t, what, p.device)
    if t.shape != p.shape or not t.is_contiguous():
        raise ValueError(f"{what} {tuple(t.shape)} of a parameter {tuple(p.shape)} must be contiguous and of its shape")


class _HipStep:
    """step() shared by the three classes: gather (param, grad, state) per bucket, one ocm_op_optim_step per bucket. A bucket
    is the parameters of one group that share the values of a step (the step count; for SGD whether the momentum buffer exists).
    The host side costs about as much as the kernels for a model of 200 tensors, so what does not change between calls is kept
    per parameter (_Entry) and only what can change is looked at again: the gradient, the parameter's address, the identity of
    the state tensors."""

    def _new_entry(self, cache, group, p, ent):  # fills ent.m / ent.v (and the step slot) from self.state[p], creating the state
        raise NotImplementedError

    def _entry_valid(self, group, ent):  # the state still holds the tensors the entry knows
        raise NotImplementedError

    def _key(self, cache, ent):  # the bucket of this step
        raise NotImplementedError

    def _hyper(self, group, key):  # -> the OcmOptimHyper of a bucket
        raise NotImplementedError

    def _after_launch(self, cache, entries):
        pass

    def _entry(self, cache, group, p, device):
        _check_tensor(p, "a parameter", device)
        if not p.is_contiguous():
            raise ValueError(f"a parameter of shape {tuple(p.shape)} is not contiguous")
        ent = _Entry()
        ent.p, ent.numel, ent.device, ent.first = p, p.numel(), p.device, False
        ent.m = ent.v = ent.step_t = None
        self._new_entry(cache, group, p, ent)
        ent.state = self.state[p] if (ent.m is not None or ent.step_t is not None) else None
        ent.m_ptr = ent.m.data_ptr() if ent.m is not None else 0
        ent.v_ptr = ent.v.data_ptr() if ent.v is not None else 0
        cache.entries[id(p)] = ent
        return ent

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        cache = self.__dict__.get("_hip_cache")
        if cache is None or cache.state is not self.state:
            cache = self.__dict__["_hip_cache"] = _StepCache(self.state)
        cache.values = [b.tolist() for b in cache.blocks]
        entries, f32, state = cache.entries, torch.float32, self.state
        device, stepped, done, keep, calls = None, [], [], [], []
        for gi, group in enumerate(self.param_groups):
            for flag in _UNSUPPORTED:
                if group.get(flag):
                    raise NotImplementedError(f"{type(self).__name__}: {flag}=True is not implemented on the HIP path")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError(f"{type(self).__name__}: a tensor lr is not implemented on the HIP path")
            buckets = {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                ent = entries.get(id(p))
                # (an entry with state must still be looking at the dict optimizer.state holds for p: `opt.state[p] = {}` and
                # `del opt.state[p]` leave the old dict, and the tensors in it, alive in the entry)
                if (ent is None or ent.p is not p or (ent.state is not None and state.get(p) is not ent.state)
                        or not self._entry_valid(group, ent)):
                    ent = self._entry(cache, group, p, device)
                if device is None:
                    device = ent.device
                # torch lets a gradient differ from its parameter in layout and strides only
                if g.is_sparse or g.dtype is not f32 or not g.is_cuda or ent.device != device:
                    _check_tensor(g, "a gradient", device)
                    _check_tensor(p, "a parameter", device)
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                key = self._key(cache, ent)
                cols = buckets.get(key)
                if cols is None:
                    cols = buckets[key] = ([], [], [], [], [])
                cols[0].append(p.data_ptr())
                cols[1].append(g.data_ptr())
                cols[2].append(ent.m_ptr)
                cols[3].append(ent.v_ptr)
                cols[4].append(ent.numel)
                stepped.append(p)
                done.append(ent)
            for j, (key, cols) in enumerate(buckets.items()):
                calls.append((cache.table((gi, j), cols), self._hyper(group, key)))
        if calls:
            with torch.cuda.device(device):
                stream = _stream()
                for table, hyper in calls:
                    _lib.check(lib.ocm_op_optim_step(table.ctypes.data, table.shape[0], C.byref(hyper), stream))
            self._after_launch(cache, done)
            torch.autograd.graph.increment_version(stepped)
        return loss


class _HipAdamStep(_HipStep):
    def _new_entry(self, cache, group, p, ent):
        state = self.state[p]
        if len(state) == 0:  # torch's Adam._init_group
            state["step"] = torch.tensor(0.0, dtype=torch.float32)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        ent.m, ent.v = state["exp_avg"], state["exp_avg_sq"]
        _check_state_tensor(ent.m, "exp_avg", p)
        _check_state_tensor(ent.v, "exp_avg_sq", p)
        state["step"], ent.block, ent.slot = cache.new_step(float(state["step"]))  # the same value, now a view of a shared block
        ent.step_t = state["step"]

    def _entry_valid(self, group, ent):
        st = ent.state
        return st.get("step") is ent.step_t and st.get("exp_avg") is ent.m and st.get("exp_avg_sq") is ent.v

    def _key(self, cache, ent):
        return cache.values[ent.block][ent.slot] + 1.0

    def _hyper(self, group, step):
        beta1, beta2 = group["betas"]
        lr = float(group["lr"])
        bias_correction1 = 1 - beta1 ** step
        bias_correction2 = 1 - beta2 ** step
        decoupled = bool(group.get("decoupled_weight_decay", False))
        return _lib.OcmOptimHyper(rule=_lib.OCM_OPTIM_ADAMW if decoupled else _lib.OCM_OPTIM_ADAM, lr=lr, beta1=beta1, beta2=beta2,
                                  eps=group["eps"], weight_decay=group["weight_decay"], step_size=lr / bias_correction1,
                                  bias_correction2_sqrt=bias_correction2 ** 0.5)

    def _after_launch(self, cache, entries):
        hits = cache.hits
        for ent in entries:
            h = hits[ent.block]
            if h is None:
                h = hits[ent.block] = [0.0] * STEP_BLOCK
            h[ent.slot] = 1.0
        for bi, h in enumerate(hits):
            if h is not None:
                cache.blocks[bi].add_(torch.tensor(h, dtype=torch.float32))
                hits[bi] = None


class AdamW(_HipAdamStep, torch.optim.AdamW):
    """torch.optim.AdamW (decoupled weight decay) stepped by kernels_optim.hip. `foreach` and `fused` are accepted and ignored."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        _refuse_unsupported("AdamW", lr, dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable,
                                              differentiable=differentiable))
        super().__init__(params, lr, betas, eps, weight_decay, False)


class Adam(_HipAdamStep, torch.optim.Adam):
    """torch.optim.Adam (L2 decay formed in registers: p.grad is never written) stepped by kernels_optim.hip."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        _refuse_unsupported("Adam", lr, dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable,
                                             differentiable=differentiable))
        super().__init__(params, lr, betas, eps, weight_decay, False, decoupled_weight_decay=decoupled_weight_decay)


class SGD(_HipStep, torch.optim.SGD):
    """torch.optim.SGD (L2 decay, momentum, dampening, Nesterov) stepped by kernels_optim.hip."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None):
        _refuse_unsupported("SGD", lr, dict(maximize=maximize, differentiable=differentiable))
        if isinstance(weight_decay, torch.Tensor):
            raise NotImplementedError("SGD: a tensor weight_decay is not implemented on the HIP path (pass a float)")
        super().__init__(params, lr, momentum, dampening, weight_decay, nesterov)

    def _new_entry(self, cache, group, p, ent):
        if group["momentum"] == 0:
            return
        state = self.state[p]
        buf = state.get("momentum_buffer")
        if buf is None:  # written, not read, by the coming step: buf = g + wd p
            buf = state["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
            ent.first = True
        _check_state_tensor(buf, "momentum_buffer", p)
        ent.m = buf

    def _entry_valid(self, group, ent):
        if group["momentum"] == 0:
            return ent.m is None
        return ent.m is not None and ent.state.get("momentum_buffer") is ent.m

    def _key(self, cache, ent):
        return ent.first

    def _after_launch(self, cache, entries):
        for ent in entries:
            ent.first = False

    def _hyper(self, group, first):
        return _lib.OcmOptimHyper(rule=_lib.OCM_OPTIM_SGD, nesterov=int(bool(group["nesterov"])), first_step=int(first),
                                  lr=float(group["lr"]), weight_decay=float(group["weight_decay"]), momentum=group["momentum"],
                                  dampening=group["dampening"], bias_correction2_sqrt=1.0)


# ---- the parameter groups of the training scripts (reference optimizer.py) ------------------------------------------------------
def check_keywords_in_name(name, keywords=()):
    """True when any of `keywords` occurs in `name`."""
    return any(keyword in name for keyword in keywords)


def get_pretrain_param_groups(model, logger, skip_list=(), skip_keywords=()):
    """mim.py's two groups over the trainable parameters: [decayed, {not decayed, weight_decay 0}]. Not decayed: 1-D parameters,
    names ending in ".bias", names in `skip_list` (the model's no_weight_decay()) and names holding one of `skip_keywords`."""
    decayed, plain = [], []
    for name, param in model.named_parameters():
        if param.requires_grad:
            exempt = param.dim() == 1 or name.endswith(".bias") or name in skip_list or check_keywords_in_name(name, skip_keywords)
            (plain if exempt else decayed).append((name, param))
    logger.info(f"No decay params: {[n for n, _ in plain]}")
    logger.info(f"Has decay params: {[n for n, _ in decayed]}")
    return [{"params": [p for _, p in decayed]}, {"params": [p for _, p in plain], "weight_decay": 0.}]


def get_params_groups(model):
    """DINO's two groups: biases and 1-D (norm) parameters are not regularised."""
    groups = ([], [])
    for name, param in model.named_parameters():
        if param.requires_grad:
            groups[name.endswith(".bias") or param.dim() == 1].append(param)
    return [{"params": groups[0]}, {"params": groups[1], "weight_decay": 0.}]


def build_pretrain_optimizer(args, model, logger):
    """The optimizer mim.py trains with: TRAIN.OPTIMIZER.NAME "adamw" -> AdamW(eps, betas), "sgd" -> Nesterov SGD(momentum), both
    with TRAIN.BASE_LR and TRAIN.WEIGHT_DECAY over get_pretrain_param_groups; any other name gives None, as in the reference."""
    logger.info(">>>>>>>>>> Build Optimizer for Pre-training Stage")
    skip = model.no_weight_decay() if hasattr(model, "no_weight_decay") else {}
    skip_keywords = model.no_weight_decay_keywords() if hasattr(model, "no_weight_decay_keywords") else {}
    logger.info(f"No weight decay: {skip}; keywords: {skip_keywords}")
    groups = get_pretrain_param_groups(model, logger, skip, skip_keywords)
    train = args.TRAIN
    name = train.OPTIMIZER.NAME.lower()
    optimizer = None
    if name == "sgd":
        optimizer = SGD(groups, momentum=train.OPTIMIZER.MOMENTUM, nesterov=True, lr=train.BASE_LR, weight_decay=train.WEIGHT_DECAY)
    elif name == "adamw":
        optimizer = AdamW(groups, eps=train.OPTIMIZER.EPS, betas=train.OPTIMIZER.BETAS, lr=train.BASE_LR,
                          weight_decay=train.WEIGHT_DECAY)
    logger.info(optimizer)
    return optimizer
