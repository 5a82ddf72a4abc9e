"""Swin-T behind the module surface the reference's Allen_data_Backbone/train.py:70-85 uses (transformers' `SwinConfig` /
`SwinForImageClassification`): same constructor fields, same state_dict keys (a transformers checkpoint loads with
`load_state_dict`), `model(pixel_values=..., labels=...)` -> object with `.loss`, `.logits` (and `.pooler_output`, optionally
`.last_hidden_state`). The arithmetic runs in libocm_vit.so (include/ocm_swin.h); there is no CPU fallback.

As a backbone: `output_hidden_states=True` adds transformers' `hidden_states` / `reshaped_hidden_states` (the per-stage
feature maps), `output_attentions=True` the window-softmax of every layer (`attentions`, one entry per LAYER: transformers
5.x returns the last block of each stage only, and only with attn_implementation="eager" — take
`attentions[cumsum(depths) - 1]` for those). `SwinModel` is the model without the classifier, and
`SwinForImageClassification.swin` the same view over a (fine-tuned) classifier's own parameters and engine.

Inference runs the engine (ocm_swin_forward) with windows of 2 to 12 — 12 is the geometry of the window12-384 checkpoints
(`SwinConfig(image_size=384, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)`), whose windows
tile a 384^2 tile's grids without padding; training takes windows of 2 to 7, and 8 to 12 after
enable_wide_window_training(). Training — train.py's Trainer loop — runs when the module is in training mode,
grad mode is on and a parameter requires grad (the parameters are created with requires_grad=False: opt in with
`model.requires_grad_(True)`): the stand-alone operators under one autograd Function (_SwinTrain) whose backward is HIP
(kernels_swin_train.hip plus the ViT training operators).
"""
import ctypes as C
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .dino.utils import trunc_normal_
from .engine import OPERAND_DTYPE, SourceCache, _p, _require_hip, _stream, _ws, from_split, signature, to_operand
from .model import _differentiable, _linear, _ln, _ln_backward, _weight_grad


class SwinConfig:
    """The fields of transformers.SwinConfig this path reads (defaults = swin-tiny-patch4-window7-224). drop_path_rate and
    the dropout probabilities act in training only, as in transformers."""

    def __init__(self, image_size=224, patch_size=4, num_channels=3, embed_dim=96, depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4.0, qkv_bias=True, hidden_act="gelu",
                 layer_norm_eps=1e-5, num_labels=2, label2id=None, id2label=None, drop_path_rate=0.1,
                 hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, encoder_stride=32, **unused):
        if hidden_act != "gelu" or not qkv_bias:
            raise ValueError("only hidden_act='gelu' with qkv_bias=True (the Swin-T defaults) is built")
        self.image_size, self.patch_size, self.num_channels, self.embed_dim = image_size, patch_size, num_channels, embed_dim
        self.depths, self.num_heads = tuple(depths), tuple(num_heads)
        self.window_size, self.mlp_ratio, self.layer_norm_eps = window_size, mlp_ratio, layer_norm_eps
        self.qkv_bias, self.hidden_act = qkv_bias, hidden_act
        self.label2id, self.id2label = label2id, id2label
        self.num_labels = len(id2label) if id2label else num_labels
        self.num_layers = len(self.depths)
        self.hidden_size = int(embed_dim * 2 ** (self.num_layers - 1))
        self.drop_path_rate = drop_path_rate
        self.hidden_dropout_prob, self.attention_probs_dropout_prob = hidden_dropout_prob, attention_probs_dropout_prob
        self.encoder_stride = encoder_stride  # SwinForMaskedImageModeling's decoder: Conv2d + PixelShuffle(encoder_stride)


class SwinOutput(types.SimpleNamespace):
    """What `forward` returns: the attributes loss, logits, pooler_output, last_hidden_state, hidden_states,
    reshaped_hidden_states, attentions (tuples, or None when not asked for), and, as transformers' ModelOutput does for a
    Trainer's compute_loss, out["loss"] and out[0] (the non-None of loss, logits, in that order)."""

    def to_tuple(self):
        return tuple(v for v in (self.loss, self.logits) if v is not None)

    def __getitem__(self, key):
        if isinstance(key, str):
            return getattr(self, key)
        return self.to_tuple()[key]


class SwinModelOutput(types.SimpleNamespace):
    """What SwinModel.forward returns: last_hidden_state, pooler_output (None without the pooling layer), hidden_states,
    reshaped_hidden_states, attentions; out["name"] and out[i] over the non-None of them in that order."""

    def to_tuple(self):
        return tuple(v for v in (self.last_hidden_state, self.pooler_output, self.hidden_states,
                                 self.reshaped_hidden_states, self.attentions) if v is not None)

    def __getitem__(self, key):
        if isinstance(key, str):
            return getattr(self, key)
        return self.to_tuple()[key]


class SwinMaskedImageModelingOutput(types.SimpleNamespace):
    """What SwinForMaskedImageModeling.forward returns: loss (None without a mask), reconstruction, hidden_states, attentions,
    reshaped_hidden_states; out["name"] and out[i] over the non-None of them in that order."""

    def to_tuple(self):
        return tuple(v for v in (self.loss, self.reconstruction, self.hidden_states, self.attentions,
                                 self.reshaped_hidden_states) if v is not None)

    def __getitem__(self, key):
        if isinstance(key, str):
            return getattr(self, key)
        return self.to_tuple()[key]


def drop_path_rates(config):
    """SwinEncoder's stochastic-depth rate of every layer in global order: drop_path_rate * i / max(sum(depths) - 1, 1)."""
    n = sum(config.depths)
    return [config.drop_path_rate * i / max(n - 1, 1) for i in range(n)]


def draw_drop_path_masks(config, batch, device):
    """The SwinDropPath draws of one training forward, in transformers' layer order: per layer None (rate 0: transformers
    builds an Identity and draws nothing) or (keep_prob, mask) with mask = floor(torch.rand((B, 1, 1)) + keep_prob) drawn
    exactly as SwinDropPath.forward draws it, so a seeded run draws the masks transformers would draw on that device."""
    out = []
    for rate in drop_path_rates(config):
        if rate == 0.0:
            out.append(None)
            continue
        keep = 1 - rate
        rnd = torch.rand((batch, 1, 1), dtype=torch.float32, device=device)
        out.append((keep, torch.floor(rnd + keep).reshape(batch)))
    return out


def _param_shapes(cfg):
    from .synth import swin_param_shapes
    return swin_param_shapes(dict(image_size=cfg.image_size, patch_size=cfg.patch_size, num_channels=cfg.num_channels,
                                  embed_dim=cfg.embed_dim, depths=cfg.depths, num_heads=cfg.num_heads,
                                  window_size=cfg.window_size, mlp_ratio=cfg.mlp_ratio, num_labels=cfg.num_labels))


def _layer_list(config, output_attentions):
    """The global layer indices whose attention map is wanted: False / None -> none, True -> every layer, or an iterable of
    layer indices (an extension: the layers after the last of them stay on their fused kernels; the other entries of
    `attentions` are None)."""
    n = sum(config.depths)
    if output_attentions is None or output_attentions is False:
        return []
    if output_attentions is True:
        return list(range(n))
    layers = sorted({int(i) for i in output_attentions})
    if layers and not 0 <= layers[0] <= layers[-1] < n:
        raise ValueError(f"output_attentions names layers {layers}; the model has layers 0 .. {n - 1}")
    return layers


class MaskTokenMissing(ValueError, NotImplementedError):
    """bool_masked_pos on a model that has no mask token. A ValueError, as the other mask refusals are, and still the
    NotImplementedError that SwinModel raised for any bool_masked_pos before the mask token was built."""


def _patch_mask(config, pixel_values, bool_masked_pos, has_token):
    """bool_masked_pos (B, L_0) torch.bool -> the uint8 bytes the kernels read, or None. transformers blends
    embeddings * (1 - w) + mask_token * w with w = the mask cast to the embeddings' dtype; this path selects rows, so anything
    but a 0 / 1 mask is refused."""
    if bool_masked_pos is None:
        return None
    if not has_token:
        raise MaskTokenMissing("bool_masked_pos needs the mask token, which this model does not have: it is built in "
                               "SwinForMaskedImageModeling and its `.swin` view")
    if not isinstance(bool_masked_pos, torch.Tensor) or bool_masked_pos.dtype != torch.bool:
        raise ValueError("bool_masked_pos must be a torch.bool tensor (this path selects rows; transformers would blend a "
                         f"fractional mask softly), got {getattr(bool_masked_pos, 'dtype', type(bool_masked_pos))}")
    L0 = (config.image_size // config.patch_size) ** 2
    if tuple(bool_masked_pos.shape) != (pixel_values.shape[0], L0):
        raise ValueError(f"expected a ({pixel_values.shape[0]}, {L0}) bool_masked_pos, got {tuple(bool_masked_pos.shape)}")
    return bool_masked_pos.to(pixel_values.device).to(torch.uint8).contiguous()


def _engine_run(eng, config, pixel_values, want_last, want_hidden, layers, patch_mask=None):
    """One inference forward through an engine entry (ocm_swin_forward_ex; ocm_swin_forward_masked with a patch mask, the
    uint8 bytes of _patch_mask) -> dict(logits, pooled, last_hidden, hidden_states, reshaped_hidden_states, attentions).
    Shapes come from ocm_swin_output_shape."""
    lib = _lib.load()
    x = pixel_values.detach().to(torch.float32).contiguous()
    dev, B = x.device, x.shape[0]
    f32 = dict(dtype=torch.float32, device=dev)
    n_hidden, n_layers = config.num_layers + 1, sum(config.depths)

    def shape(kind, index):
        dims = (C.c_int64 * 4)()
        _lib.check(lib.ocm_swin_output_shape(C.byref(eng["cfg"]), B, kind, index, dims))
        return tuple(dims)

    _, L, Cl, _ = shape(_lib.OCM_SWIN_OUT_HIDDEN, config.num_layers)
    logits = torch.empty((B, eng["labels"]), **f32) if eng["labels"] else None
    pooled = torch.empty((B, Cl), **f32)
    hidden = torch.empty((B, L, Cl), **f32) if want_last else None
    outs, hs, rs, at = None, None, None, None
    if want_hidden or layers:
        outs = _lib.OcmSwinOutputs()
        if want_hidden:
            hs = tuple(torch.empty(shape(_lib.OCM_SWIN_OUT_HIDDEN, i)[:3], **f32) for i in range(n_hidden))
            rs = tuple(torch.empty(shape(_lib.OCM_SWIN_OUT_RESHAPED, i), **f32) for i in range(n_hidden))
            for i in range(n_hidden):
                outs.hidden[i], outs.reshaped[i] = hs[i].data_ptr(), rs[i].data_ptr()
        if layers:
            ptrs = (C.c_void_p * n_layers)()
            at = [None] * n_layers
            for i in layers:
                at[i] = torch.empty(shape(_lib.OCM_SWIN_OUT_ATTENTION, i), **f32)
                ptrs[i] = at[i].data_ptr()
            outs.attentions = C.cast(ptrs, C.POINTER(C.c_void_p))
            at = tuple(at)
    ws = eng["ws"].get(B)
    if ws is None:
        nbytes = lib.ocm_swin_workspace_bytes(eng["h"], B)
        ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        eng["ws"] = {B: ws}
    off = (-ws.data_ptr()) % 256
    with torch.cuda.device(dev):
        if patch_mask is None:
            _lib.check(lib.ocm_swin_forward_ex(eng["h"], _p(x), B, _p(logits), _p(pooled), _p(hidden),
                                               C.byref(outs) if outs is not None else None,
                                               C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream()))
        else:
            _lib.check(lib.ocm_swin_forward_masked(eng["h"], _p(x), _p(patch_mask), B, _p(logits), _p(pooled), _p(hidden),
                                                   C.byref(outs) if outs is not None else None,
                                                   C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream()))
    return dict(logits=logits, pooled=pooled, last_hidden=hidden, hidden_states=hs, reshaped_hidden_states=rs, attentions=at)


class _SwinBase(nn.Module):
    """Parameters registered flat under their transformers state_dict keys (so `state_dict()` / `load_state_dict()`
    interoperate with transformers checkpoints key for key), the precision switch and the engine made from them.
    `_engine_prefix` + key is the engine's parameter name, `_engine_labels` its classifier width (0: a backbone)."""

    _engine_prefix = ""

    def _register(self, shapes=None, params=None):
        """Create the parameters of `shapes` (key -> shape, transformers' initialisation), or adopt `params` (key -> Parameter)."""
        self._names = {}
        for key in (shapes if params is None else params):
            if params is None:
                p = nn.Parameter(torch.zeros(shapes[key]), requires_grad=False)
                if "norm" in key and key.endswith("weight"):
                    nn.init.ones_(p)
                elif key.endswith("weight") or key.endswith("relative_position_bias_table"):
                    trunc_normal_(p, std=.02)
            else:
                p = params[key]
            flat = key.replace(".", "__")
            self.register_parameter(flat, p)
            self._names[flat] = key
        self._register_state_dict_hook(self._rename_out)
        self._register_load_state_dict_pre_hook(self._rename_in)
        self.__dict__["_engine_cache"] = SourceCache()  # "engine" -> dict(h, ws), made from every parameter, per device
        self.__dict__["_precision"] = "bf16"

    # ---- transformers key names in and out ----------------------------------------------------
    @staticmethod
    def _rename_out(module, state_dict, prefix, local_metadata):
        for flat, key in module._names.items():
            if prefix + flat in state_dict:
                state_dict[prefix + key] = state_dict.pop(prefix + flat)
        return state_dict

    def _rename_in(self, state_dict, prefix, *args):
        for flat, key in self._names.items():
            if prefix + key in state_dict:
                state_dict[prefix + flat] = state_dict.pop(prefix + key)

    def set_precision(self, precision):
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
        if precision != self._precision:
            self.__dict__["_precision"] = precision
            self._drop_engine()
        return self

    @property
    def _engine(self):  # the engine entry of the latest inference forward, or None
        return self._engine_cache.peek("engine")

    def _drop_engine(self):
        eng = self._engine
        if eng is not None:
            _lib.load().ocm_swin_destroy(eng["h"])
        self.__dict__["_engine_cache"] = SourceCache()

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    def _engine_params(self):
        """(flat name, parameter) of what the engine holds: every parameter, unless a subclass has some of its own."""
        return list(self.named_parameters())

    def _get_engine(self, device):
        named = self._engine_params()
        params = [p for _, p in named]
        sig = signature(params)
        eng = self._engine_cache.hit("engine", sig, device)
        if eng is not None:
            return eng
        self._drop_engine()
        lib, c = _lib.load(), self.config
        labels = self._engine_labels
        cfg = _lib.OcmSwinConfig(image_size=c.image_size, patch_size=c.patch_size, num_channels=c.num_channels,
                                 embed_dim=c.embed_dim, num_stages=c.num_layers, window_size=c.window_size,
                                 num_labels=labels, mlp_ratio=c.mlp_ratio, ln_eps=c.layer_norm_eps,
                                 precision=_lib.PRECISIONS[self._precision],
                                 reserved=0 if labels else _lib.OCM_SWIN_CFG_BACKBONE)
        for i in range(c.num_layers):
            cfg.depths[i], cfg.num_heads[i] = c.depths[i], c.num_heads[i]
        h = C.c_void_p(0)
        with torch.cuda.device(device):
            _lib.check(lib.ocm_swin_create(C.byref(cfg), C.byref(h)))
            for flat, p in named:
                if p.device != device:
                    lib.ocm_swin_destroy(h)
                    raise RuntimeError(f"parameters are on {p.device} but the input is on {device}; call model.to(device)")
                t = p.detach().to(torch.float32).contiguous()
                name = self._engine_prefix + self._names[flat]
                _lib.check(lib.ocm_swin_set_param(h, name.encode(), _p(t), t.numel(), _stream()))
            torch.cuda.current_stream().synchronize()
        return self._engine_cache.put("engine", sig, device, params, dict(h=h, ws={}, cfg=cfg, labels=labels))

    def _check_pixels(self, pixel_values):
        _require_hip(pixel_values, "pixel_values")
        c = self.config
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (c.num_channels, c.image_size, c.image_size):
            raise ValueError(f"expected (B, {c.num_channels}, {c.image_size}, {c.image_size}) pixel_values, got "
                             f"{tuple(pixel_values.shape)}")


def _check_swin_trainable(c, x, padded=False, wide=False):
    """What the Swin training path refuses, before anything is launched (SwinForImageClassification and
    SwinForMaskedImageModeling; `padded` / `wide`: the classifier's enable_padded_training / enable_wide_window_training)."""
    if x.requires_grad:
        raise NotImplementedError("the training path does not produce the gradient of the input image; pass pixel_values "
                                  "that do not require grad")
    if c.hidden_dropout_prob or c.attention_probs_dropout_prob:
        raise NotImplementedError(f"training is built without dropout (hidden_dropout_prob = {c.hidden_dropout_prob}, "
                                  f"attention_probs_dropout_prob = {c.attention_probs_dropout_prob}); set both to 0. "
                                  "Stochastic depth (drop_path_rate) is supported")
    if c.patch_size != 4 or not 2 <= c.window_size <= (12 if wide else 7):
        raise NotImplementedError("training is built for patch_size 4 and windows of 2 to 12" if wide else
                                  "training is built for patch_size 4 and windows of 2 to 7; "
                                  "model.enable_wide_window_training() trains windows of 8 to 12")
    side = c.image_size // c.patch_size
    hint = "; model.enable_padded_training() trains through transformers' padding paths"
    for s in range(c.num_layers):
        if c.embed_dim * 2 ** s != 32 * c.num_heads[s] or c.embed_dim % 32 or c.embed_dim > 128:
            raise NotImplementedError(f"stage {s}: training is built for 32-wide heads and embed_dim a multiple of 32 "
                                      "up to 128")
        if padded and side < c.window_size:
            raise NotImplementedError(f"stage {s}: its {side} x {side} grid is smaller than window_size {c.window_size}; "
                                      "neither training nor inference is built for that")
        if not padded and (side < c.window_size or side % c.window_size):
            raise NotImplementedError(f"stage {s}: its {side} x {side} grid is not a multiple of window_size "
                                      f"{c.window_size}; training is built for geometries without transformers' padding "
                                      "paths (every stage grid a multiple of the window, even before each merge)" + hint)
        if s + 1 < c.num_layers:
            if side % 2 and not padded:
                raise NotImplementedError(f"stage {s}: the odd {side} x {side} grid would be padded before the patch "
                                          "merging; training is built for geometries without transformers' padding paths"
                                          + hint)
            side = (side + 1) // 2


class SwinForImageClassification(_SwinBase):
    """transformers' SwinForImageClassification: the classifier on the pooled output of the backbone (`.swin`).

    forward(pixel_values, labels=None, output_hidden_states=False, output_attentions=False):
      * output_hidden_states=True: `last_hidden_state` (the final LayerNorm's output, this path's own attribute), and in
        inference `hidden_states` (num_stages + 1 token-major tensors: the embeddings output, every stage's output after its
        patch merging, the last one before the final LayerNorm) and `reshaped_hidden_states` (the same as (B, C, H, W)).
      * output_attentions=True (or an iterable of global layer indices): `attentions`, a tuple with one
        (B * nW, heads, ws^2, ws^2) tensor per layer (None for a layer not asked for), nW counted on the padded grid. The
        layers up to the last one asked for run their attention half unfused (a map does not depend on which other maps
        are asked for); in split-bf16 the other outputs then agree with the plain call to fp32 rounding, in fp32 and bf16
        bit for bit.
      * in training mode (module.train(), grad mode on, a parameter requiring grad) the attention maps are not built:
        output_attentions raises NotImplementedError, and hidden_states / reshaped_hidden_states are None (the training
        forward keeps what its backward needs, not the stage outputs); last_hidden_state is returned as before."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.num_labels = config.num_labels
        self._register(shapes=_param_shapes(config))

    @property
    def _engine_labels(self):
        return self.config.num_labels

    @property
    def swin(self):
        """The backbone as a SwinModel over this module's own Parameter objects and engine (no second packed copy of the
        weights): `model.swin(pixel_values, output_hidden_states=True)` after fine-tuning the classifier. The view is built on
        access and is not a submodule: state_dict(), parameters() and named_parameters() of the classifier do not see it."""
        return SwinModel._view_of(self)

    def forward(self, pixel_values=None, labels=None, output_hidden_states=False, output_attentions=False, **unused):
        self._check_pixels(pixel_values)
        if _differentiable(self):
            if _layer_list(self.config, output_attentions):
                raise NotImplementedError("attention maps are built in inference only: call model.eval() (or run under "
                                          "torch.no_grad()) to get `attentions`")
            return self._train_forward(pixel_values, labels, output_hidden_states)
        with torch.no_grad():
            return self._infer(pixel_values, labels, output_hidden_states, _layer_list(self.config, output_attentions))

    # ---- training ----------------------------------------------------------------------------------------------------------
    def enable_padded_training(self, on=True):
        """Opt in to training on the geometries that need transformers' padding paths: a stage grid that is not a multiple of
        the window (SwinLayer.maybe_pad: Swin-T on a 384^2 tile has grids 96 / 48 / 24 / 12 for windows of 7) or an odd grid
        before a patch merging. A per-module setting, not part of the state_dict; geometries without padding launch what
        they launch without it. Returns self."""
        self.__dict__["_padded_training"] = bool(on)
        return self

    def enable_wide_window_training(self, on=True):
        """Opt in to training with windows of 8 to 12 (the window12-384 checkpoints: grids 96 / 48 / 24 / 12 on a 384^2 tile,
        no padding in any stage): their window-attention backward is ocm_op_swin_window_attention_backward_wide. A per-module
        setting, not part of the state_dict; windows of 2 to 7 launch what they launch without it. Composes with
        enable_padded_training (image 80 with windows of 8 pads 20 -> 24 and 10 -> 16). Returns self."""
        self.__dict__["_wide_window_training"] = bool(on)
        return self

    def _check_trainable(self, x, labels):
        """What the training path refuses, before anything is launched."""
        c = self.config
        _check_swin_trainable(c, x, self.__dict__.get("_padded_training", False),
                              self.__dict__.get("_wide_window_training", False))
        if labels is not None:
            if c.num_labels < 2:
                raise ValueError(f"training with labels is built for single-label classification with num_labels >= 2 (got "
                                 f"{c.num_labels}); the regression and multi-label losses are not built")
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
                raise ValueError("labels must be int64 class indices (single-label classification), got "
                                 f"{getattr(labels, 'dtype', type(labels))}")

    def _train_forward(self, pixel_values, labels, output_hidden_states):
        self._check_trainable(pixel_values, labels)
        x = pixel_values.detach().to(torch.float32).contiguous()
        dev = x.device
        named = [(self._names[n], p) for n, p in self.named_parameters()]
        for key, p in named:
            if p.device != dev:
                raise RuntimeError(f"parameters are on {p.device} but the input is on {dev}; call model.to(device)")
        meta = {"model": self, "keys": [k for k, _ in named],
                "masks": draw_drop_path_masks(self.config, x.shape[0], dev)}
        with torch.cuda.device(dev):
            logits, pooled = _SwinTrain.apply(meta, x, *[p for _, p in named])
        self.__dict__["_train_kept_bytes"] = meta["kept_bytes"]  # what the backward holds
        loss = None
        if labels is not None:
            loss = nn.functional.cross_entropy(logits, labels.to(dev))
        hidden = meta["hidden"] if output_hidden_states else None  # the final LayerNorm's output, without a graph
        return SwinOutput(loss=loss, logits=logits, pooler_output=pooled, last_hidden_state=hidden, hidden_states=None,
                          reshaped_hidden_states=None, attentions=None)

    # ---- inference ---------------------------------------------------------------------------------------------------------
    def _infer(self, pixel_values, labels, output_hidden_states, layers=()):
        r = _engine_run(self._get_engine(pixel_values.device), self.config, pixel_values, output_hidden_states,
                        output_hidden_states, list(layers))
        loss = None
        if labels is not None:
            loss = nn.functional.cross_entropy(r["logits"], labels.to(pixel_values.device))
        return SwinOutput(loss=loss, logits=r["logits"], pooler_output=r["pooled"], last_hidden_state=r["last_hidden"],
                          hidden_states=r["hidden_states"], reshaped_hidden_states=r["reshaped_hidden_states"],
                          attentions=r["attentions"])


class SwinModel(_SwinBase):
    """transformers' SwinModel: the backbone without the classifier, inference only. Parameters are registered under
    transformers' SwinModel keys (the classifier model's keys without the `swin.` prefix and without classifier.*).

    forward(pixel_values, output_hidden_states=False, output_attentions=False) -> SwinModelOutput(last_hidden_state,
    pooler_output (None when add_pooling_layer=False), hidden_states, reshaped_hidden_states, attentions), the three
    tuples as SwinForImageClassification.forward describes them. The `.swin` view of a SwinForMaskedImageModeling holds its
    `embeddings.mask_token`; its forward(bool_masked_pos=...) takes a torch.bool (B, L_0) tensor and replaces the masked tokens
    of the embeddings output by the token (ocm_swin_forward_masked; any other dtype raises ValueError). Not built
    (NotImplementedError): use_mask_token=True on a stand-alone SwinModel, a bool_masked_pos on a model without the token
    (MaskTokenMissing, refused before anything else as it always was), interpolate_pos_encoding=True, and training (training
    mode with a parameter that requires grad)."""

    _engine_prefix = "swin."
    _engine_labels = 0

    def __init__(self, config, add_pooling_layer=True, use_mask_token=False):
        super().__init__()
        if use_mask_token:
            raise NotImplementedError("use_mask_token=True is not built for a stand-alone SwinModel: the mask token lives in "
                                      "SwinForMaskedImageModeling, whose `.swin` is the backbone with it")
        self.config = config
        self.add_pooling_layer = add_pooling_layer
        self.__dict__["_owner"] = None
        self._register(shapes={k[len("swin."):]: v for k, v in _param_shapes(config).items() if k.startswith("swin.")})

    @classmethod
    def _view_of(cls, owner, add_pooling_layer=True):
        """A SwinModel over the `swin.*` Parameter objects of a SwinForImageClassification or SwinForMaskedImageModeling,
        running through its engine."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.config, self.add_pooling_layer = owner.config, add_pooling_layer
        self.__dict__["_owner"] = owner
        self._register(params={owner._names[flat][len("swin."):]: p for flat, p in owner.named_parameters()
                               if owner._names[flat].startswith("swin.")})
        self.__dict__["_precision"] = owner._precision
        self.training = owner.training
        return self

    def set_precision(self, precision):
        if self._owner is not None:  # one engine, the owner's
            self._owner.set_precision(precision)
            self.__dict__["_precision"] = self._owner._precision
            return self
        return super().set_precision(precision)

    def forward(self, pixel_values=None, bool_masked_pos=None, output_hidden_states=False, output_attentions=False,
                interpolate_pos_encoding=False, **unused):
        has_token = "embeddings.mask_token" in self._names.values()
        if bool_masked_pos is not None and not has_token:
            _patch_mask(self.config, pixel_values, bool_masked_pos, False)  # raises MaskTokenMissing, before anything else
        if interpolate_pos_encoding:
            raise NotImplementedError("interpolate_pos_encoding=True is not built: pixel_values must be config.image_size wide")
        self._check_pixels(pixel_values)
        if _differentiable(self):
            raise NotImplementedError("SwinModel is inference only: call .eval(), run under torch.no_grad(), or train "
                                      "through SwinForImageClassification")
        layers = _layer_list(self.config, output_attentions)
        mask = _patch_mask(self.config, pixel_values, bool_masked_pos, has_token)
        with torch.no_grad():
            eng = (self._owner if self._owner is not None else self)._get_engine(pixel_values.device)
            r = _engine_run(eng, self.config, pixel_values, True, output_hidden_states, layers, mask)
        return SwinModelOutput(last_hidden_state=r["last_hidden"], pooler_output=r["pooled"] if self.add_pooling_layer else None,
                               hidden_states=r["hidden_states"], reshaped_hidden_states=r["reshaped_hidden_states"],
                               attentions=r["attentions"])


class SwinForMaskedImageModeling(_SwinBase):
    """transformers' SwinForMaskedImageModeling (SimMIM pre-training; the checkpoint microsoft/swin-base-simmim-window6-192
    loads with load_state_dict): the backbone with a mask token and without a pooler (`.swin`), and the decoder
    Conv2d(hidden_size, encoder_stride^2 * num_channels, 1) + PixelShuffle(encoder_stride) under the keys decoder.0.weight /
    decoder.0.bias.

    forward(pixel_values, bool_masked_pos=None, output_hidden_states=False, output_attentions=False) ->
    SwinMaskedImageModelingOutput(loss, reconstruction, hidden_states, attentions, reshaped_hidden_states). bool_masked_pos is a
    torch.bool (B, L_0) tensor over the patch grid (data.MaskGenerator's layout, flattened); the loss is SimMIM's masked L1,
    sum |x - rec| * m / (sum m + 1e-5) / num_channels with m the mask repeated over each patch's pixels, and None without a mask.
      * inference (eval mode, no_grad, or nothing trainable): the engine's masked forward, the decoder GEMM on
        last_hidden_state in the module's precision, then ocm_op_mim_l1_loss for the reconstruction and the loss.
      * training (module.train(), grad mode on, a parameter requiring grad): _SwinTrain with the sequence ending and the mask
        select in its embeddings unit, then _MimHead (one GEMM + ocm_op_mim_l1_loss, which leaves the loss gradient in the
        GEMM's row layout). Stochastic depth as in the classifier; hidden_states and attentions are inference only.
    The geometries of the classifier's training path without its opt-ins (patch 4, 32-wide heads, windows of 2 to 7 on grids
    that are multiples of the window), no dropout."""

    _engine_labels = 0

    def __init__(self, config):
        super().__init__()
        if config.encoder_stride != config.patch_size * 2 ** (config.num_layers - 1):
            raise ValueError(f"encoder_stride {config.encoder_stride} must be patch_size * 2^(num_layers - 1) = "
                             f"{config.patch_size * 2 ** (config.num_layers - 1)}: the decoder's PixelShuffle has to give the "
                             "image back")
        self.config = config
        shapes = {k: v for k, v in _param_shapes(config).items() if k.startswith("swin.")}
        shapes["swin.embeddings.mask_token"] = (1, 1, config.embed_dim)
        shapes["decoder.0.weight"] = (config.encoder_stride ** 2 * config.num_channels, config.hidden_size, 1, 1)
        shapes["decoder.0.bias"] = (config.encoder_stride ** 2 * config.num_channels,)
        self._register(shapes=shapes)

    def _engine_params(self):  # the decoder is not the engine's
        return [(flat, p) for flat, p in self.named_parameters() if self._names[flat].startswith("swin.")]

    @property
    def swin(self):
        """The backbone as a SwinModel (with the mask token, no pooling layer) over this module's own Parameter objects and
        engine; built on access, not a submodule."""
        return SwinModel._view_of(self, add_pooling_layer=False)

    def forward(self, pixel_values=None, bool_masked_pos=None, output_hidden_states=False, output_attentions=False,
                interpolate_pos_encoding=False, **unused):
        if interpolate_pos_encoding:
            raise NotImplementedError("interpolate_pos_encoding=True is not built: pixel_values must be config.image_size wide")
        self._check_pixels(pixel_values)
        mask = _patch_mask(self.config, pixel_values, bool_masked_pos, True)
        layers = _layer_list(self.config, output_attentions)
        if _differentiable(self):
            if layers or output_hidden_states:
                raise NotImplementedError("hidden_states and attentions are built in inference only: call model.eval() (or "
                                          "run under torch.no_grad())")
            return self._train_forward(pixel_values, mask)
        with torch.no_grad():
            return self._infer(pixel_values, mask, output_hidden_states, layers)

    def _named(self, dev):
        named = [(self._names[n], p) for n, p in self.named_parameters()]
        for key, p in named:
            if p.device != dev:
                raise RuntimeError(f"parameters are on {p.device} but the input is on {dev}; call model.to(device)")
        return named

    def _train_forward(self, pixel_values, mask):
        _check_swin_trainable(self.config, pixel_values)
        x = pixel_values.detach().to(torch.float32).contiguous()
        dev = x.device
        named = self._named(dev)
        trunk = [(k, p) for k, p in named if k.startswith("swin.")]
        P = dict(named)
        meta = {"model": self, "keys": [k for k, _ in trunk], "ending": "sequence", "patch_mask": mask,
                "masks": draw_drop_path_masks(self.config, x.shape[0], dev)}
        with torch.cuda.device(dev):
            seq = _SwinTrain.apply(meta, x, *[p for _, p in trunk])
            loss, rec = _MimHead.apply({"model": self}, seq, P["decoder.0.weight"], P["decoder.0.bias"], x, mask)
        self.__dict__["_train_kept_bytes"] = meta["kept_bytes"]
        return SwinMaskedImageModelingOutput(loss=loss if mask is not None else None, reconstruction=rec, hidden_states=None,
                                             attentions=None, reshaped_hidden_states=None)

    def _infer(self, pixel_values, mask, output_hidden_states, layers=()):
        dev = pixel_values.device
        r = _engine_run(self._get_engine(dev), self.config, pixel_values, True, output_hidden_states, list(layers), mask)
        P = dict(self._named(dev))
        x = pixel_values.detach().to(torch.float32).contiguous()
        with torch.cuda.device(dev):
            _, rec, loss = _mim_head_forward(self, P, r["last_hidden"], x, mask, False)
        return SwinMaskedImageModelingOutput(loss=loss, reconstruction=rec, hidden_states=r["hidden_states"],
                                             attentions=r["attentions"], reshaped_hidden_states=r["reshaped_hidden_states"])


# ---- training: SwinForImageClassification as stand-alone operators under one autograd Function. Token-major rows
# m = (image, y, x); T = B * H * W tokens of a stage with C channels. ----
def _kpad(K, prec):
    """K rounded up to the GEMM operands' K step: 64 for bf16, 32 for fp32 and split pairs."""
    step = 64 if prec == _lib.OCM_PREC_BF16 else 32
    return -(-K // step) * step


def _pad_cols(t, K):
    return t if t.shape[1] == K else F.pad(t, (0, K - t.shape[1]))


def _operand(t32, prec):
    """fp32 [M][K] -> the GEMM operand [M][kpad(K)], padding columns zero."""
    return to_operand(_pad_cols(t32, _kpad(t32.shape[1], prec)), prec)


def _pad_rows(lib, src, B, H, Hp):
    """Rows (B * H * H, n) of any element type -> (B * Hp * Hp, n): SwinLayer.maybe_pad, zeros right of and below the grid."""
    dst = torch.empty((B * Hp * Hp, src.shape[1]), dtype=src.dtype, device=src.device)
    _lib.check(lib.ocm_op_swin_pad_rows(_p(src), _p(dst), B, H, H, Hp, Hp, src.shape[1] * src.element_size(), _stream()))
    return dst


def _crop_rows(lib, src, B, H, Hp):
    """The inverse: rows (B * Hp * Hp, n) -> the (B * H * H, n) at the real positions."""
    dst = torch.empty((B * H * H, src.shape[1]), dtype=src.dtype, device=src.device)
    _lib.check(lib.ocm_op_swin_crop_rows(_p(src), _p(dst), B, H, H, Hp, Hp, src.shape[1] * src.element_size(), _stream()))
    return dst


class _Weights:
    """Operand copies of weight matrices ([N][K] and the transposes the data gradients read), K zero-padded to the operand's
    K step, cached in the module under the parameters they are made from and the precision (engine.SourceCache): an optimizer
    step or load_state_dict makes new copies, an unchanged parameter is not repacked."""

    def __init__(self, model, P, prec):
        self.cache, self.P, self.prec = model.__dict__.setdefault("_train_cache", SourceCache()), P, prec

    def _mat(self, keys, rows):
        w = torch.cat([self.P[k].detach().float().reshape(self.P[k].shape[0], -1) for k in keys])
        return F.pad(w, (0, 0, 0, rows - w.shape[0])) if rows and rows > w.shape[0] else w

    def w(self, *keys, rows=None):
        """cat(keys) as [N][K] (rows zero-padded up to `rows`)."""
        return self.cache.get(keys, [self.P[k] for k in keys], lambda: _operand(self._mat(keys, rows), self.prec), self.prec)

    def wt(self, *keys, rows=None):
        """The transpose [K][N] of w(*keys, rows=rows): the data gradient dX = dY W runs as a linear with W^T."""
        return self.cache.get(("T",) + keys, [self.P[k] for k in keys],
                              lambda: _operand(self._mat(keys, rows).t().contiguous(), self.prec), self.prec)


def _ctx_f32(cx, C, prec):
    """The window attention's context (operand rows of kpad(C) columns) as fp32 [T][C]."""
    if prec == _lib.OCM_PREC_BF16X3:
        return from_split(cx)
    if prec == _lib.OCM_PREC_FP32:
        return cx
    return cx[:, :C].float().contiguous()


class _SwinTrain(torch.autograd.Function):
    """SwinForImageClassification in training mode: forward(meta, pixel_values, *params) -> (logits, pooled); backward ->
    parameter gradients (the image gets none). The forward runs the stand-alone operators in the module's precision (not the
    engine, not the fused Swin kernels): patch unfold + GEMM + LayerNorm, per layer LayerNorm -> q | k | v GEMM (fp32) ->
    window attention (on the grid padded to the window where enable_padded_training applies: operand rows zero-padded before
    the projection, the context cropped after the attention) -> o_proj (+ drop path) -> LayerNorm -> fc1 (fp32
    pre-activation) -> GELU -> fc2, the merging LayerNorm +
    reduction, the final LayerNorm, token mean and classifier (rows zero-padded to a multiple of 32). Kept per layer: the two
    LayerNorm inputs, the fp32 q | k | v, the context in operand form and the fp32 fc1 pre-activation; per merge its input;
    LayerNorm statistics and outputs are recomputed in the backward."""

    @staticmethod
    def forward(ctx, meta, x, *params):
        model = meta["model"]
        c = model.config
        P = dict(zip(meta["keys"], params))
        lib, dev = _lib.load(), x.device
        prec = _lib.PRECISIONS[model._precision]
        f32 = dict(device=dev, dtype=torch.float32)
        adt = OPERAND_DTYPE[prec]
        W = _Weights(model, P, prec)
        eps, F32 = float(c.layer_norm_eps), _lib.OCM_LN_F32
        B, Cin, S = x.shape[0], c.num_channels, c.image_size
        H, C = S // c.patch_size, c.embed_dim
        ctx.set_materialize_grads(False)

        # embeddings: Conv2d(p = 4, stride 4) as patch rows (K = Cin * 16 zero-padded) x weight, then embeddings.norm (eps 1e-5)
        e = "swin.embeddings."
        T = B * H * H
        cols = torch.empty((T, Cin * 16), **f32)
        _lib.check(lib.ocm_op_patch_unfold(_p(x), _p(cols), B, Cin, S, S, c.patch_size, _stream()))
        tok = _linear(lib, prec, _operand(cols, prec), W.w(e + "patch_embeddings.projection.weight"),
                      P[e + "patch_embeddings.projection.bias"], None, T, C, _kpad(Cin * 16, prec))
        del cols
        t = _ln(lib, tok, P[e + "norm.weight"], P[e + "norm.bias"], F32, T, C, 1e-5, torch.float32)
        pmask = meta.get("patch_mask")  # uint8 (B, L_0) or None: SwinEmbeddings' mask-token select, after embeddings.norm
        if pmask is not None:
            _lib.check(lib.ocm_op_swin_mask_tokens(_p(t), _p(pmask), _p(P[e + "mask_token"].detach().contiguous()), T, C,
                                                   _stream()))
        keep = [tok]  # tensors for the backward, in this order: tok, per layer 6, per merge 1, final input, pooled
        masks, li = meta["masks"], 0
        for s in range(c.num_layers):
            heads, M, ws = c.num_heads[s], int(c.mlp_ratio * C), c.window_size
            T, Kc, Km = B * H * H, _kpad(C, prec), _kpad(M, prec)
            Hp = -(-H // ws) * ws  # the grid padded to the window (enable_padded_training); Hp = H elsewhere
            Tp = B * Hp * Hp
            for b in range(c.depths[s]):
                pre = f"swin.encoder.layers.{s}.blocks.{b}."
                a = pre + "attention."
                shift = ws // 2 if b % 2 and H > ws else 0  # set_shift_and_window_size: no shift when the grid is the window
                xn = _ln(lib, t, P[pre + "layernorm_before.weight"], P[pre + "layernorm_before.bias"], F32, T, C, eps,
                         torch.float32)
                xo = _operand(xn, prec)
                del xn
                if Hp != H:  # SwinLayer.maybe_pad: zero rows after layernorm_before; their q | k | v is the projection bias
                    xo = _pad_rows(lib, xo, B, H, Hp)
                qkv = _linear(lib, prec, xo, W.w(a + "q_proj.weight", a + "k_proj.weight", a + "v_proj.weight"),
                              torch.cat([P[a + n + "_proj.bias"] for n in "qkv"]), None, Tp, 3 * C, Kc)
                del xo
                cx = torch.zeros((Tp, Kc), dtype=adt, device=dev)
                scratch = torch.empty(lib.ocm_swin_window_scratch_floats(ws, heads), **f32)
                table = P[a + "relative_position_bias.relative_position_bias_table"]
                _lib.check(lib.ocm_op_swin_window_attention(prec, _p(to_operand(qkv, prec)), 3 * C, _p(cx), Kc, _p(table),
                                                            _p(scratch), B, Hp, Hp, ws, shift, heads, _stream()))
                if Hp != H:  # the padded positions' context is dropped; o_proj is row-wise and runs on the real rows
                    cx = _crop_rows(lib, cx, B, H, Hp)
                wo, bo = W.w(a + "o_proj.weight"), P[a + "o_proj.bias"]
                scale = None
                if masks[li] is None:
                    x1 = _linear(lib, prec, cx, wo, bo, t, T, C, Kc, _lib.OCM_EPI_BIAS_RESID_F32)
                else:  # SwinDropPath on the attention branch: x1 = t + branch * mask / keep_prob per image
                    kp, mask = masks[li]
                    scale = (mask / kp).contiguous()
                    br = _linear(lib, prec, cx, wo, bo, None, T, C, Kc)
                    x1 = torch.empty((T, C), **f32)
                    _lib.check(lib.ocm_op_swin_drop_path(_p(t), _p(br), _p(scale), _p(x1), B, H * H, C, _stream()))
                    del br
                xn2 = _ln(lib, x1, P[pre + "layernorm_after.weight"], P[pre + "layernorm_after.bias"], F32, T, C, eps,
                          torch.float32)
                hpre = _linear(lib, prec, _operand(xn2, prec), W.w(pre + "mlp.fc1.weight"), P[pre + "mlp.fc1.bias"], None, T,
                               M, Kc)
                del xn2
                if Km == M:
                    g = torch.empty((T, M), dtype=adt, device=dev)
                    _lib.check(lib.ocm_op_gelu(prec, _p(hpre), _p(g), None, T * M, _stream()))
                else:
                    g32 = torch.empty((T, M), **f32)
                    _lib.check(lib.ocm_op_gelu(_lib.OCM_PREC_FP32, _p(hpre), _p(g32), None, T * M, _stream()))
                    g = _operand(g32, prec)
                    del g32
                x2 = _linear(lib, prec, g, W.w(pre + "mlp.fc2.weight"), P[pre + "mlp.fc2.bias"], x1, T, C, Km,
                             _lib.OCM_EPI_BIAS_RESID_F32)
                del g
                keep += [t, qkv, cx, x1, hpre, scale]
                t, li = x2, li + 1
            if s + 1 < c.num_layers:  # SwinPatchMerging: gather + LayerNorm(4C) in one kernel, then the reduction
                dn = f"swin.encoder.layers.{s}.downsample."
                H2 = (H + 1) // 2  # SwinPatchMerging.maybe_pad: an odd grid gets a zero row and column (in the kernel)
                T4, K4 = B * H2 * H2, _kpad(4 * C, prec)
                y = torch.empty((T4, K4), dtype=adt, device=dev)
                _lib.check(lib.ocm_op_swin_merge_ln(prec, _p(t), _p(P[dn + "norm.weight"]), _p(P[dn + "norm.bias"]), _p(y), B,
                                                    H, H, C, K4, _stream()))
                keep.append(t)
                t = _linear(lib, prec, y, W.w(dn + "reduction.weight"), torch.zeros(2 * C, **f32), None, T4, 2 * C, K4)
                del y
                H, C = H2, 2 * C
        # head: final LayerNorm, token mean, classifier
        L, nl = H * H, c.num_labels
        NLp = -(-nl // 32) * 32
        seq = _ln(lib, t, P["swin.layernorm.weight"], P["swin.layernorm.bias"], F32, B * L, C, eps, torch.float32)
        if meta.get("ending") == "sequence":  # SwinForMaskedImageModeling: the sequence output, no pool and no classifier
            keep += [t, None]
            meta["kept_bytes"] = sum(k.numel() * k.element_size() for k in keep if k is not None)
            ctx.meta, ctx.prec = meta, prec
            ctx.save_for_backward(x, *keep, *params)
            return seq.view(B, L, C)
        pooled = torch.empty((B, C), **f32)
        _lib.check(lib.ocm_op_swin_pool(_p(seq), _p(pooled), B, L, C, _stream()))
        meta["hidden"] = seq.view(B, L, C)
        logits = _linear(lib, prec, _operand(pooled, prec), W.w("classifier.weight", rows=NLp),
                         F.pad(P["classifier.bias"].detach(), (0, NLp - nl)), None, B, NLp, _kpad(C, prec))
        keep += [t, pooled]
        meta["kept_bytes"] = sum(k.numel() * k.element_size() for k in keep if k is not None)
        # through save_for_backward: autograd frees them after the backward, refuses a second backward over the same graph and
        # raises if a parameter is modified in place between this forward and the backward
        ctx.meta, ctx.prec = meta, prec
        ctx.save_for_backward(x, *keep, *params)
        return logits[:, :nl].contiguous(), pooled

    @staticmethod
    def backward(ctx, *douts):
        meta, prec = ctx.meta, ctx.prec
        sequence = meta.get("ending") == "sequence"
        dlogits, dpooled = (None, None) if sequence else douts
        model, keys = meta["model"], meta["keys"]
        c = model.config
        lib = _lib.load()
        st = ctx.saved_tensors
        nkeep = len(st) - 1 - len(keys)
        x, keep, P = st[0], list(st[1:1 + nkeep]), dict(zip(keys, st[1 + nkeep:]))
        need = dict(zip(keys, ctx.needs_input_grad[2:]))
        dev = x.device
        f32 = dict(device=dev, dtype=torch.float32)
        W = _Weights(model, P, prec)
        eps = float(c.layer_norm_eps)
        grads = {}

        # units in forward order: the backward walks them in reverse and stops after the earliest one that has a parameter
        # needing a gradient (a classifier-only fine-tune does not walk the encoder)
        units = [("emb", "swin.embeddings.")]
        for s in range(c.num_layers):
            units += [("layer", f"swin.encoder.layers.{s}.blocks.{b}.") for b in range(c.depths[s])]
            if s + 1 < c.num_layers:
                units.append(("merge", f"swin.encoder.layers.{s}.downsample."))
        units.append(("head", None))
        heads_keys = ("swin.layernorm.weight", "swin.layernorm.bias", "classifier.weight", "classifier.bias")
        wanted = [any(need[k] for k in keys if (k.startswith(pre) if pre else k in heads_keys)) for _, pre in units]
        if True not in wanted:  # the sequence ending with a frozen trunk behind a graph of the caller's: nothing to walk
            return (None, None, *[None] * len(keys))
        stop = wanted.index(True)

        def wgrad(dy, xin, wkey, bkey, rows=None):
            if need.get(wkey) or (bkey and need.get(bkey)):
                dw, db = _weight_grad(prec, dy, xin, bool(bkey and need.get(bkey)))
                if need.get(wkey):
                    grads[wkey] = dw[:rows] if rows else dw
                if bkey and need.get(bkey):
                    grads[bkey] = db[:rows] if rows else db

        def lngrads(pre, dg, db):
            for k, v in ((pre + "weight", dg), (pre + "bias", db)):
                if need[k]:
                    grads[k] = v

        # geometry of every unit, walking forward
        geo, H, C = [], c.image_size // c.patch_size, c.embed_dim
        B = x.shape[0]
        for s in range(c.num_layers):
            geo += [(s, b, H, C) for b in range(c.depths[s])]
            if s + 1 < c.num_layers:
                geo.append((s, None, H, C))
                H, C = (H + 1) // 2, 2 * C
        L, nl = H * H, c.num_labels
        NLp = -(-nl // 32) * 32
        tL, pooled = keep[-2], keep[-1]
        with torch.cuda.device(dev):
            dx = None
            if sequence:  # the backward starts from d_seq: the final LayerNorm, then the units
                if douts[0] is None:
                    return (None, None, *[None] * len(keys))
                dseq = douts[0].detach().to(torch.float32).contiguous().view(B * L, C)
                dx, dg, db = _ln_backward(lib, dseq, tL, P["swin.layernorm.weight"], None, B * L, C, eps)
                lngrads("swin.layernorm.", dg, db)
            else:
                # head: logits = pooled W^T + b (rows padded to NLp), pooled = mean_l LayerNorm(tL)
                dl = torch.zeros((B, NLp), **f32)
                if dlogits is not None:
                    dl[:, :nl] = dlogits
                wgrad(dl, pooled, "classifier.weight", "classifier.bias", rows=nl)
                if stop < len(units) - 1 or need["swin.layernorm.weight"] or need["swin.layernorm.bias"]:
                    dp = _linear(lib, prec, _operand(dl, prec), W.wt("classifier.weight", rows=NLp), torch.zeros(C, **f32), None,
                                 B, C, _kpad(NLp, prec))
                    if dpooled is not None:
                        dp = dp + dpooled
                    dseq = torch.empty((B * L, C), **f32)
                    _lib.check(lib.ocm_op_swin_pool_backward(_p(dp), _p(dseq), B, L, C, _stream()))
                    dx, dg, db = _ln_backward(lib, dseq, tL, P["swin.layernorm.weight"], None, B * L, C, eps)
                    lngrads("swin.layernorm.", dg, db)
            ki = len(keep) - 2
            for u in reversed(range(1, len(units) - 1)):
                if u < stop:
                    break
                kind, pre = units[u]
                s, b, H, C = geo[u - 1]
                T = B * H * H
                if kind == "merge":
                    ki -= 1
                    xin = keep[ki]
                    T4, C2 = B * ((H + 1) // 2) ** 2, 2 * C
                    odd = "_pad" if H % 2 else ""  # the gather / scatter that append the zero row and column
                    if need[pre + "reduction.weight"]:
                        y32 = torch.empty((T4, 4 * C), **f32)
                        _lib.check(lib.ocm_op_swin_merge_ln(_lib.OCM_PREC_FP32, _p(xin), _p(P[pre + "norm.weight"]),
                                                            _p(P[pre + "norm.bias"]), _p(y32), B, H, H, C, 4 * C, _stream()))
                        wgrad(dx, y32, pre + "reduction.weight", None)
                        del y32
                    dy = _linear(lib, prec, _operand(dx, prec), W.wt(pre + "reduction.weight"), torch.zeros(4 * C, **f32), None,
                                 T4, 4 * C, _kpad(C2, prec))
                    gth = torch.empty((T4, 4 * C), **f32)
                    _lib.check(getattr(lib, "ocm_op_swin_merge_gather" + odd)(_p(xin), _p(gth), B, H, H, C, _stream()))
                    dg4, dg, db = _ln_backward(lib, dy, gth, P[pre + "norm.weight"], None, T4, 4 * C, 1e-5)
                    lngrads(pre + "norm.", dg, db)
                    del dy, gth
                    dx = torch.empty((T, C), **f32)
                    _lib.check(getattr(lib, "ocm_op_swin_merge_scatter" + odd)(_p(dg4), _p(dx), B, H, H, C, _stream()))
                    continue
                # a SwinLayer: x1 = t + drop_path(o_proj(attn(LN1(t)))), x2 = x1 + fc2(gelu(fc1(LN2(x1))))
                ki -= 6
                t, qkv, cx, x1, hpre, scale = keep[ki:ki + 6]
                heads, M, ws = c.num_heads[s], int(c.mlp_ratio * C), c.window_size
                shift = ws // 2 if b % 2 and H > ws else 0
                Hp = -(-H // ws) * ws
                Tp = B * Hp * Hp
                a = pre + "attention."
                dh = _linear(lib, prec, _operand(dx, prec), W.wt(pre + "mlp.fc2.weight"), torch.zeros(M, **f32), None, T, M,
                             _kpad(C, prec))
                g32 = torch.empty((T, M), **f32)
                _lib.check(lib.ocm_op_gelu_backward(_p(dh), _p(hpre), _p(dh), _p(g32), T * M, _stream()))
                wgrad(dx, g32, pre + "mlp.fc2.weight", pre + "mlp.fc2.bias")
                del g32
                g2 = P[pre + "layernorm_after.weight"]
                if need[pre + "mlp.fc1.weight"] or need[pre + "mlp.fc1.bias"]:
                    xn2 = _ln(lib, x1, g2, P[pre + "layernorm_after.bias"], _lib.OCM_LN_F32, T, C, eps, torch.float32)
                    wgrad(dh, xn2, pre + "mlp.fc1.weight", pre + "mlp.fc1.bias")
                    del xn2
                dxn2 = _linear(lib, prec, _operand(dh, prec), W.wt(pre + "mlp.fc1.weight"), torch.zeros(C, **f32), None, T, C,
                               _kpad(M, prec))
                del dh
                dx1, dg, db = _ln_backward(lib, dxn2, x1, g2, dx, T, C, eps)
                lngrads(pre + "layernorm_after.", dg, db)
                del dxn2, dx
                dbr = dx1
                if scale is not None:
                    dbr = torch.empty((T, C), **f32)
                    _lib.check(lib.ocm_op_swin_drop_path_backward(_p(dx1), _p(scale), _p(dbr), B, H * H, C, _stream()))
                if need[a + "o_proj.weight"] or need[a + "o_proj.bias"]:
                    wgrad(dbr, _ctx_f32(cx, C, prec), a + "o_proj.weight", a + "o_proj.bias")
                dctx = _linear(lib, prec, _operand(dbr, prec), W.wt(a + "o_proj.weight"), torch.zeros(C, **f32), None, T, C,
                               _kpad(C, prec))
                del dbr
                if Hp != H:  # the crop's gradient: zeros at the padded positions
                    dctx = _pad_rows(lib, dctx, B, H, Hp)
                tkey = a + "relative_position_bias.relative_position_bias_table"
                dqkv = torch.empty((Tp, 3 * C), **f32)
                dtab = torch.empty(P[tkey].shape, **f32)
                wide = "_wide" if ws > 7 else ""  # windows of 8 to 12: the MFMA backward (enable_wide_window_training)
                nbytes = getattr(lib, f"ocm_swin_window_attention_backward{wide}_workspace_bytes")(B, Hp, Hp, ws, heads)
                wsb = _ws(nbytes, dev)
                _lib.check(getattr(lib, "ocm_op_swin_window_attention_backward" + wide)(
                    _p(qkv), _p(dctx), _p(P[tkey]), _p(dqkv), _p(dtab), B, Hp, Hp, ws, shift, heads, _p(wsb), nbytes, _stream()))
                if need[tkey]:
                    grads[tkey] = dtab
                del dctx, wsb
                g1 = P[pre + "layernorm_before.weight"]
                pk = [a + n + "_proj." for n in "qkv"]
                if any(need[k + "weight"] or need[k + "bias"] for k in pk):
                    xn1 = _ln(lib, t, g1, P[pre + "layernorm_before.bias"], _lib.OCM_LN_F32, T, C, eps, torch.float32)
                    if Hp != H:  # the padded rows' input is zero (nothing for the weights), their dq | dk | dv reaches the biases
                        xn1 = _pad_rows(lib, xn1, B, H, Hp)
                    dw, dbq = _weight_grad(prec, dqkv, xn1, True)
                    for i, k in enumerate(pk):
                        if need[k + "weight"]:
                            grads[k + "weight"] = dw[i * C:(i + 1) * C]
                        if need[k + "bias"]:
                            grads[k + "bias"] = dbq[i * C:(i + 1) * C]
                    del xn1
                if Hp != H:  # the padding's gradient: the real positions' rows
                    dqkv = _crop_rows(lib, dqkv, B, H, Hp)
                dxn1 = _linear(lib, prec, _operand(dqkv, prec), W.wt(*[k + "weight" for k in pk]), torch.zeros(C, **f32), None,
                               T, C, _kpad(3 * C, prec))
                del dqkv
                dx, dg, db = _ln_backward(lib, dxn1, t, g1, dx1, T, C, eps)
                lngrads(pre + "layernorm_before.", dg, db)
                del dxn1, dx1
            if stop == 0:  # embeddings: tok = patch rows x W^T + b, t0 = LayerNorm(tok)
                e = "swin.embeddings."
                C, H = c.embed_dim, c.image_size // c.patch_size
                T, Cin = B * H * H, c.num_channels
                pmask = meta.get("patch_mask")
                if pmask is not None:  # the select's backward: masked rows pass nothing down, their sum is the token's gradient
                    mk = e + "mask_token"
                    dtk = torch.empty(C, **f32) if need[mk] else None
                    nbytes = lib.ocm_swin_mask_tokens_backward_workspace_bytes(T, C)
                    wsb = _ws(nbytes, dev)
                    _lib.check(lib.ocm_op_swin_mask_tokens_backward(_p(dx), _p(pmask), _p(dx), _p(dtk), T, C, _p(wsb), nbytes,
                                                                    _stream()))
                    if need[mk]:
                        grads[mk] = dtk
                dtok, dg, db = _ln_backward(lib, dx, keep[0], P[e + "norm.weight"], None, T, C, 1e-5)
                lngrads(e + "norm.", dg, db)
                wk = e + "patch_embeddings.projection."
                if need[wk + "weight"] or need[wk + "bias"]:
                    cols = torch.empty((T, Cin * 16), **f32)
                    _lib.check(lib.ocm_op_patch_unfold(_p(x), _p(cols), B, Cin, c.image_size, c.image_size, c.patch_size,
                                                       _stream()))
                    cols = _pad_cols(cols, -(-Cin * 16 // 32) * 32)
                    dw, dbe = _weight_grad(prec, dtok, cols, True)
                    if need[wk + "weight"]:
                        grads[wk + "weight"] = dw[:, :Cin * 16]
                    if need[wk + "bias"]:
                        grads[wk + "bias"] = dbe
        out = []
        for k in keys:
            g = grads.get(k)
            p = P[k]
            out.append(None if g is None else g.contiguous().reshape(p.shape).to(dtype=p.dtype))
        return (None, None, *out)


# ---- SwinForMaskedImageModeling's head: Conv2d(C_last, s^2 * channels, 1) on the token rows, PixelShuffle(s), masked L1 ----
def _mim_head_forward(model, P, seq, x, mask, want_dlin):
    """seq (B, L, C) fp32 -> (dlin, reconstruction, loss): one GEMM over the token rows in the module's precision (the weight
    operand cached in the module's SourceCache, _Weights), then ocm_op_mim_l1_loss reading the GEMM's rows once — or, without
    a mask (uint8 (B, L_0), _patch_mask), ocm_op_pixel_shuffle alone and no loss. dlin (the loss gradient in the GEMM's row
    layout) only where asked for."""
    c = model.config
    lib, dev = _lib.load(), seq.device
    prec = _lib.PRECISIONS[model._precision]
    B, L, C = seq.shape
    hp = int(L ** 0.5)
    s, ch = c.encoder_stride, c.num_channels
    O = s * s * ch
    f32 = dict(device=dev, dtype=torch.float32)
    lin = _linear(lib, prec, _operand(seq.detach().reshape(B * L, C), prec), _Weights(model, P, prec).w("decoder.0.weight"),
                  P["decoder.0.bias"].detach().float().contiguous(), None, B * L, O, _kpad(C, prec))
    rec = torch.empty((B, ch, hp * s, hp * s), **f32)
    if mask is None:
        _lib.check(lib.ocm_op_pixel_shuffle(_p(lin), _p(rec), B, hp, hp, ch, s, _stream()))
        return None, rec, None
    loss = torch.empty((), **f32)
    dlin = torch.empty_like(lin) if want_dlin else None
    nbytes = lib.ocm_mim_l1_loss_workspace_bytes(B, hp, hp, ch, s)
    wsb = _ws(nbytes, dev)
    _lib.check(lib.ocm_op_mim_l1_loss(_p(lin), _p(x), _p(mask), B, hp, hp, ch, s, c.patch_size, _p(rec), _p(dlin), _p(loss),
                                      _p(wsb), nbytes, _stream()))
    return dlin, rec, loss


class _MimHead(torch.autograd.Function):
    """SwinForMaskedImageModeling's decoder and loss in training mode: forward(meta, seq, weight, bias, x, mask) -> (loss,
    reconstruction) as _mim_head_forward computes them (without a mask the loss is a zero that carries no graph). Kept: seq
    and dlin = d loss / d lin, which ocm_op_mim_l1_loss wrote in the forward (every element +scale, -scale or 0). backward:
    d_lin = d_loss * dlin with the device scalar (no host read), plus ocm_op_pixel_shuffle_backward(d_reconstruction) when that
    gradient arrives; the weight and bias gradients from _weight_grad, d_seq from the transposed-weight GEMM only when the trunk
    carries a graph."""

    @staticmethod
    def forward(ctx, meta, seq, weight, bias, x, mask):
        model = meta["model"]
        ctx.set_materialize_grads(False)
        dlin, rec, loss = _mim_head_forward(model, {"decoder.0.weight": weight, "decoder.0.bias": bias}, seq, x, mask, True)
        ctx.meta, ctx.prec, ctx.bias = meta, _lib.PRECISIONS[model._precision], bias
        ctx.save_for_backward(seq, weight, dlin)
        if loss is None:
            loss = torch.zeros((), dtype=torch.float32, device=seq.device)
            ctx.mark_non_differentiable(loss)
        return loss, rec

    @staticmethod
    def backward(ctx, dloss, drec):
        model, prec = ctx.meta["model"], ctx.prec
        seq, weight, dlin = ctx.saved_tensors
        _, need_x, need_w, need_b = ctx.needs_input_grad[:4]
        c = model.config
        lib, dev = _lib.load(), seq.device
        B, L, C = seq.shape
        hp, s, M = int(L ** 0.5), c.encoder_stride, B * L
        O = weight.shape[0]
        dx = dw = db = None
        with torch.cuda.device(dev):
            d = None
            if dloss is not None and dlin is not None:
                d = dlin * dloss.to(torch.float32)
            if drec is not None:
                g = drec.detach().to(torch.float32).contiguous()
                dsh = torch.empty((M, O), dtype=torch.float32, device=dev)
                _lib.check(lib.ocm_op_pixel_shuffle_backward(_p(g), _p(dsh), B, hp, hp, c.num_channels, s, _stream()))
                d = dsh if d is None else d + dsh
            if d is None:
                return None, None, None, None, None, None
            if need_w or need_b:
                dw, db = _weight_grad(prec, d, seq.reshape(M, C), need_b)
            if need_x:
                P = {"decoder.0.weight": weight}
                dx = _linear(lib, prec, _operand(d, prec), _Weights(model, P, prec).wt("decoder.0.weight"),
                             torch.zeros(C, dtype=torch.float32, device=dev), None, M, C, _kpad(O, prec)).view(B, L, C)
        return (None, dx, dw.reshape(weight.shape).to(weight.dtype) if need_w else None,
                db.reshape(ctx.bias.shape).to(ctx.bias.dtype) if need_b else None, None, None)
