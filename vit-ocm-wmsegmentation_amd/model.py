"""Mirror of the reference's model.py wrappers around the ViT trunk:

  VisionTransformerForSimMIM    model.py:10-53    patch embed -> mask-token blend -> trunk -> (B,C,H,W)
  MIM                           model.py:55-83    encoder + Conv2d(1x1) + PixelShuffle decoder, masked L1 loss
  VisionTransformerForFinetune  model.py:110-139  trunk -> (B,C,H,W)
  LinearProbing                 model.py:142-174  encoder + one-layer (1x1 conv + PixelShuffle) decoder
  build_model / build_finetune_model / get_state_dict   model.py:85-108,176-226
  build_unet (convolution_block, encoder_block, decoder_block)   model.py:227-320  U-Net inference on the direct 3x3 convolution;
                                                                 training (opt-in, enable_training) through _UNetTrain

Same constructor arguments, attributes and state_dict keys. The encoders run in one engine call (the mask
blend is fused into the patch-embedding epilogue, the (B,C,H,W) permute is a device transpose); the 1x1-conv
decoders run token-major as one MFMA GEMM + a pixel-shuffle kernel: one head (_head_forward, differentiable as
_PixelShuffleHead) serves MIM and LinearProbing(layer_num=1) in eval and in training mode. The SimMIM encoder and MIM train:
in training mode with grad mode on and a parameter that requires grad, the encoder runs as the stand-alone operators under
one autograd Function (_EncoderTrain) whose backward is HIP (kernels_train.hip, kernels_train_attn.hip). LinearProbing
also trains: in training mode with a frozen encoder (no encoder parameter requires grad: finetune.py's linear
probing) its decoder differentiates through HIP kernels (_PixelShuffleHead; the two-layer decoder, with batch statistics,
_DecoderTrain). With a trainable VisionTransformerForFinetune that has opted in (enable_finetune(): build_finetune_model
does) the same decoders also return the gradient of the patch tokens and the encoder differentiates through _EncoderTrain
without a mask: finetune.py --finetune True. Every cached operand copy of a decoder weight is keyed on the tensors it is made
from (_cached_operand); biases are read on every call. The reference initialises mask_token with timm's trunc_normal_; here
the package's own trunc_normal_ (dino/utils.py) with the same bounds is used.
"""
import collections
import contextlib
import ctypes as C
import operator
import os
from functools import lru_cache, partial

import torch
import torch.nn as nn

from . import _lib
from .dino.utils import trunc_normal_
from .dino import vision_transformer as _vt
from .dino.vision_transformer import VisionTransformer
from .engine import OPERAND_DTYPE as _OPERAND_DTYPE, SourceCache, _p, _require_hip, _stream, _ws, to_operand


class _FmapEncoder(VisionTransformer):
    """Shared body of the two encoders: prepare tokens (optionally masked), all blocks, final norm, drop the
    CLS token and return the (B, C, H, W) map."""

    def _positions(self, npatch, device):
        """The (N, D) position table of a forward over npatch patches: interpolated for the CONFIGURED size (model.py:38-39,
        124-125); at 224 the reference adds pos_embed itself (model.py:40-41,126-127), which needs the native token count."""
        side = self.img_size[0]
        if side == 224 and npatch != self.pos_embed.shape[1] - 1:
            raise RuntimeError(f"The size of tensor a ({npatch + 1}) must match the size of tensor b "
                               f"({self.pos_embed.shape[1]}) at non-singleton dimension 1")
        return self._pos_for(npatch, side, side, device)

    def _encode(self, x, mask=None, tokens=False):
        x = self._check_input(x)
        eng = self._engine(x.device)
        pos = self._positions((x.shape[-2] // eng.p) * (x.shape[-1] // eng.p), x.device)
        flags = _lib.OCM_OUT_FEAT if tokens else _lib.OCM_OUT_FMAP
        out = eng.forward(x, pos, flags=flags, patch_mask=mask)
        if tokens:
            return out["feat"][0]
        fmap = out["fmap"]
        B, Cc, hp, wp = fmap.shape
        side_t = int((hp * wp) ** 0.5)  # model.py:50-52: H = W = int(L ** 0.5)
        return fmap.reshape(B, Cc, side_t, side_t)


class VisionTransformerForSimMIM(_FmapEncoder):
    def __init__(self, interpolate_encoding=False, img_size=224, **kwargs):
        super().__init__(**kwargs)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, self.embed_dim))
        self.img_size = img_size
        self._trunc_normal_(self.mask_token, std=.02)
        self.interpolate_encoding = interpolate_encoding

    def _trunc_normal_(self, tensor, mean=0., std=1.):
        trunc_normal_(tensor, mean=mean, std=std, a=-std, b=std)

    def forward(self, x, mask):
        assert mask is not None
        if _differentiable(self):
            _check_trainable(self, x, mask=mask)
            return _tokens_to_fmap(_encode_train(self, x, mask.to(x.device)))
        return self._encode(x, mask=mask.to(x.device))


class VisionTransformerForFinetune(_FmapEncoder):
    def __init__(self, interpolate_encoding=False, img_size=224, **kwargs):
        super().__init__(**kwargs)
        self.img_size = img_size
        self.interpolate_encoding = interpolate_encoding
        self.finetune_backward = False  # a plain attribute: not a parameter, not a buffer, not in the state_dict

    def _trunc_normal_(self, tensor, mean=0., std=1.):
        trunc_normal_(tensor, mean=mean, std=std, a=-std, b=std)

    def enable_finetune(self, flag=True):
        """Opt this encoder in to (or out of) the HIP backward: in training mode with grad mode on and a trainable parameter,
        forward() and LinearProbing.forward() then build a graph into the encoder's parameters (finetune.py --finetune True).
        build_finetune_model() turns it on; a directly constructed encoder keeps the graph-free behaviour."""
        self.finetune_backward = bool(flag)
        return self

    def forward(self, x):
        if _finetunes(self):
            _check_trainable(self, x, masked=False)
            return _tokens_to_fmap(_encode_train(self, x, None))
        return self._encode(x)


def _tokens_to_fmap(tokens):
    """Normed tokens (B, N, D) -> the (B, D, side, side) map of the patch rows (model.py:50-52,136-138: H = W = int(L ** 0.5))."""
    B, N, D = tokens.shape
    side = int((N - 1) ** 0.5)
    return tokens[:, 1:].transpose(1, 2).reshape(B, D, side, side)


def _pixel_shuffle_head(channels, stride, out_mult):
    """Conv2d(channels, stride^2 * out_mult, 1) -> PixelShuffle(stride): the decoder head of model.py:60-66,147-152.
    Kept as torch modules for their parameters / state_dict keys; the arithmetic runs in _head_forward."""
    return nn.Sequential(nn.Conv2d(channels, stride * stride * out_mult, kernel_size=1), nn.PixelShuffle(stride))


def _prefixed(encoder, method):
    fn = getattr(encoder, method, None)
    return {"encoder." + name for name in fn()} if fn is not None else {}


class MIM(nn.Module):
    """model.py:55-83: masked-image-modelling wrapper, forward(x, mask) -> (loss, x_rec, mask)."""

    def __init__(self, encoder, encoder_stride):
        super().__init__()
        self.encoder, self.encoder_stride = encoder, encoder_stride
        self.decoder = _pixel_shuffle_head(encoder.num_features, encoder_stride, 3)
        self.in_chans, self.patch_size = 3, 8
        self.__dict__["_dec_cache"] = SourceCache()

    def forward(self, x, mask):
        if _differentiable(self):  # training mode, grad mode on, something to train: the HIP backward (_EncoderTrain)
            return self._forward(x, mask, train=True)
        with torch.no_grad():
            return self._forward(x, mask, train=False)

    def _forward(self, x, mask, train):
        enc = self.encoder
        if train:
            _check_trainable(enc, x, encoder=_differentiable(enc), mask=mask)
        _require_hip(x, "input")
        mask = mask.to(x.device)
        if train and _differentiable(enc):
            tokens = _encode_train(enc, x, mask)
        else:
            with torch.no_grad():
                tokens = enc._encode(x, mask=mask, tokens=True)
        conv = self.decoder[0]
        head = _PixelShuffleHead.apply if train else _head_forward
        x_rec = head(_head_meta(self), tokens[:, 1:].contiguous(), conv.weight, conv.bias)
        # masked L1 reconstruction loss (model.py:71-73) — training bookkeeping, a handful of elementwise torch ops
        p = self.patch_size
        m32 = mask.to(torch.float32).contiguous()
        pixel_mask = torch.empty((m32.shape[0], m32.shape[1] * p, m32.shape[2] * p), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().ocm_op_nearest_upsample(_p(m32), _p(pixel_mask), m32.shape[0], m32.shape[1], m32.shape[2], p,
                                                           _stream()))
        pixel_mask = pixel_mask.to(mask.dtype).unsqueeze(1)  # 0 / 1 values: exact in the caller's dtype
        err = (x - x_rec).abs() * pixel_mask
        loss = err.sum() / (pixel_mask.sum() + 1e-5) / self.in_chans
        return loss, x_rec, pixel_mask

    @torch.jit.ignore
    def no_weight_decay(self):
        return _prefixed(self.encoder, "no_weight_decay")

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return _prefixed(self.encoder, "no_weight_decay_keywords")


class LinearProbing(nn.Module):
    """model.py:142-174: encoder + segmentation decoder (layer_num 1: 1x1 conv + PixelShuffle; 2: two 3x3 convs)."""

    def __init__(self, encoder, encoder_stride, layer_num=1):
        super().__init__()
        self.encoder, self.layer_num, self.encoder_stride = encoder, layer_num, encoder_stride
        feats, s2 = encoder.num_features, encoder_stride ** 2
        self.one_layer_decoder = _pixel_shuffle_head(feats, encoder_stride, 1)
        self.two_layer_decoder = nn.Sequential(
            nn.Conv2d(feats, 4 * s2, kernel_size=3, padding=1), nn.BatchNorm2d(4 * s2), nn.ReLU(inplace=True),
            nn.Conv2d(4 * s2, s2, kernel_size=3, padding=1), nn.PixelShuffle(encoder_stride))
        self.__dict__["_dec_cache"] = SourceCache()

    def _two_layer(self, tokens):
        """two_layer_decoder (model.py:154-166) in eval mode on the HIP path, token-major: im2col(3x3) + MFMA GEMM with
        the BatchNorm (running statistics) folded into the first convolution's weights, ReLU applied while gathering the
        second convolution's operand, PixelShuffle by the scatter kernel."""
        conv1, bn, _, conv2, _ = self.two_layer_decoder
        if bn.training:
            raise NotImplementedError("training mode runs on the HIP path only with a frozen encoder (linear probing: set "
                                      "requires_grad=False on every encoder parameter) or with an encoder that has opted "
                                      "in to fine-tuning (encoder.enable_finetune(); build_finetune_model does). For "
                                      "inference call .eval()")
        dev, cache = tokens.device, self._dec_cache
        prec = _lib.PRECISIONS[self.encoder._precision]
        B, N, D = tokens.shape
        hp = wp = int((N - 1) ** 0.5)
        mid, out_c = conv1.out_channels, conv2.out_channels
        f32 = dict(device=dev, dtype=torch.float32)

        def gain():  # the BatchNorm scale per channel, from the running statistics
            return bn.weight.detach().to(**f32) / torch.sqrt(bn.running_var.detach().to(**f32) + bn.eps)

        w1 = _cached_operand(cache, "conv1.folded", (conv1.weight, bn.weight, bn.running_var), prec, lambda: to_operand(
            _rows3x3(conv1.weight.detach().to(**f32) * gain()[:, None, None, None]).contiguous(), prec))
        b1 = _cached_operand(cache, "conv1.folded_bias", (conv1.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var), prec,
                             lambda: ((conv1.bias.detach().to(**f32) - bn.running_mean.detach().to(**f32)) * gain()
                                      + bn.bias.detach().to(**f32)).contiguous())
        w2 = _weight_operand(cache, "conv2", conv2.weight, prec, dev, _rows3x3)
        patches = tokens[:, 1:].contiguous()  # (B, hp*wp, D) fp32
        with torch.cuda.device(dev):
            y1 = _conv3x3(prec, patches, w1, b1, (B, hp, wp), D, mid)
            y2 = _conv3x3(prec, y1, w2, _vec(conv2.bias, out_c, dev), (B, hp, wp), mid, out_c, relu=True)  # ReLU on the way
            return _pixel_shuffle(y2, B, hp, wp, self.encoder_stride)

    def _encoder_frozen(self):
        return not any(p.requires_grad for p in self.encoder.parameters())

    def forward(self, x):
        enc = self.encoder
        finetune = self.training and _finetunes(enc)  # finetune.py --finetune True: the encoder trains too
        if finetune:
            _check_trainable(enc, x, masked=False)
        _require_hip(x, "input")
        if finetune:
            tokens = _encode_train(enc, x, None)
        else:
            with torch.no_grad():
                tokens = enc._encode(x, tokens=True)
        # the training decoder: a frozen encoder (linear probing), or one that has opted in to fine-tuning — differentiated
        # above, or not right now (no_grad, or its own eval mode). Any other encoder keeps the eval decoder.
        if self.training and (self._encoder_frozen() or getattr(enc, "finetune_backward", False)):
            return _train_forward(self, tokens)
        with torch.no_grad():
            if self.layer_num == 2:
                return self._two_layer(tokens)
            conv = self.one_layer_decoder[0]
            return _head_forward(_head_meta(self), tokens[:, 1:].contiguous(), conv.weight, conv.bias)


# ---- the decoders' pieces. Token-major rows m = (image, y, x), M = B*hp*wp; s = stride, mid = 4 s^2. Training (finetune.py,
# mim.py) runs the forward with batch statistics and the backward through kernels_train.hip. ----
def _rows1x1(w):
    """(O, C, 1, 1) kernel -> the (O, C) weight of ocm_op_linear over the token rows."""
    return w.reshape(w.shape[0], -1)


def _rows1x1_t(w):
    """(O, C, 1, 1) kernel -> (C, O): the data gradient dX = dY W runs as ocm_op_linear(dY, W^T)."""
    return _rows1x1(w).t()


def _rows3x3(w):
    """(O, C, 3, 3) kernel -> (O, 9*C) with K = (ky*3 + kx)*C + c: the K order of ocm_op_im2col3x3."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def flip_conv3x3(w):
    """(O, C, 3, 3) kernel -> (C, 9*O) weight of the data gradient as a token-major 3x3 convolution: row c, column
    (ky*3 + kx)*O + o holds w[o][c][2-ky][2-kx]. im2col3x3(dY) @ flip_conv3x3(w)^T equals conv2d_input(dY, w) with padding
    1 (the transposed convolution is the convolution with the flipped, channel-transposed kernel)."""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1)


def _put(t, like):
    """A gradient in the parameter's own shape, on its device and in its dtype."""
    return None if t is None else t.reshape(like.shape).to(device=like.device, dtype=like.dtype)


def _weight_grad(prec, dy, x, want_bias):
    """dW = dy^T x (and db = column sums of dy) on the weight-gradient kernel; dy (M, N), x (M, K) fp32."""
    lib, (M, N), K = _lib.load(), dy.shape, x.shape[1]
    dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    db = torch.empty((N,), dtype=torch.float32, device=dy.device) if want_bias else None
    nbytes = lib.ocm_weight_grad_workspace_bytes(M, N, K)
    ws = _ws(nbytes, dy.device)
    _lib.check(lib.ocm_op_weight_grad(prec, _p(dy), _p(x), _p(dw), _p(db), M, N, K, _p(ws), nbytes, _stream()))
    return dw, db


def _pixel_shuffle(lin, B, hp, wp, s):
    """PixelShuffle(s) of the token-major rows lin (B*hp*wp, c*s*s) -> (B, c, hp*s, wp*s) fp32."""
    c_out = lin.shape[1] // (s * s)
    out = torch.empty((B, c_out, hp * s, wp * s), dtype=torch.float32, device=lin.device)
    _lib.check(_lib.load().ocm_op_pixel_shuffle(_p(lin), _p(out), B, hp, wp, c_out, s, _stream()))
    return out


def _pixel_shuffle_backward(g, M, s, hp, wp):
    g = g.detach().to(torch.float32).contiguous()
    B, c_out = g.shape[0], g.shape[1]
    lin = torch.empty((M, c_out * s * s), dtype=torch.float32, device=g.device)
    _lib.check(_lib.load().ocm_op_pixel_shuffle_backward(_p(g), _p(lin), B, hp, wp, c_out, s, _stream()))
    return lin


def _cached_operand(cache, name, srcs, prec, make):
    """What make() builds from `srcs` (a parameter, or a tuple of parameters and buffers) in `prec`: engine.SourceCache."""
    return cache.get(name, srcs if isinstance(srcs, tuple) else (srcs,), make, prec)


def _weight_operand(cache, name, w, prec, dev, layout):
    """Operand copy of a convolution kernel in one of the layouts above, cached under the kernel's own key."""
    return _cached_operand(cache, f"{name}.{layout.__name__}", w, prec, lambda: to_operand(
        layout(w.detach().to(device=dev, dtype=torch.float32)).contiguous(), prec))


def _zeros(cache, n, dev):
    """The all-zero fp32 bias of a GEMM that adds none: one vector per length."""
    return cache.get(("zeros", n), (), lambda: torch.zeros(n, device=dev, dtype=torch.float32), dev)


def _im2col3x3(prec, x, grid, C, relu=False, affine=None):
    """The (M, 9*C) rows of a 3x3 pad-1 convolution over x (M, C) fp32, in the operand type of `prec`: gathered as they are,
    through a ReLU, or through the per-channel affine (g, h) of a BatchNorm and a ReLU."""
    lib, (B, hp, wp) = _lib.load(), grid
    a = torch.empty((B * hp * wp, 9 * C), dtype=_OPERAND_DTYPE[prec], device=x.device)
    if affine is not None:
        _lib.check(lib.ocm_op_bn_relu_im2col3x3(prec, _p(x), _p(affine[0]), _p(affine[1]), _p(a), B, hp, wp, C, _stream()))
    else:
        _lib.check(lib.ocm_op_im2col3x3(prec, _p(x), _p(a), B, hp, wp, C, int(relu), _stream()))
    return a


def _conv3x3(prec, x, w_op, bias, grid, C, O, **gather):
    """One 3x3 pad-1 convolution on the token-major rows: _im2col3x3, then ocm_op_linear on the (O, 9*C) operand -> (M, O)."""
    B, hp, wp = grid
    return _linear(_lib.load(), prec, _im2col3x3(prec, x, grid, C, **gather), w_op, bias, None, B * hp * wp, O, 9 * C)


def _head_meta(module):
    """What the pixel-shuffle head needs of its wrapper (MIM, LinearProbing): precision, stride and the operand cache."""
    return {"prec": _lib.PRECISIONS[module.encoder._precision], "stride": module.encoder_stride, "cache": module._dec_cache}


def _head_forward(meta, patches, weight, bias):
    """Conv2d(D, s*s*c, 1) + PixelShuffle(s) on the normed patch rows (B, P, D) fp32 (the caller has dropped the CLS row): one
    GEMM over the rows and a scatter. Returns (B, c, hp*s, wp*s) fp32."""
    prec, dev = meta["prec"], patches.device
    B, P, D = patches.shape
    hp = wp = int(P ** 0.5)
    M, O = B * P, weight.shape[0]
    w = _weight_operand(meta["cache"], "head", weight, prec, dev, _rows1x1)
    with torch.cuda.device(dev):
        lin = _linear(_lib.load(), prec, to_operand(patches.reshape(M, D), prec), w, _vec(bias, O, dev), None, M, O, D)
        return _pixel_shuffle(lin, B, hp, wp, meta["stride"])


class _PixelShuffleHead(torch.autograd.Function):
    """The head of MIM and of LinearProbing(layer_num=1) in training mode: forward(meta, patches, weight, bias) as _head_forward
    computes it; backward -> the weight / bias gradients and, when the patch rows carry a graph (a trainable encoder), dPatches
    (B, P, D) fp32 = dlin W. Patch rows from a frozen encoder get none and cost nothing. The callers slice the CLS row off the
    tokens themselves, so autograd gives it its zero gradient."""

    @staticmethod
    def forward(ctx, meta, patches, weight, bias):
        ctx.meta, ctx.bias = meta, bias
        ctx.save_for_backward(patches, weight)
        return _head_forward(meta, patches, weight, bias)

    @staticmethod
    def backward(ctx, grad_out):
        meta, (patches, weight) = ctx.meta, ctx.saved_tensors
        prec, s, cache, dev = meta["prec"], meta["stride"], meta["cache"], grad_out.device
        B, P, D = patches.shape
        hp = wp = int(P ** 0.5)
        M, O = B * P, weight.shape[0]
        _, need_x, need_w, need_b = ctx.needs_input_grad
        dx = dw = db = None
        with torch.cuda.device(dev):
            dlin = _pixel_shuffle_backward(grad_out, M, s, hp, wp)  # (M, O)
            if need_w or need_b:
                dw, db = _weight_grad(prec, dlin, patches.reshape(M, D), need_b)
            if need_x:
                wt = _weight_operand(cache, "head", weight, prec, dev, _rows1x1_t)
                dx = _linear(_lib.load(), prec, to_operand(dlin, prec), wt, _zeros(cache, D, dev), None, M, D, O)
                dx = dx.reshape(B, P, D)
        return None, dx, _put(dw, weight) if need_w else None, _put(db, ctx.bias) if need_b else None


class _DecoderTrain(torch.autograd.Function):
    """One training-mode call of the two-layer decoder: forward(patches, *params) -> (B, 1, hp*s, wp*s); backward -> parameter
    gradients and, when the patch tokens carry a graph (a trainable encoder), dPatches (B, P, D) fp32: conv1's data gradient
    (the 3x3 pad-1 convolution of dy1 with the flipped, channel-transposed kernel). Patch tokens from a frozen encoder get
    none and cost nothing. `meta` carries the module, its precision and, for the caller, the batch statistics of the forward
    (the running-statistics update happens outside the graph)."""

    @staticmethod
    def forward(ctx, meta, patches, *params):
        lp, prec, dev = meta["module"], meta["prec"], patches.device
        lib, s, cache = _lib.load(), lp.encoder_stride, lp._dec_cache
        conv1, bn, _, conv2, _ = lp.two_layer_decoder
        B, P, D = patches.shape
        hp = wp = int(P ** 0.5)
        M, mid, oc = B * P, conv1.out_channels, conv2.out_channels
        f32 = dict(device=dev, dtype=torch.float32)
        ctx.meta, ctx.shape = meta, (B, hp, wp, D, M)
        y1 = _conv3x3(prec, patches, _weight_operand(cache, "conv1", conv1.weight, prec, dev, _rows3x3),
                      _vec(conv1.bias, mid, dev), (B, hp, wp), D, mid)
        mean, var = torch.empty(mid, **f32), torch.empty(mid, **f32)
        nbytes = lib.ocm_channel_reduce_workspace_bytes(M, mid)
        ws = _ws(nbytes, dev)
        _lib.check(lib.ocm_op_batch_stats(_p(y1), _p(mean), _p(var), M, mid, _p(ws), nbytes, _stream()))
        # per-channel affine of the normalisation (mid-length vectors): z = relu(y1 * g + h)
        invstd = torch.rsqrt(var + bn.eps)
        gamma = bn.weight.detach().to(**f32) if bn.weight is not None else torch.ones(mid, **f32)
        g = (gamma * invstd).contiguous()
        h = (_vec(bn.bias, mid, dev) - mean * g).contiguous()
        y2 = _conv3x3(prec, y1, _weight_operand(cache, "conv2", conv2.weight, prec, dev, _rows3x3),
                      _vec(conv2.bias, oc, dev), (B, hp, wp), mid, oc, affine=(g, h))
        meta["mean"], meta["var"] = mean, var
        ctx.save_for_backward(patches, y1, mean, invstd, g, h)
        return _pixel_shuffle(y2, B, hp, wp, s)

    @staticmethod
    def backward(ctx, grad_out):
        meta = ctx.meta
        lp, prec = meta["module"], meta["prec"]
        B, hp, wp, D, M = ctx.shape
        s, lib, cache = lp.encoder_stride, _lib.load(), lp._dec_cache
        need, need_x = ctx.needs_input_grad[2:], ctx.needs_input_grad[1]
        dev, grid = grad_out.device, (B, hp, wp)
        f32 = dict(device=dev, dtype=torch.float32)
        patches, y1, mean, invstd, g, h = ctx.saved_tensors
        conv1, bn, _, conv2, _ = lp.two_layer_decoder
        mid, oc = conv1.out_channels, conv2.out_channels
        dpatches, grads = None, [None] * 6
        with torch.cuda.device(dev):
            dy2 = _pixel_shuffle_backward(grad_out, M, s, hp, wp)  # (M, oc)
            if need[4] or need[5]:
                a2 = _im2col3x3(_lib.OCM_PREC_FP32, y1, grid, mid, affine=(g, h))  # conv2's operand again, in fp32
                dw2, db2 = _weight_grad(prec, dy2, a2, need[5])
                del a2
                grads[4] = _put(dw2.reshape(oc, 3, 3, mid).permute(0, 3, 1, 2), conv2.weight) if need[4] else None
                grads[5] = _put(db2, conv2.bias) if need[5] else None
            if any(need[:4]) or need_x:
                # conv2's data gradient: a 3x3 pad-1 convolution of dY2 with the flipped, channel-transposed kernel
                dz = _conv3x3(prec, dy2, _weight_operand(cache, "conv2", conv2.weight, prec, dev, flip_conv3x3),
                              _zeros(cache, mid, dev), grid, oc, mid)
                dy1, dgam, dbet = torch.empty((M, mid), **f32), torch.empty(mid, **f32), torch.empty(mid, **f32)
                nbytes = lib.ocm_channel_reduce_workspace_bytes(M, mid)
                ws = _ws(nbytes, dev)
                _lib.check(lib.ocm_op_bn_relu_backward(_p(dz), _p(y1), _p(mean), _p(invstd), _p(g), _p(h), _p(dy1), _p(dgam),
                                                       _p(dbet), M, mid, _p(ws), nbytes, _stream()))
                del dz
                grads[2] = _put(dgam, bn.weight) if need[2] else None
                grads[3] = _put(dbet, bn.bias) if need[3] else None
                if need[0] or need[1]:
                    a1 = _im2col3x3(_lib.OCM_PREC_FP32, patches, grid, D)  # im2col of the patch tokens again, in fp32
                    dw1, db1 = _weight_grad(prec, dy1, a1, need[1])
                    del a1
                    grads[0] = _put(dw1.reshape(mid, 3, 3, D).permute(0, 3, 1, 2), conv1.weight) if need[0] else None
                    grads[1] = _put(db1, conv1.bias) if need[1] else None
                if need_x:  # conv1's data gradient, by the same construction (K = 9 mid, N = D)
                    dpatches = _conv3x3(prec, dy1, _weight_operand(cache, "conv1", conv1.weight, prec, dev, flip_conv3x3),
                                        _zeros(cache, D, dev), grid, mid, D).reshape(B, hp * wp, D)
        return (None, dpatches, *grads)


def _train_forward(lp, tokens):
    """LinearProbing.forward in training mode: the decoder (layer_num 2: with batch statistics, the running statistics updated as
    nn.BatchNorm2d updates them) and a graph into its parameters when grad mode is on. The normed tokens (B, N, D) come from a
    frozen encoder without a graph, or carry one (a trainable encoder, or a leaf that requires grad): then the decoder's patch
    gradient goes back into rows 1..N-1 and the CLS row, which no decoder reads, gets zeros."""
    B, N, D = tokens.shape
    patches = tokens[:, 1:].contiguous()
    if lp.layer_num != 2:
        conv = lp.one_layer_decoder[0]
        return _PixelShuffleHead.apply(_head_meta(lp), patches, conv.weight, conv.bias)
    conv1, bn, _, conv2, _ = lp.two_layer_decoder
    if not bn.training:
        raise NotImplementedError("the training-mode decoder normalises with batch statistics: BatchNorm2d in eval "
                                  "mode inside a training LinearProbing is not supported on the HIP path")
    if B * (N - 1) < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size "
                         f"{[B, conv1.out_channels, 1, 1]}")
    meta = {"module": lp, "prec": _lib.PRECISIONS[lp.encoder._precision]}
    with torch.cuda.device(tokens.device):
        out = _DecoderTrain.apply(meta, patches, conv1.weight, conv1.bias, bn.weight, bn.bias, conv2.weight, conv2.bias)
        if bn.track_running_stats and bn.running_mean is not None:
            _update_running_stats(bn, meta["mean"], meta["var"], B * (N - 1))
    return out


@torch.no_grad()
def _update_running_stats(bn, mean, var, n):
    """nn.BatchNorm2d's update in training mode, in place on the buffers themselves (their _version moves, so the eval
    path's cache of the folded weights sees it): momentum, or the cumulative average when momentum is None; the
    unbiased variance goes into running_var."""
    bn.num_batches_tracked.add_(1)
    f = (1.0 / float(bn.num_batches_tracked)) if bn.momentum is None else bn.momentum
    rm, rv = bn.running_mean, bn.running_var
    unbiased = var * (n / (n - 1))
    rm.mul_(1.0 - f).add_(mean.to(device=rm.device, dtype=rm.dtype), alpha=f)
    rv.mul_(1.0 - f).add_(unbiased.to(device=rv.device, dtype=rv.dtype), alpha=f)


# ---- SimMIM pre-training (mim.py): the encoder forward as the stand-alone operators, keeping what the backward needs, and the
# backward through kernels_train.hip / kernels_train_attn.hip. Token-major rows m = b*N + n, T = B*N. ----
_LN_KIND = {_lib.OCM_PREC_BF16: _lib.OCM_LN_BF16, _lib.OCM_PREC_FP32: _lib.OCM_LN_F32, _lib.OCM_PREC_BF16X3: _lib.OCM_LN_SPLIT}


def _differentiable(module):
    """The training path runs when the module is in training mode, grad mode is on and a parameter requires grad."""
    return module.training and torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters())


def _finetunes(enc):
    """A VisionTransformerForFinetune that has opted in (enable_finetune) and has something to train right now."""
    return getattr(enc, "finetune_backward", False) and _differentiable(enc)


def _check_mask(enc, x, mask):
    """The SimMIM mask must hold one entry per patch of every image (the kernels read B * P of them), as the eval path's
    Engine.forward_tiles requires."""
    p = enc.patch_embed.patch_size
    B, npatch = x.shape[0], (x.shape[-2] // p) * (x.shape[-1] // p)
    if mask is None or mask.numel() != B * npatch:
        got = "no mask" if mask is None else f"mask has {mask.numel() / max(B, 1):g} entries per image"
        raise ValueError(f"{got}, expected {npatch}")


def _check_trainable(enc, x, encoder=True, mask=None, masked=True):
    """What the training path refuses, before anything is launched (`encoder`: the encoder itself is to be differentiated;
    `masked`: it blends a mask token in, VisionTransformerForSimMIM, and needs one mask entry per patch)."""
    hd = enc.embed_dim // enc._hyper["num_heads"]
    if encoder and hd not in (64, 128):
        raise NotImplementedError(f"training the encoder needs 64- or 128-wide heads (the attention backward is built for "
                                  f"those); this one has {hd}-wide heads")
    if isinstance(x, torch.Tensor) and x.requires_grad:
        raise NotImplementedError("the training path does not produce the gradient of the input image; pass an input that "
                                  "does not require grad")
    if encoder and enc._gray_fold:
        raise NotImplementedError("the grayscale-folded patch embedding is inference only; disable it for training")
    if encoder and masked:
        _check_mask(enc, x, mask)


def _encoder_params(enc):
    """(name, parameter) of everything the encoder's training path differentiates, in a fixed order."""
    names = ["cls_token", "pos_embed", "mask_token", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    for i in range(len(enc.blocks)):
        names += [f"blocks.{i}.{m}.{t}" for m in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2")
                  for t in ("weight", "bias")]
    names += ["norm.weight", "norm.bias"]
    out = []
    for n in names:
        prefix, _, key = n.rpartition(".")
        mod = enc.get_submodule(prefix) if prefix else enc
        p = mod._parameters.get(key)
        if p is not None:
            out.append((n, p))
    return out


def _first_block_to_train(enc, named):
    """The lowest block with a trainable parameter (len(blocks) when none has one) when nothing below the blocks trains — the
    patch embedding, cls_token, pos_embed and a mask_token are all frozen — else 0. Below it the forward keeps nothing and the
    backward does not go: the remaining gradients come from the same operators in the same order, so they keep their bits."""
    if any(p.requires_grad for n, p in named if not n.startswith(("blocks.", "norm."))):
        return 0
    trainable = [int(n.split(".")[1]) for n, p in named if n.startswith("blocks.") and p.requires_grad]
    return min(trainable) if trainable else len(enc.blocks)


def _encode_train(enc, x, mask, own_size=False):
    """Differentiable token path of VisionTransformerForSimMIM (with its mask), of VisionTransformerForFinetune (mask None: no
    blend) and, with own_size, of a plain VisionTransformer that has opted in (enable_training): (B, N, D) normed tokens with a
    graph into the encoder's parameters. The position table is the one of the configured size for the two map encoders
    (_FmapEncoder._positions) and the one of the input's own (w, h) with own_size, as prepare_tokens takes it at every call."""
    x = enc._check_input(x).contiguous()
    if mask is not None or "mask_token" in enc._parameters:
        _check_mask(enc, x, mask)
    eng = enc._engine(x.device, training_path=True)
    npatch = (x.shape[-2] // eng.p) * (x.shape[-1] // eng.p)
    named = _encoder_params(enc)
    wh = (x.shape[-2], x.shape[-1]) if own_size else (enc.img_size[0], enc.img_size[0])
    if own_size:  # one cached table per crop size: a step alternates between the global and the local crops' sizes
        pos = enc._pos_cache.get(("pos", wh), (enc.pos_embed,), lambda: enc._interpolated_pos(npatch, *wh)[0].to(
            device=x.device, dtype=torch.float32).contiguous(), (npatch, x.device))
    else:
        pos = enc._positions(npatch, x.device)
    dropout = _dropout_sites(enc, x.device)  # drawn before the drop-path tables: a seeded run is reproducible
    meta = {"enc": enc, "eng": eng, "names": [n for n, _ in named], "pos": pos, "wh": wh, "npatch": npatch, "dropout": dropout,
            "first": _first_block_to_train(enc, named), "scales": _drop_path_scales(enc, x.shape[0], x.device),
            "mask": mask.reshape(x.shape[0], -1).to(torch.float32).contiguous() if mask is not None else None}
    with torch.cuda.device(x.device):
        return _EncoderTrain.apply(meta, x, *[p for _, p in named])


def _drop_path_scales(enc, batch, dev):
    """The per-image DropPath scale tables of one training forward (vision_transformer.draw_drop_path_scales, looked up at call
    time): 2 * depth entries, None or a contiguous fp32 (batch,) tensor on `dev`. One call per _encode_train call, so DINO's
    MultiCropWrapper draws per resolution group, as upstream's does."""
    scales = list(_vt.draw_drop_path_scales(enc, batch, dev))
    if len(scales) != 2 * len(enc.blocks):
        raise ValueError(f"draw_drop_path_scales returned {len(scales)} entries for {len(enc.blocks)} blocks")
    for j, sc in enumerate(scales):
        if sc is not None:
            if sc.numel() != batch:
                raise ValueError(f"drop-path scale table {j} has {sc.numel()} entries for a batch of {batch}")
            scales[j] = sc.detach().to(device=dev, dtype=torch.float32).reshape(batch).contiguous()
    return scales


def _dropout_sites(enc, dev):
    """Dropout of one training forward of an encoder that has opted in (enable_dropout): None when no site has a rate above 0,
    else (seeds, sites): the int64 device tensor of vision_transformer.draw_dropout_seeds (looked up at call time; one draw per
    _encode_train call) and per site None or (thresh, inv_keep) as ocm_dropout_threshold forms them. Site order:
    vision_transformer.dropout_site_rates."""
    if not getattr(enc, "dropout_enabled", False):
        return None
    rates = _vt.dropout_site_rates(enc)
    seeds = _vt.draw_dropout_seeds(enc, dev)
    if seeds is None:
        return None
    if seeds.numel() != len(rates) or seeds.dtype != torch.int64:
        raise ValueError(f"draw_dropout_seeds returned {seeds.numel()} {seeds.dtype} entries for {len(rates)} sites")
    lib, sites = _lib.load(), []
    for r in rates:
        if r > 0:
            th, ik = C.c_uint32(), C.c_float()
            _lib.check(lib.ocm_dropout_threshold(r, C.byref(th), C.byref(ik)))
            sites.append((th.value, ik.value))
        else:
            sites.append(None)
    return seeds.detach().to(device=dev).contiguous(), sites


def _vec(t, n, dev):
    return t.detach().to(device=dev, dtype=torch.float32).contiguous() if t is not None else torch.zeros(n, device=dev)


def _ln(lib, x, w, b, kind, rows, dim, eps, dtype):
    y = torch.empty((rows, dim), dtype=dtype, device=x.device)
    _lib.check(lib.ocm_op_layernorm(_p(x), _p(w), _p(b), _p(y), kind, rows, dim, eps, _stream()))
    return y


def _drop_path_ln(lib, x, branch, scale, w, b, kind, B, N, dim, eps, dtype):
    """(x + branch * scale[image], its LayerNorm in `kind`) from one kernel; the sum is written over `branch`."""
    y = torch.empty((B * N, dim), dtype=dtype, device=x.device)
    _lib.check(lib.ocm_op_drop_path_layernorm(_p(x), _p(branch), _p(scale), _p(w), _p(b), _p(branch), _p(y), kind, B, N, dim, eps,
                                              _stream()))
    return branch, y


def _dropout_ln(lib, x, branch, seeds, site, drop, scale, w, b, kind, B, N, dim, eps, dtype):
    """(x + branch * factor [* scale[image]], its LayerNorm in `kind`) from one kernel; the sum is written over `branch`."""
    y = torch.empty((B * N, dim), dtype=dtype, device=x.device)
    _lib.check(lib.ocm_op_dropout_layernorm(_p(x), _p(branch), _p(seeds), site, drop[0], drop[1], _p(scale), _p(w), _p(b),
                                            _p(branch), _p(y), kind, B, N, dim, eps, _stream()))
    return branch, y


def _dropout_backward(lib, prec, dout, seeds, site, drop, scale, B, N, dim):
    """(dout * factor [* scale[image]] in fp32, the same as the operand of the data-gradient GEMM) from one kernel."""
    d32 = torch.empty_like(dout)
    if prec == _lib.OCM_PREC_FP32 and scale is None:
        # nothing to fuse: no scale, no operand copy. ocm_op_dropout writes the same bits and measured 0.8 us faster than the
        # eight-element kernel at 12 608 x 384, so this one site runs the composition
        _lib.check(lib.ocm_op_dropout(_p(dout), _p(seeds), site, drop[0], drop[1], _p(d32), dout.numel(), _stream()))
        return d32, d32
    if prec == _lib.OCM_PREC_FP32:
        d_op = d32
    else:
        d_op = torch.empty((B * N, dim), dtype=_OPERAND_DTYPE[prec], device=dout.device)
    _lib.check(lib.ocm_op_dropout_backward(prec, _p(dout), _p(seeds), site, drop[0], drop[1], _p(scale), _p(d32),
                                           None if d_op is d32 else _p(d_op), B, N, dim, _stream()))
    return d32, d_op


def _drop_path_backward(lib, prec, dout, scale, B, N, dim):
    """(dout * scale[image] in fp32, the same as the operand of the data-gradient GEMM) from one kernel."""
    d32 = torch.empty_like(dout)
    if prec == _lib.OCM_PREC_FP32:
        d_op = d32
    else:
        d_op = torch.empty((B * N, dim), dtype=_OPERAND_DTYPE[prec], device=dout.device)
    _lib.check(lib.ocm_op_drop_path_backward(prec, _p(dout), _p(scale), _p(d32), None if d_op is d32 else _p(d_op), B, N, dim,
                                             _stream()))
    return d32, d_op


def _ln_backward(lib, dy, x, w, dres, rows, dim, eps):
    """(dx, dgamma, dbeta) of a LayerNorm, dres (the residual branch's gradient) added into dx."""
    f32 = dict(device=dy.device, dtype=torch.float32)
    dx, dg, db = torch.empty((rows, dim), **f32), torch.empty(dim, **f32), torch.empty(dim, **f32)
    nbytes = lib.ocm_layernorm_backward_workspace_bytes(rows, dim)
    ws = _ws(nbytes, dy.device)
    _lib.check(lib.ocm_op_layernorm_backward(_p(dy), _p(x), _p(w), _p(dres), _p(dx), _p(dg), _p(db), rows, dim, eps, _p(ws),
                                             nbytes, _stream()))
    return dx, dg, db


def _linear(lib, prec, a_op, w_op, bias, resid, M, N, K, epi=_lib.OCM_EPI_BIAS_F32):
    out = torch.empty((M, N), dtype=torch.float32, device=bias.device)
    _lib.check(lib.ocm_op_linear(prec, _p(a_op), _p(w_op), _p(bias), _p(resid), _p(out), M, N, K, epi, _stream()))
    return out


class _EncoderTrain(torch.autograd.Function):
    """The SimMIM / fine-tuning encoder in training mode: forward(meta, x, *params) -> normed tokens (B, N, D); backward ->
    parameter gradients. Per block from meta["first"] on (_first_block_to_train) it keeps the block input (norm1's input), qkv_f32, lse2, the context in the operand type, norm2's input
    and the fp32 fc1 pre-activation: (5 + mlp_ratio) * N * D * 4 bytes per image plus the context (2 or 4 bytes per element)
    — 35 MB per block per image at 384^2, D = 384. The LayerNorm outputs are recomputed in fp32.
    Stochastic depth (meta["scales"]: per branch None or a per-image scale table, _drop_path_scales): a branch with a table runs its
    attn.proj / mlp.fc2 GEMM with the plain bias epilogue into a temporary and ocm_op_drop_path_layernorm writes the new residual
    stream and the NEXT LayerNorm's output (norm2, the next block's norm1, or the final norm), so a site's LayerNorm output may
    arrive from the preceding branch; its backward starts with ocm_op_drop_path_backward while the residual gradient passes on
    unscaled. A branch without a table runs the launches it always ran. The tables are kept with the saved tensors.
    Dropout (meta["dropout"]: None or (seeds, sites), _dropout_sites): pos_drop is ocm_op_dropout in place on the prepared tokens;
    a branch whose proj_drop / second mlp.drop has a rate takes the same hand-off as a scaled one through
    ocm_op_dropout_layernorm (with the branch's scale table, if it has one) and starts its backward with
    ocm_op_dropout_backward; the first mlp.drop is ocm_op_gelu_dropout / ocm_op_gelu_dropout_backward in place of the GELU
    operators. A site at rate 0 runs the launches it always ran. Only the seeds are kept: every mask is recomputed (DESIGN.md
    3.41)."""

    @staticmethod
    def forward(ctx, meta, x, *params):
        enc, eng = meta["enc"], meta["eng"]
        lib, dev = _lib.load(), x.device
        prec = _lib.PRECISIONS[enc._precision]
        P = dict(zip(meta["names"], params))
        B, _, Hpx, Wpx = x.shape
        N, D, H, L = eng.n_tokens(Hpx, Wpx), eng.D, eng.H, eng.L
        hd, T, eps = D // H, B * N, float(enc.norm.eps)
        Mh = enc.blocks[0].mlp.fc1.out_features if L else 4 * D
        f32 = dict(device=dev, dtype=torch.float32)
        adt = _OPERAND_DTYPE[prec]
        kind = _LN_KIND[prec]
        cache = enc.__dict__.setdefault("_train_cache", SourceCache())

        def op(name):
            w = P[name]
            return _cached_operand(cache, name, w, prec, lambda: to_operand(w.detach().to(**f32), prec))

        io = eng._io(x, (x.stride(0), x.stride(1), x.stride(2)), None, B, Hpx, Wpx, meta["pos"])
        if meta["mask"] is not None:
            io.patch_mask = meta["mask"].data_ptr()
        t = torch.empty((T, D), **f32)
        _lib.check(lib.ocm_vit_prepare_tokens(eng._h, C.byref(io), _p(t)))
        npad = lib.ocm_n_pad_prec(prec, N)
        saved = []
        scales = meta["scales"]
        seeds, sites = meta["dropout"] or (None, [None] * (1 + 3 * L))
        if sites[0] is not None:  # pos_drop
            _lib.check(lib.ocm_op_dropout(_p(t), _p(seeds), 0, *sites[0], _p(t), T * D, _stream()))
        xn = out = None  # a LayerNorm output that arrived with the preceding scaled branch (ocm_op_drop_path_layernorm)

        def norm_args(name):
            return P[name + ".weight"], _vec(P.get(name + ".bias"), D, dev)

        for i, blk in enumerate(enc.blocks):
            pre = f"blocks.{i}."
            s_attn, s_mlp = scales[2 * i], scales[2 * i + 1]
            d_proj, d_act, d_fc2 = sites[1 + 3 * i], sites[2 + 3 * i], sites[3 + 3 * i]
            if xn is None:
                xn = _ln(lib, t, *norm_args(pre + "norm1"), kind, T, D, eps, adt)
            q = torch.empty((B * H, npad, hd), dtype=adt, device=dev)
            k = torch.empty_like(q)
            vt = torch.zeros((B * H, hd, npad), dtype=adt, device=dev)
            qkv = torch.empty((3, B, H, N, hd), **f32)
            _lib.check(lib.ocm_op_qkv_proj_hd(prec, _p(xn), _p(op(pre + "attn.qkv.weight")),
                                              _p(_vec(P.get(pre + "attn.qkv.bias"), 3 * D, dev)), _p(q), _p(k), _p(vt),
                                              _p(qkv), B, N, H, hd, _stream()))
            cx = torch.empty((T, D), dtype=adt, device=dev)
            lse = torch.empty((B * H, N), **f32)
            _lib.check(lib.ocm_op_attention_hd(prec, _p(q), _p(k), _p(vt), _p(cx), _p(lse), B, N, H, hd,
                                               float(blk.attn.scale), _stream()))
            del q, k, vt, xn
            if s_attn is None and d_proj is None:
                x1 = _linear(lib, prec, cx, op(pre + "attn.proj.weight"), _vec(P.get(pre + "attn.proj.bias"), D, dev), t, T, D, D,
                             _lib.OCM_EPI_BIAS_RESID_F32)
                xn2 = _ln(lib, x1, *norm_args(pre + "norm2"), kind, T, D, eps, adt)
            else:  # the plain GEMM into a temporary, then residual + scaled branch and norm2 in one kernel
                br = _linear(lib, prec, cx, op(pre + "attn.proj.weight"), _vec(P.get(pre + "attn.proj.bias"), D, dev), None, T,
                             D, D)
                if d_proj is None:
                    x1, xn2 = _drop_path_ln(lib, t, br, s_attn, *norm_args(pre + "norm2"), kind, B, N, D, eps, adt)
                else:
                    x1, xn2 = _dropout_ln(lib, t, br, seeds, 1 + 3 * i, d_proj, s_attn, *norm_args(pre + "norm2"), kind, B, N, D,
                                          eps, adt)
            hpre = _linear(lib, prec, xn2, op(pre + "mlp.fc1.weight"), _vec(P.get(pre + "mlp.fc1.bias"), Mh, dev), None,
                           T, Mh, D)
            del xn2
            g = torch.empty((T, Mh), dtype=adt, device=dev)
            if d_act is None:
                _lib.check(lib.ocm_op_gelu(prec, _p(hpre), _p(g), None, T * Mh, _stream()))
            else:
                _lib.check(lib.ocm_op_gelu_dropout(prec, _p(hpre), _p(seeds), 2 + 3 * i, *d_act, _p(g), None, T * Mh, _stream()))
            xn = None
            if s_mlp is None and d_fc2 is None:
                x2 = _linear(lib, prec, g, op(pre + "mlp.fc2.weight"), _vec(P.get(pre + "mlp.fc2.bias"), D, dev), x1, T, D, Mh,
                             _lib.OCM_EPI_BIAS_RESID_F32)
            else:  # the next LayerNorm is norm1 of the next block, or the final norm (fp32) behind the last block
                br = _linear(lib, prec, g, op(pre + "mlp.fc2.weight"), _vec(P.get(pre + "mlp.fc2.bias"), D, dev), None, T, D, Mh)
                nxt = (*norm_args(f"blocks.{i + 1}.norm1"), kind, B, N, D, eps, adt) if i + 1 < L else (
                    *norm_args("norm"), _lib.OCM_LN_F32, B, N, D, eps, torch.float32)
                if d_fc2 is None:
                    x2, y = _drop_path_ln(lib, x1, br, s_mlp, *nxt)
                else:
                    x2, y = _dropout_ln(lib, x1, br, seeds, 3 + 3 * i, d_fc2, s_mlp, *nxt)
                if i + 1 < L:
                    xn = y
                else:
                    out = y
            del g
            if i >= meta["first"]:
                saved.append((t, qkv, lse, cx, x1, hpre))
            t = x2
        if out is None:
            out = _ln(lib, t, *norm_args("norm"), _lib.OCM_LN_F32, T, D, eps, torch.float32)
        # through save_for_backward: autograd frees them after the backward, refuses a second backward over the same graph
        # and raises if a parameter is modified in place between this forward and the backward
        ctx.meta, ctx.nblocks = meta, len(saved)
        ctx.dims = (B, N, D, H, hd, T, Mh, eps, prec)
        ctx.scaled = [j for j in range(2 * meta["first"], 2 * L) if scales[j] is not None]
        ctx.sites = sites
        ctx.save_for_backward(x, t, *[a for blk in saved for a in blk], *params, *[scales[j] for j in ctx.scaled],
                              *([] if seeds is None else [seeds]))
        return out.reshape(B, N, D)

    @staticmethod
    def backward(ctx, gout):
        meta = ctx.meta
        enc, names = meta["enc"], meta["names"]
        B, N, D, H, hd, T, Mh, eps, prec = ctx.dims
        need = dict(zip(names, ctx.needs_input_grad[2:]))
        st = ctx.saved_tensors
        x, xL, nb, first = st[0], st[1], ctx.nblocks, meta["first"]
        blocks = {first + i: st[2 + 6 * i:8 + 6 * i] for i in range(nb)}
        params = dict(zip(names, st[2 + 6 * nb:]))
        scales = dict(zip(ctx.scaled, st[2 + 6 * nb + len(names):]))  # branch 2 i: attention of block i, 2 i + 1: its MLP
        sites = ctx.sites  # dropout: site 0 pos_drop, 1 + 3 i / 2 + 3 i / 3 + 3 i block i's proj_drop, mlp.drop twice
        seeds = st[-1] if any(d is not None for d in sites) else None
        lib, dev = _lib.load(), gout.device
        f32 = dict(device=dev, dtype=torch.float32)
        cache = enc.__dict__.setdefault("_train_cache", SourceCache())
        grads = {}

        def op_t(name):  # operand copy of W^T: the data gradient dX = dY W runs as ocm_op_linear(dY, W^T)
            w = params[name]
            return _cached_operand(cache, name + ".T", w, prec, lambda: to_operand(w.detach().to(**f32).t().contiguous(), prec))

        zero = partial(_zeros, cache, dev=dev)  # the zero biases of the data-gradient GEMMs

        def wgrad(dy, xin, wname, bname):
            if need.get(wname) or need.get(bname):
                dw, db = _weight_grad(prec, dy, xin, bool(need.get(bname)))
                if need.get(wname):
                    grads[wname] = dw
                if need.get(bname):
                    grads[bname] = db

        def branch_grad(dres, j):
            """(fp32, operand) gradient of branch j from the gradient of the residual stream behind it: that gradient itself, or
            scaled per image where the forward dropped paths (the stream's own gradient passes on unscaled)."""
            site = 1 + 3 * (j // 2) + 2 * (j % 2)
            if sites[site] is not None:
                return _dropout_backward(lib, prec, dres, seeds, site, sites[site], scales.get(j), B, N, D)
            if j in scales:
                return _drop_path_backward(lib, prec, dres, scales[j], B, N, D)
            return dres, to_operand(dres, prec)

        def put(n):
            return _put(grads.get(n), params[n])

        def lngrads(pre, dg, db):
            if need.get(pre + ".weight"):
                grads[pre + ".weight"] = dg
            if need.get(pre + ".bias"):
                grads[pre + ".bias"] = db

        with torch.cuda.device(dev):
            dT = gout.detach().to(torch.float32).contiguous().reshape(T, D)
            dx, dg, db = _ln_backward(lib, dT, xL, params["norm.weight"], None, T, D, eps)
            lngrads("norm", dg, db)
            for i in reversed(range(first, len(enc.blocks))):
                pre = f"blocks.{i}."
                blk = enc.blocks[i]
                xin, qkv, lse, cx, x1, hpre = blocks[i]
                # mlp: x2 = x1 + fc2(gelu(fc1(norm2(x1))))
                db2, db2_op = branch_grad(dx, 2 * i + 1)
                dh = _linear(lib, prec, db2_op, op_t(pre + "mlp.fc2.weight"), zero(Mh), None, T, Mh, D)
                g32 = torch.empty((T, Mh), **f32)
                if sites[2 + 3 * i] is None:
                    _lib.check(lib.ocm_op_gelu_backward(_p(dh), _p(hpre), _p(dh), _p(g32), T * Mh, _stream()))
                else:  # the masked dg through gelu', and the masked activation for fc2's weight gradient
                    _lib.check(lib.ocm_op_gelu_dropout_backward(_p(dh), _p(hpre), _p(seeds), 2 + 3 * i, *sites[2 + 3 * i], _p(dh),
                                                                _p(g32), T * Mh, _stream()))
                wgrad(db2, g32, pre + "mlp.fc2.weight", pre + "mlp.fc2.bias")
                del g32, db2, db2_op
                g2w, g2b = params[pre + "norm2.weight"], _vec(params.get(pre + "norm2.bias"), D, dev)
                if need.get(pre + "mlp.fc1.weight") or need.get(pre + "mlp.fc1.bias"):
                    xn2 = _ln(lib, x1, g2w, g2b, _lib.OCM_LN_F32, T, D, eps, torch.float32)
                    wgrad(dh, xn2, pre + "mlp.fc1.weight", pre + "mlp.fc1.bias")
                    del xn2
                dxn2 = _linear(lib, prec, to_operand(dh, prec), op_t(pre + "mlp.fc1.weight"), zero(D), None, T, D, Mh)
                del dh
                dx1, dg, db = _ln_backward(lib, dxn2, x1, g2w, dx, T, D, eps)
                lngrads(pre + "norm2", dg, db)
                del dxn2, dx
                # attention: x1 = xin + proj(attn(norm1(xin)))
                db1, db1_op = branch_grad(dx1, 2 * i)
                dctx = _linear(lib, prec, db1_op, op_t(pre + "attn.proj.weight"), zero(D), None, T, D, D)
                delta = torch.empty((B * H, N), **f32)
                c32 = torch.empty((T, D), **f32)
                _lib.check(lib.ocm_op_attention_backward_delta(prec, _p(cx), _p(dctx), _p(delta), _p(c32), B, N, H, hd,
                                                               _stream()))
                wgrad(db1, c32, pre + "attn.proj.weight", pre + "attn.proj.bias")
                del c32, db1, db1_op
                dqkv = torch.empty((T, 3 * D), **f32)
                _lib.check(lib.ocm_op_attention_backward(_p(qkv), _p(lse), _p(dctx), _p(delta), _p(dqkv), B, N, H, hd,
                                                         float(blk.attn.scale), _stream()))
                del dctx, delta
                g1w, g1b = params[pre + "norm1.weight"], _vec(params.get(pre + "norm1.bias"), D, dev)
                if need.get(pre + "attn.qkv.weight") or need.get(pre + "attn.qkv.bias"):
                    xn1 = _ln(lib, xin, g1w, g1b, _lib.OCM_LN_F32, T, D, eps, torch.float32)
                    wgrad(dqkv, xn1, pre + "attn.qkv.weight", pre + "attn.qkv.bias")
                    del xn1
                dxn1 = _linear(lib, prec, to_operand(dqkv, prec), op_t(pre + "attn.qkv.weight"), zero(D), None, T, D, 3 * D)
                del dqkv
                dx, dg, db = _ln_backward(lib, dxn1, xin, g1w, dx1, T, D, eps)
                lngrads(pre + "norm1", dg, db)
                del dxn1, dx1
            if first > 0 or not any(need.get(n) for n in names if not n.startswith(("blocks.", "norm."))):
                return (None, None, *[put(n) for n in names])  # nothing below the blocks trains
            # tokens t = pos_drop(cat(cls, patch * (1 - w) + mask_token * w) + pos)
            if sites[0] is not None:
                _lib.check(lib.ocm_op_dropout(_p(dx), _p(seeds), 0, *sites[0], _p(dx), T * D, _stream()))
            mask = meta["mask"]
            P_ = N - 1
            dpatch, dmask, dpos = torch.empty((B * P_, D), **f32), torch.empty(D, **f32), torch.empty((N, D), **f32)
            nbytes = lib.ocm_patch_embed_backward_workspace_bytes(B, N, D)
            ws = _ws(nbytes, dev)
            _lib.check(lib.ocm_op_patch_embed_backward(_p(dx), _p(mask), _p(dpatch), _p(dmask), _p(dpos), B, N, D, _p(ws),
                                                       nbytes, _stream()))
            if need.get("mask_token") and mask is not None:
                grads["mask_token"] = dmask
            if need.get("cls_token"):
                grads["cls_token"] = dpos[0]
            if need.get("patch_embed.proj.weight") or need.get("patch_embed.proj.bias"):
                Cc, p = x.shape[1], enc.patch_embed.patch_size
                cols = torch.empty((B * P_, Cc * p * p), **f32)
                _lib.check(lib.ocm_op_patch_unfold(_p(x), _p(cols), B, Cc, x.shape[2], x.shape[3], p, _stream()))
                wgrad(dpatch, cols, "patch_embed.proj.weight", "patch_embed.proj.bias")
                del cols
            if need.get("pos_embed"):
                # back through the host-side bicubic resampling of _interpolated_pos, with torch autograd on the small table
                pe = params["pos_embed"].detach().float().cpu().requires_grad_(True)
                with torch.enable_grad():
                    full = enc._interpolated_pos(meta["npatch"], *meta["wh"], pos=pe)
                    (gpe,) = torch.autograd.grad(full, pe, dpos.cpu().reshape(full.shape))
                grads["pos_embed"] = gpe
        return (None, None, *[put(n) for n in names])


# ---- the U-Net (model.py:227-320). The nn modules hold the parameters and buffers (same tree, same state_dict keys); the
# arithmetic runs through kernels_conv.hip on token-major fp32 rows: _unet_plan is the graph, _unet_walk the forward. ----
class convolution_block(nn.Module):
    def __init__(self, in_c, out_c):
        super().__init__()
        self.conv1 = nn.Conv2d(in_c, out_c, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm2d(out_c)
        self.conv2 = nn.Conv2d(out_c, out_c, kernel_size=3, padding=1)
        self.bn2 = nn.BatchNorm2d(out_c)
        self.relu = nn.ReLU()


class encoder_block(nn.Module):
    def __init__(self, in_c, out_c):
        super().__init__()
        self.conv = convolution_block(in_c, out_c)
        self.pool = nn.MaxPool2d((2, 2))


class decoder_block(nn.Module):
    def __init__(self, in_c, out_c):
        super().__init__()
        self.up = nn.ConvTranspose2d(in_c, out_c, kernel_size=2, stride=2, padding=0)
        self.conv = convolution_block(out_c + out_c, out_c)


def _rows_up2x2(w):
    """(C, O, 2, 2) ConvTranspose2d kernel -> (4*O, C), row (i*2 + j)*O + o: the N order of ocm_op_upconv2x2."""
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0])


def _unet_composed(prec, out_channels):
    """Whether a 3x3 layer of the U-Net runs as ocm_op_im2col3x3 + ocm_op_linear_relu instead of ocm_op_conv3x3: the layer classes
    at which the direct kernel measured slower at 384^2, batch 8 — in split-bf16 the three deepest levels (512 and
    1024 output channels: e4, b, d1), in fp32 and bf16 the bottleneck. Decided by the layer, not by the batch, so that an image's
    logits do not depend on the batch it is in."""
    return out_channels >= (512 if prec == _lib.OCM_PREC_BF16X3 else 1024)


def _unet_empty(shape, device):
    """Activation buffers of build_unet.forward (fp32). Every element an operator reads was written by the operator before it."""
    return torch.empty(shape, dtype=torch.float32, device=device)


def _rows_up2x2_t(w):
    """(C, O, 2, 2) ConvTranspose2d kernel -> (C, 4*O): the up-convolution's data gradient dIn = g W runs as ocm_op_linear(g, W^T)
    on the rows g of ocm_op_upconv2x2_gather."""
    return _rows_up2x2(w).t()


def _image_kstep(prec):
    """Columns of the first layer's operand: ocm_op_conv3x3_image's 27, padded with zeros to one K step of the operand type."""
    return 64 if prec == _lib.OCM_PREC_BF16 else 32


def _image_rows(rows, prec):
    """The (O, 27) fp32 rows (_rows3x3) of the first layer's kernel -> (O, _image_kstep(prec))."""
    return nn.functional.pad(rows, (0, _image_kstep(prec) - rows.shape[1]))


_UNET_WIDTHS = (64, 128, 256, 512)
_IM2COL_CAP = 1 << 30  # bytes of the fp32 im2col operand one weight-gradient launch of the U-Net reads
_At = collections.namedtuple("_At", "buf col ld")  # columns [col, col + width) of the fp32 rows `buf`, whose row stride is ld
_Step = collections.namedtuple("_Step", "op key bn C O grid src dst")


def _sub(net, key):  # nn.Module.get_submodule without its checks: this runs per layer, per call
    return operator.attrgetter(key)(net)


@lru_cache(maxsize=None)
def _unet_plan(H, W):
    """build_unet's graph, stated once for the forward walk, the backward and the operand cache: [(kind, steps)] in forward order,
    kind "enc" (conv1, conv2, pool) x 4, "mid" (conv1, conv2), "dec" (up, conv1, conv2) x 4, "head". A step names its module
    (`key`; a 3x3 layer also its BatchNorm2d, `bn`: state_dict prefixes), its channels C -> O, the (h, w) grid of its input rows
    and where it reads and writes. torch.cat([up, skip], 1) is the buffer e<k>.cat: the encoder's second convolution writes its
    right half, which the pool reads in place, the up-convolution its left half."""
    def block(pre, lvl, src, C, O, dst):
        t = _At(pre.split(".")[0] + ".t", 0, O)
        return [_Step("conv", pre + ".conv1", pre + ".bn1", C, O, (H >> lvl, W >> lvl), src, t),
                _Step("conv", pre + ".conv2", pre + ".bn2", O, O, (H >> lvl, W >> lvl), t, dst)]

    plan, cur, C = [], _At("x", None, None), 3  # the image is read in place, as (B, 3, H, W) planes
    for lvl, O in enumerate(_UNET_WIDTHS):
        e = f"e{lvl + 1}"
        skip, pooled = _At(e + ".cat", O, 2 * O), _At(e + ".pool", 0, O)
        plan.append(("enc", block(e + ".conv", lvl, cur, C, O, skip)
                     + [_Step("pool", e + ".pool", None, O, O, (H >> lvl, W >> lvl), skip, pooled)]))
        cur, C = pooled, O
    z = _At("b.z", 0, 2 * C)
    plan.append(("mid", block("b", 4, cur, C, 2 * C, z)))
    cur, C = z, 2 * C
    for lvl, O in reversed(list(enumerate(_UNET_WIDTHS))):
        d = f"d{4 - lvl}"
        cat, z = _At(f"e{lvl + 1}.cat", 0, 2 * O), _At(d + ".z", 0, O)
        plan.append(("dec", [_Step("up", d + ".up", None, C, O, (H >> (lvl + 1), W >> (lvl + 1)), cur, cat)]
                     + block(d + ".conv", lvl, cat, 2 * O, O, z)))
        cur, C = z, O
    plan.append(("head", [_Step("head", "outputs", None, C, 1, (H, W), cur, None)]))
    return tuple((kind, tuple(steps)) for kind, steps in plan)


def _im2col_chunks(batch, rows_per_image, k, cap=_IM2COL_CAP):
    """[(first image, images)] of the weight gradient of a 3x3 layer: its fp32 im2col operand (rows_per_image x k per image) is
    built for whole images at a time, as many as fit under `cap` bytes and at least one. A function of the shapes alone: the
    per-chunk gradients are added in this order, so the sum has the same bits on every run."""
    per = max(1, cap // (rows_per_image * k * 4))
    return [(b0, min(per, batch - b0)) for b0 in range(0, batch, per)]


@contextlib.contextmanager
def _phase(net, name):
    """Device time of a part of _UNetTrain.backward for tools/bench_unet_train.py: when the module carries a `_phase_log` list,
    (name, start event, end event) is appended to it; otherwise nothing happens."""
    log = net.__dict__.get("_phase_log")
    if log is None:
        yield
        return
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    yield
    b.record()
    log.append((name, a, b))


def _unet_conv(net, prec, src, grid, C, w_op, bias, dst, ld_out, O, relu):
    """Columns [0, O) of the rows at address dst (row stride ld_out) = the 3x3 pad-1 convolution of src with the (O, 9 C) operand
    + bias, through a ReLU when `relu`. src is dense rows (M, C): the direct kernel, or im2col + GEMM for the layer classes of
    _unet_composed (few rows, long K: the LDS-DMA GEMM measures faster); or the (B, 3, H, W) image, read in place. Serves the
    eval forward (folded operands, ReLU), the training forward and, with the flipped kernel and a zero bias, the data gradients."""
    lib, st, (B, h, w) = _lib.load(), _stream(), grid
    M = B * h * w
    if src.dim() == 4:
        _lib.check(lib.ocm_op_conv3x3_image(prec, _p(src), src.stride(0), src.stride(1), src.stride(2), _p(w_op), _p(bias), dst,
                                            ld_out, B, h, w, O, int(relu), st))
    elif _unet_composed(prec, O):
        cols = net._alloc((M, 9 * C * _OPERAND_DTYPE[prec].itemsize // 4), src.device)  # operand rows, in fp32-sized words
        _lib.check(lib.ocm_op_im2col3x3(prec, _p(src), _p(cols), B, h, w, C, 0, st))
        if relu:
            _lib.check(lib.ocm_op_linear_relu(prec, _p(cols), _p(w_op), _p(bias), dst, ld_out, M, O, 9 * C, st))
        else:  # ocm_op_linear writes dense rows: ld_out == O at every call without ReLU
            _lib.check(lib.ocm_op_linear(prec, _p(cols), _p(w_op), _p(bias), None, dst, M, O, 9 * C, _lib.OCM_EPI_BIAS_F32, st))
    else:
        _lib.check(lib.ocm_op_conv3x3(prec, _p(src), C, _p(w_op), _p(bias), dst, ld_out, B, h, w, C, O, int(relu), st))


def _head_weight(cache, w, prec, dev):
    """The classifier's (64,) fp32 weight: one cache entry for both forwards and the backward."""
    return _cached_operand(cache, "outputs.weight", w, prec,
                           lambda: w.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous())


def _unet_walk(net, x, layer, keep):
    """The forward of build_unet, eval and training: the steps of _unet_plan in order on token-major fp32 rows from net._alloc.
    `layer(prec, step, B, src, dst)` runs one 3x3 layer from the tensor src to the address dst: build_unet._eval_layer, or the
    training step of _unet_train_pass. Without `keep` (inference) a buffer is allocated in front of its first writer and only
    the four [up | skip] buffers and the two newest dense ones (a layer's source and destination) are held; with `keep`
    (training) a stage's buffers are allocated together and all are held. Returns (logits, {name: buffer held}, "x" the image)."""
    lib, dev, prec, st = _lib.load(), x.device, _lib.PRECISIONS[net._precision], _stream()
    B, _, H, W = x.shape
    cache, bufs, dense = net._op_cache, {"x": x}, [None, None]
    for _, stage in _unet_plan(H, W):
        for s in stage:
            if s.op == "head":
                mod, out = _sub(net, s.key), torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
                wo = _head_weight(cache, mod.weight, prec, dev)
                bo = _cached_operand(cache, s.key + ".bias", mod.bias, prec, lambda: _vec(mod.bias, 1, dev))
                _lib.check(lib.ocm_op_conv1x1_planes(_p(bufs[s.src.buf]), s.src.ld, _p(wo), _p(bo), _p(out), B, H * W, s.C, st))
                return out, bufs
            for t in (stage if keep and s.dst.buf not in bufs else (s,)):
                if t.dst.buf not in bufs:
                    bufs[t.dst.buf] = net._alloc((B * t.grid[0] * t.grid[1] // (4 if t.op == "pool" else 1), t.dst.ld), dev)
                    if not keep and t.dst.ld == t.O:  # dense: the one before the last two has no reader left
                        dense.append(t.dst.buf)
                        bufs.pop(dense[-3], None)
            src, dst, (h, w) = bufs[s.src.buf], bufs[s.dst.buf].data_ptr() + 4 * s.dst.col, s.grid
            if s.op == "conv":
                layer(prec, s, B, src, dst)
            elif s.op == "pool":
                _lib.check(lib.ocm_op_maxpool2x2(src.data_ptr() + 4 * s.src.col, s.src.ld, dst, s.dst.ld, B, h, w, s.O, st))
                newest_pool = bufs[s.dst.buf]  # noqa: F841  held until the next pool, e4's until the walk returns: the peak as it was
            else:
                up = _sub(net, s.key)
                wu = _weight_operand(cache, s.key, up.weight, prec, dev, _rows_up2x2)
                bu = _cached_operand(cache, s.key + ".bias", up.bias, prec, lambda: _vec(up.bias, s.O, dev))
                _lib.check(lib.ocm_op_upconv2x2(prec, _p(src), s.src.ld, _p(wu), _p(bu), dst, s.dst.ld, B, h, w, s.C, s.O, st))


def _unet_train_pass(net, x):
    """build_unet in training mode, forward: _unet_walk with the training step — per convolution y = conv(z_prev) + bias (no ReLU,
    raw operands), the batch statistics of y and z = max(y * scale + shift, 0) written where inference writes it. Returns (logits,
    what the backward reads by name, [(BatchNorm2d, batch mean, biased batch variance, values per channel)] in forward order)."""
    lib, dev, cache, st = _lib.load(), x.device, net._op_cache, _stream()
    f32 = dict(device=dev, dtype=torch.float32)
    S, stats = {}, []

    def layer(prec, s, B, src, dst):
        cv, bn, O, M = _sub(net, s.key), _sub(net, s.bn), s.O, B * s.grid[0] * s.grid[1]
        y, bias = net._alloc((M, O), dev), _vec(cv.bias, O, dev)
        if src.dim() == 4:
            w = _cached_operand(cache, s.key + ".image", cv.weight, prec, lambda: to_operand(
                _image_rows(_rows3x3(cv.weight.detach().to(**f32)), prec).contiguous(), prec))
        else:
            w = _weight_operand(cache, s.key, cv.weight, prec, dev, _rows3x3)
        _unet_conv(net, prec, src, (B, *s.grid), s.C, w, bias, y.data_ptr(), O, O, False)
        mean, var = torch.empty(O, **f32), torch.empty(O, **f32)
        nbytes = lib.ocm_channel_reduce_workspace_bytes(M, O)
        ws = _ws(nbytes, dev)
        _lib.check(lib.ocm_op_batch_stats(_p(y), _p(mean), _p(var), M, O, _p(ws), nbytes, st))
        invstd = torch.rsqrt(var + bn.eps)
        g = (bn.weight.detach().to(**f32) * invstd).contiguous()
        h = (_vec(bn.bias, O, dev) - mean * g).contiguous()
        _lib.check(lib.ocm_op_bn_relu(_p(y), _p(g), _p(h), dst, s.dst.ld, M, O, st))
        stats.append((bn, mean, var, M))
        S.update({f"{s.key}.{k}": v for k, v in (("y", y), ("mean", mean), ("invstd", invstd), ("g", g), ("h", h))})

    out, bufs = _unet_walk(net, x, layer, True)
    return out, {**bufs, **S}, stats


class _UNetTrain(torch.autograd.Function):
    """One training-mode call of build_unet: forward(meta, x, *params) -> (B, 1, H, W) logits (_unet_train_pass); backward -> the
    parameter gradients, none for the image: the stages of _unet_plan in reverse. It keeps y (pre-BatchNorm) and z (post-ReLU) of
    all 18 layers, the pooled maps and the per-channel statistics: 5.3 GB at 384^2, batch 8. Weight gradients
    run ocm_op_weight_grad on an fp32 im2col operand built under _IM2COL_CAP (_im2col_chunks), data gradients as the 3x3
    convolution with the flipped kernel; a frozen parameter's weight-gradient launches are skipped. `meta` carries the module
    and, for the caller, the batch statistics (the running statistics are updated outside the graph)."""

    @staticmethod
    def forward(ctx, meta, x, *params):
        out, S, meta["stats"] = _unet_train_pass(meta["net"], x)
        ctx.meta, ctx.keys = meta, list(S)
        ctx.save_for_backward(*S.values(), *params)
        return out

    @staticmethod
    def backward(ctx, gout):
        meta, keys = ctx.meta, ctx.keys
        net, names = meta["net"], meta["names"]
        st_ = ctx.saved_tensors
        S, P = dict(zip(keys, st_[:len(keys)])), dict(zip(names, st_[len(keys):]))
        need = dict(zip(names, ctx.needs_input_grad[2:]))
        lib, dev, prec = _lib.load(), gout.device, _lib.PRECISIONS[net._precision]
        alloc, cache = net._alloc, net._op_cache
        f32 = dict(device=dev, dtype=torch.float32)
        x = S["x"]
        B, _, H, W = x.shape
        grads = {}

        def conv_backward(s, dz, want_dx):
            """Through ReLU, BatchNorm and the convolution of the step s: fills the gradients of the layer's parameters; returns
            the gradient of its source rows when want_dx."""
            key, C, (hh, ww), src = s.key, s.C, s.grid, (None if s.src.buf == "x" else S[s.src.buf])
            y, mean, invstd, g, h = (S[f"{key}.{k}"] for k in ("y", "mean", "invstd", "g", "h"))
            (M, O), st = y.shape, _stream()
            dy, dgam, dbet = alloc((M, O), dev), torch.empty(O, **f32), torch.empty(O, **f32)
            nbytes = lib.ocm_channel_reduce_workspace_bytes(M, O)
            ws = _ws(nbytes, dev)
            _lib.check(lib.ocm_op_bn_relu_backward(_p(dz), _p(y), _p(mean), _p(invstd), _p(g), _p(h), _p(dy), _p(dgam), _p(dbet),
                                                   M, O, _p(ws), nbytes, st))
            if need[s.bn + ".weight"]:
                grads[s.bn + ".weight"] = dgam
            if need[s.bn + ".bias"]:
                grads[s.bn + ".bias"] = dbet
            nw, nb = need[key + ".weight"], need[key + ".bias"]
            if nw or nb:
                K, rpi = (_image_kstep(_lib.OCM_PREC_FP32) if src is None else 9 * C), hh * ww
                dw = db = None
                for b0, n in _im2col_chunks(B, rpi, K):
                    with _phase(net, "weight"):
                        cols = alloc((n * rpi, K), dev)
                        if src is None:
                            _lib.check(lib.ocm_op_im2col3x3_image(_p(x[b0:]), x.stride(0), x.stride(1), x.stride(2), _p(cols), n, hh,
                                                                  ww, st))
                        else:
                            _lib.check(lib.ocm_op_im2col3x3(_lib.OCM_PREC_FP32, _p(src[b0 * rpi:]), _p(cols), n, hh, ww, C, 0, st))
                        dwi, dbi = _weight_grad(prec, dy[b0 * rpi:(b0 + n) * rpi], cols, nb)
                        del cols
                        dw = dwi if dw is None else dw.add_(dwi)
                        if nb:
                            db = dbi if db is None else db.add_(dbi)
                if nw:
                    grads[key + ".weight"] = dw[:, :9 * C].reshape(O, 3, 3, C).permute(0, 3, 1, 2)
                if nb:
                    grads[key + ".bias"] = db
            if not want_dx:
                return None
            dx = alloc((M, C), dev)
            with _phase(net, "data"):
                _unet_conv(net, prec, dy, (B, hh, ww), O, _weight_operand(cache, key, P[key + ".weight"], prec, dev, flip_conv3x3),
                           _zeros(cache, C, dev), dx.data_ptr(), C, C, False)
            return dx

        with torch.cuda.device(dev):
            st = _stream()
            *stages, (_, (head,)) = _unet_plan(H, W)
            # the classifier
            dl = gout.detach().to(torch.float32).contiguous()
            M, C = B * H * W, head.C
            dcur = alloc((M, C), dev)
            nw, nb = need[head.key + ".weight"], need[head.key + ".bias"]
            dwo, dbo = (torch.empty(C, **f32) if nw else None), (torch.empty(1, **f32) if nb else None)
            wo = _head_weight(cache, P[head.key + ".weight"], prec, dev)
            nbytes = lib.ocm_conv1x1_planes_backward_workspace_bytes(M, C)
            ws = _ws(nbytes, dev)
            _lib.check(lib.ocm_op_conv1x1_planes_backward(_p(dl), _p(S[head.src.buf]), head.src.ld, _p(wo), _p(dcur), C, _p(dwo),
                                                          _p(dbo), B, H * W, C, _p(ws), nbytes, st))
            if nw:
                grads[head.key + ".weight"] = dwo
            if nb:
                grads[head.key + ".bias"] = dbo
            dcats = {}  # the gradient of each [up | skip] buffer, from the decoder's first convolution to the encoder's pool
            for kind, stage in reversed(stages):
                if kind == "dec":  # d4 .. d1: conv2, conv1 over [up | skip], the up-convolution
                    up, c1, c2 = stage
                    dz1 = conv_backward(c2, dcur, True)
                    dcat = dcats[c1.src.buf] = conv_backward(c1, dz1, True)
                    del dz1
                    (hs, wsm), O, Cin = up.grid, up.O, up.C
                    Ms = B * hs * wsm
                    g = alloc((Ms, 4 * O), dev)
                    _lib.check(lib.ocm_op_upconv2x2_gather(_p(dcat), up.dst.ld, _p(g), B, hs, wsm, O, st))
                    if need[up.key + ".weight"] or need[up.key + ".bias"]:
                        with _phase(net, "weight"):
                            dw, db = _weight_grad(prec, g, S[up.src.buf], need[up.key + ".bias"])
                        if need[up.key + ".weight"]:
                            grads[up.key + ".weight"] = dw.reshape(2, 2, O, Cin).permute(3, 2, 0, 1)
                        if need[up.key + ".bias"]:
                            grads[up.key + ".bias"] = db.reshape(4, O).sum(0)
                    dcur = alloc((Ms, Cin), dev)
                    wt = _weight_operand(cache, up.key, P[up.key + ".weight"], prec, dev, _rows_up2x2_t)
                    with _phase(net, "data"):
                        _lib.check(lib.ocm_op_linear(prec, _p(to_operand(g, prec)), _p(wt), _p(_zeros(cache, Cin, dev)), None,
                                                     _p(dcur), Ms, Cin, 4 * O, _lib.OCM_EPI_BIAS_F32, st))
                    del g
                elif kind == "mid":
                    c1, c2 = stage
                    dz1 = conv_backward(c2, dcur, True)
                    dcur = conv_backward(c1, dz1, True)
                else:  # e4 .. e1: the pool's backward adds the skip's gradient, the right half of the level's dcat, in place
                    c1, c2, pool = stage
                    (hh, ww), O, skip = pool.grid, pool.O, pool.src
                    cat, dcat = S[skip.buf], dcats.pop(skip.buf)
                    dz = alloc((B * hh * ww, O), dev)
                    _lib.check(lib.ocm_op_maxpool2x2_backward(cat.data_ptr() + 4 * skip.col, skip.ld, _p(dcur), O,
                                                              dcat.data_ptr() + 4 * skip.col, skip.ld, _p(dz), O, B, hh, ww, O, st))
                    del dcat
                    dz1 = conv_backward(c2, dz, True)
                    del dz
                    if c1.src.buf != "x":
                        dcur = conv_backward(c1, dz1, True)
                    else:  # no image gradient
                        conv_backward(c1, dz1, False)
        return (None, None, *[_put(grads.get(n), P[n]) if need[n] else None for n in names])


def _check_unet_input(inputs):
    """What build_unet accepts, eval or training: (B, 3, H, W) that four 2x2 pools divide. Returns (B, H, W)."""
    if not isinstance(inputs, torch.Tensor) or inputs.dim() != 4 or inputs.shape[1] != 3:
        raise RuntimeError(f"build_unet expects a (B, 3, H, W) input, got {tuple(getattr(inputs, 'shape', ()))}")
    B, _, H, W = inputs.shape
    if H % 16 or W % 16 or H == 0 or W == 0 or B == 0:
        raise RuntimeError(f"build_unet needs H and W that are multiples of 16 (four 2x2 pools, then four stride-2 "
                           f"up-convolutions whose outputs are concatenated with the skips); got H={H}, W={W}")
    return B, H, W


def _unet_image(inputs):
    """The fp32 image on its HIP device as the first layer reads it: any batch, plane and row strides, unit pixel stride."""
    _require_hip(inputs, "input")
    x = inputs.detach().to(torch.float32)
    return x if x.stride(3) == 1 else x.contiguous()


class build_unet(nn.Module):
    """model.py:280-320: the U-Net PGT.py trains on pseudo ground truth and unet.py trains supervised. Inference runs on the
    HIP path: every BatchNorm is folded, from its running statistics, into the convolution in front of it; ReLU sits in the
    convolution's epilogue (the deepest layers run as im2col + GEMM, _unet_composed); torch.cat([up, skip], 1) is two writers of
    one 2 O-wide buffer (_unet_plan). Training (PGT.py's train, unet.py) runs on the HIP path for a net that has opted in with
    enable_training(): batch statistics in the forward, the backward through _UNetTrain; any other net keeps refusing training
    mode. Both forwards are _unet_walk. _op_cache is keyed by a layer's state_dict prefix: inference's folded operands under
    "<key>.folded.*", the raw operands of training and the data gradients under "<key>.<layout>" / "<key>.image" — different
    numbers from the same weights, kept apart so that PGT.py's train() / eval() alternation within an epoch rebuilds neither."""

    def __init__(self):
        super().__init__()
        self.e1 = encoder_block(3, 64)
        self.e2 = encoder_block(64, 128)
        self.e3 = encoder_block(128, 256)
        self.e4 = encoder_block(256, 512)
        self.b = convolution_block(512, 1024)
        self.d1 = decoder_block(1024, 512)
        self.d2 = decoder_block(512, 256)
        self.d3 = decoder_block(256, 128)
        self.d4 = decoder_block(128, 64)
        self.outputs = nn.Conv2d(64, 1, kernel_size=1, padding=0)
        self.__dict__["_precision"] = _lib.DEFAULT_PRECISION
        self.__dict__["_op_cache"] = SourceCache()
        self.train_backward = False  # a plain attribute: not a parameter, not a buffer, not in the state_dict
        self.__dict__["_alloc"] = _unet_empty  # a test seam: the memory tests swap in an allocator of poisoned, guard-banded buffers

    @property
    def precision(self):
        return self._precision

    @precision.setter
    def precision(self, name):
        if name not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {name!r}")
        self.__dict__["_precision"] = name

    def enable_training(self, flag=True):
        """Opt this net in to (or out of) training on the HIP path: in training mode forward() then normalises with batch
        statistics, updates the running statistics as nn.BatchNorm2d does and, with grad mode on and a parameter that requires
        grad, builds a graph into the parameters (_UNetTrain). A net that has not opted in refuses training mode."""
        self.train_backward = bool(flag)
        return self

    def _folded(self, name, conv, bn, prec, dev, image=False):
        """(operand copy of the convolution's weight, fp32 bias) with the BatchNorm's running statistics folded in."""
        f32 = dict(device=dev, dtype=torch.float32)

        def gain():
            return bn.weight.detach().to(**f32) / torch.sqrt(bn.running_var.detach().to(**f32) + bn.eps)

        def weight():
            rows = _rows3x3(conv.weight.detach().to(**f32) * gain()[:, None, None, None])
            return to_operand((_image_rows(rows, prec) if image else rows).contiguous(), prec)

        w = _cached_operand(self._op_cache, name + ".folded.weight", (conv.weight, bn.weight, bn.running_var), prec, weight)
        b = _cached_operand(self._op_cache, name + ".folded.bias", (conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var),
                            prec, lambda: ((conv.bias.detach().to(**f32) - bn.running_mean.detach().to(**f32)) * gain()
                                           + bn.bias.detach().to(**f32)).contiguous())
        return w, b

    def _eval_layer(self, prec, s, B, src, dst):
        """The eval step of _unet_walk: folded operands, the convolution with ReLU in its epilogue."""
        w, b = self._folded(s.key, _sub(self, s.key), _sub(self, s.bn), prec, src.device, image=src.dim() == 4)
        _unet_conv(self, prec, src, (B, *s.grid), s.C, w, b, dst, s.dst.ld, s.O, True)

    def forward(self, inputs):
        if self.training and self.train_backward:
            return self._train_forward(inputs)
        if self.training and torch.is_grad_enabled():
            raise NotImplementedError("build_unet runs inference on the HIP path; training (batch statistics, the backward of the "
                                      "convolutions, pool and up-convolution) is not implemented. A new module is in training "
                                      "mode: call .eval() (PGT.py's evaluate / fully_test do), or wrap the call in torch.no_grad(); "
                                      "to train on the HIP path opt in with enable_training()")
        if any(m.training for m in self.modules() if isinstance(m, nn.BatchNorm2d)):
            raise NotImplementedError("a BatchNorm2d of this build_unet is in training mode: inference is what runs on the HIP "
                                      "path (running statistics are folded into the convolutions); call .eval()")
        _check_unet_input(inputs)
        x = _unet_image(inputs)
        with torch.no_grad(), torch.cuda.device(x.device):
            return _unet_walk(self, x, self._eval_layer, False)[0]

    def _train_forward(self, inputs):
        """forward() of a net that has opted in (enable_training) in training mode: what is refused, before anything is launched;
        then the batch-statistics forward, with a graph into the parameters when grad mode is on and one of them requires grad;
        then nn.BatchNorm2d's update of the running statistics."""
        B, H, W = _check_unet_input(inputs)
        if torch.is_grad_enabled() and inputs.requires_grad:
            raise NotImplementedError("the training path does not produce the gradient of the input image; pass an input that "
                                      "does not require grad")
        if not all(m.training for m in self.modules() if isinstance(m, nn.BatchNorm2d)):
            raise NotImplementedError("the training-mode build_unet normalises with batch statistics: a BatchNorm2d in eval mode "
                                      "inside a training build_unet is not supported on the HIP path")
        if B * (H // 16) * (W // 16) < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, 1024, 1, 1]}")
        x = _unet_image(inputs)
        with torch.cuda.device(x.device):
            if _differentiable(self):
                named = list(self.named_parameters())
                meta = {"net": self, "names": [n for n, _ in named]}
                out = _UNetTrain.apply(meta, x, *[p for _, p in named])
                stats = meta.pop("stats")
            else:
                with torch.no_grad():
                    out, _, stats = _unet_train_pass(self, x)
            for bn, mean, var, n in stats:
                if bn.track_running_stats and bn.running_mean is not None:
                    _update_running_stats(bn, mean, var, n)
        return out


def build_model(args):
    """model.py:85-103: the MIM pre-training encoder — depth 4, THREE heads of 128 channels. Heads that are not 64 wide
    run the engine's generic fp32 attention kernel (kernels_attn.hip::attn_generic_kernel); everything else is the
    same MFMA path as the DINO-shaped encoders."""
    return VisionTransformerForSimMIM(patch_size=args.MODEL.PATCH_SIZE, embed_dim=384, depth=4, num_heads=3,
                                      mlp_ratio=4, img_size=[args.DATA.IMG_SIZE], qkv_bias=True,
                                      norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)


def build_finetune_model(args):
    encoder = VisionTransformerForFinetune(patch_size=args.MODEL.PATCH_SIZE, embed_dim=384, depth=12, num_heads=6,
                                           mlp_ratio=4, img_size=[args.DATA.IMG_SIZE], qkv_bias=True,
                                           norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)
    state_dict = get_state_dict(args)
    encoder.load_state_dict(state_dict, strict=False)
    return encoder.enable_finetune()  # finetune.py trains every parameter of this encoder (args.finetune = True)


def get_state_dict(args):
    """model.py:190-226: a local checkpoint file is loaded (weights_only) and its `module.` / `backbone.`
    prefixes stripped. The reference's fallback downloads DINO weights from dl.fbaipublicfiles.com; there is
    no network on this path, so a missing file is an error."""
    if os.path.isfile(args.PRETRAINED_WEIGHTS):
        state_dict = torch.load(args.PRETRAINED_WEIGHTS, map_location="cpu", weights_only=True)
        key = getattr(args, "checkpoint_key", None)
        if key is not None and key in state_dict:
            state_dict = state_dict[key]
        state_dict = {k.replace("module.", ""): v for k, v in state_dict.items()}
        state_dict = {k.replace("backbone.", ""): v for k, v in state_dict.items()}
        return state_dict
    raise FileNotFoundError(f"pretrained weights {args.PRETRAINED_WEIGHTS!r} not found (the reference would download "
                            "DINO weights here; no network on this path)")
