"""Torch twins of the DINO training pieces (dino/vision_transformer.py DINOHead, dino/utils.py DINOLoss, the centre, the EMA) for
the tests: a head built from nn.Linear / nn.GELU / F.normalize / nn.utils.weight_norm, the loss and centre formulas of
include/ocm_vit.h in whatever dtype the inputs have (float64 for the reference, float32 for torch's own fp32 error), the CLS row of
the oracle's encoder on requires_grad leaves, and the fingerprints of the two map encoders' training outputs and gradients.

Error measure everywhere: max |a - a64| / max |a64| per tensor (rel)."""
import hashlib
import warnings
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import vit_oracle as O


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    denom = float(ref.abs().max())
    return float((a - ref).abs().max()) / (denom if denom > 0 else 1.0)


class TwinHead(nn.Module):
    """The DINO projection head as plain torch modules: an MLP of nlayers Linear layers with GELU between them (BatchNorm1d after
    every hidden Linear with use_bn), L2 normalisation of the bottleneck, a weight-normed bias-free last Linear whose magnitudes
    start at 1 and are frozen with norm_last_layer."""

    def __init__(self, in_dim, out_dim, use_bn=False, norm_last_layer=True, nlayers=3, hidden_dim=2048, bottleneck_dim=256):
        super().__init__()
        n = max(nlayers, 1)
        if n == 1:
            self.mlp = nn.Linear(in_dim, bottleneck_dim)
        else:
            mods, width = [], in_dim
            for _ in range(n - 1):
                mods.append(nn.Linear(width, hidden_dim))
                if use_bn:
                    mods.append(nn.BatchNorm1d(hidden_dim))
                mods.append(nn.GELU())
                width = hidden_dim
            mods.append(nn.Linear(width, bottleneck_dim))
            self.mlp = nn.Sequential(*mods)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.last_layer = nn.utils.weight_norm(nn.Linear(bottleneck_dim, out_dim, bias=False))
        self.last_layer.weight_g.data.fill_(1)
        if norm_last_layer:
            self.last_layer.weight_g.requires_grad = False

    def forward(self, x):
        return self.last_layer(F.normalize(self.mlp(x), dim=-1, p=2))


def fill_head(head, seed, g_spread=0.0):
    """Deterministic values for a head's parameters (either implementation: the keys are the same): N(0, 0.05) weights, N(0, 0.02)
    biases, weight_g = 1 + g_spread * N(0, 1). Returns the state dict it loaded."""
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in head.state_dict().items():
        if k.endswith("weight_g"):
            sd[k] = 1.0 + g_spread * torch.randn(v.shape, generator=gen)
        elif k.endswith("bias"):
            sd[k] = 0.02 * torch.randn(v.shape, generator=gen)
        elif v.dtype.is_floating_point and "running" not in k:
            sd[k] = 0.05 * torch.randn(v.shape, generator=gen)
        else:
            sd[k] = v.clone()
    head.load_state_dict(sd, strict=True)
    return sd


def l2_normalize(x):
    norm = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return x / norm, norm[..., 0]


def weight_norm(v, g):
    norm = v.norm(dim=1)
    return v * (g / norm)[:, None], norm


def dino_loss(student, teacher, center, student_temp, teacher_temp, ncrops):
    """The DINO loss of include/ocm_vit.h in the dtype of its inputs: student (V*B, K) crop-major, teacher (2*B, K), center (K,)."""
    B = teacher.shape[0] // 2
    logp = F.log_softmax(student / student_temp, dim=-1).reshape(ncrops, B, -1)
    q = F.softmax((teacher - center) / teacher_temp, dim=-1).reshape(2, B, -1)
    total, terms = 0.0, 0
    for i in range(2):
        for v in range(ncrops):
            if v == i:
                continue
            total = total + (-q[i] * logp[v]).sum(dim=-1).mean()
            terms += 1
    return total / terms


def center_update(center, batch_sum, count, momentum):
    """The three fp32 statements of the centre update, from a batch sum."""
    mean = batch_sum / count
    keep = center * momentum
    return keep + mean * (1 - momentum)


def sequential_sum(teacher):
    """Rows added in rising order in the tensor's own dtype: the order ocm_op_dino_center's sum has."""
    s = teacher[0].clone()
    for r in range(1, teacher.shape[0]):
        s = s + teacher[r]
    return s


def teacher_temp_schedule(warmup, final, warmup_epochs, nepochs):
    import numpy as np
    return np.concatenate((np.linspace(warmup, final, warmup_epochs), np.ones(nepochs - warmup_epochs) * final))


def encoder_cls(sd, cfg, x):
    """The normed CLS row of the oracle's encoder with the graph kept (oracle.vit_oracle.forward_feats runs under no_grad): the
    same steps, position table interpolated to the input's own size."""
    t = O.prepare_tokens(sd, cfg, x)
    for i in range(cfg["depth"]):
        t = O.block(sd, cfg, i, t)[0]
    return O.layer_norm(sd, "norm", t, cfg["eps"])[:, 0]


# ---- the two map encoders' training path, fingerprinted: WRAPPER_CASES' wrap_p8_64 encoder (dim 128, depth 2, 2 heads, patch 8,
# batch 2, seed 11) on 224^2 tiles, the position table's native 28 x 28 grid, so nothing but device kernels forms the values ----
def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def encoder_fingerprints(dev, precision):
    """{"finetune" | "simmim": {"out" | parameter name: 16 hex digits of sha256 over the fp32 bytes}} of
    VisionTransformerForFinetune (opted in) and VisionTransformerForSimMIM in training mode: the output map and every gradient of
    out.backward(G), G a fixed normal tensor."""
    from vit_ocm_wmsegmentation_amd import model as M
    from vit_ocm_wmsegmentation_amd import synth
    dim, depth, heads, patch, size, batch, seed = 128, 2, 2, 8, 224, 2, 11
    sd = synth.synth_state_dict(dim, depth, patch, seed=seed, variant="full", img_size=size)
    wp = synth.synth_wrapper_params(dim, patch, 3, seed=seed)
    x = synth.synth_tiles(batch, size, seed=seed + 100).to(dev)
    mask = synth.synth_patch_mask(batch, size // patch, seed=seed)
    kw = dict(patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=4, img_size=[size], qkv_bias=True,
              norm_layer=partial(nn.LayerNorm, eps=1e-6), interpolate_encoding=True)
    out = {}
    for kind in ("finetune", "simmim"):
        if kind == "finetune":
            enc = M.VisionTransformerForFinetune(**kw)
            enc.load_state_dict(sd, strict=True)
            enc.enable_finetune()
        else:
            enc = M.VisionTransformerForSimMIM(**kw)
            enc.load_state_dict(dict(sd, mask_token=wp["mask_token"]), strict=True)
        enc.set_precision(precision)
        enc = enc.to(dev).train()
        y = enc(x) if kind == "finetune" else enc(x, mask)
        g = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(dev)
        y.backward(g)
        torch.cuda.synchronize()
        prints = {"out": _digest(y)}
        for n, p in enc.named_parameters():
            if p.grad is not None:
                prints[n] = _digest(p.grad)
        out[kind] = prints
    return out
