"""References of the Swin SimMIM tests (transformers' SwinForMaskedImageModeling): the cases, a torch twin of its forward that
runs in the dtype of its inputs (float64 as the reference; pinned on the installed transformers by tests/test_swin_mim_host.py)
and a numpy restatement of ocm_op_mim_l1_loss. TEST INFRASTRUCTURE ONLY: nothing in the product imports this file."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import swin_oracle as SO
from vit_ocm_wmsegmentation_amd import synth

BATCH = 2
# name -> the configuration (synth's keys plus encoder_stride) and the seed of its weights, image and mask
CASES = {
    "t96_w6": dict(cfg=dict(image_size=96, num_channels=3, embed_dim=96, depths=(2, 2), num_heads=(3, 6), window_size=6,
                            encoder_stride=8), seed=301),
    "b96_w6": dict(cfg=dict(image_size=96, num_channels=3, embed_dim=128, depths=(2, 2), num_heads=(4, 8), window_size=6,
                            encoder_stride=8), seed=302),  # the widths of microsoft/swin-base-simmim-window6-192
    "t192_w6_s32": dict(cfg=dict(image_size=192, num_channels=3, embed_dim=96, depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24),
                                 window_size=6, encoder_stride=32), seed=303),  # the real 768 -> 3072 decoder
    "gray56_w7": dict(cfg=dict(image_size=56, num_channels=1, embed_dim=32, depths=(2, 1), num_heads=(1, 2), window_size=7,
                               encoder_stride=8), seed=304),  # a 64-wide decoder
}
for _c in CASES.values():
    _c["cfg"].update(patch_size=4, mlp_ratio=4.0, layer_norm_eps=1e-5, num_labels=2)


def hf_kwargs(cfg, **extra):
    """The keyword arguments of SwinConfig (ours or transformers') for a case."""
    return dict({k: v for k, v in cfg.items() if k != "num_labels"}, **extra)


def case(name, batch=BATCH, dtype=torch.float32):
    """-> (cfg, state_dict under SwinForMaskedImageModeling's keys, pixel_values (B, c, S, S), bool_masked_pos (B, L0)).
    synth.synth_swin_state_dict weights without the classifier, a mask token ~ N(0, 0.02^2), a decoder drawn here
    (weight N(0, 0.02^2) as transformers initialises it, bias N(0, 0.02^2)), about 60 % of the patches masked."""
    c = CASES[name]
    cfg, seed = c["cfg"], c["seed"]
    sd = {k: v for k, v in synth.synth_swin_state_dict(cfg, seed=seed).items() if k.startswith("swin.")}
    g = torch.Generator().manual_seed(seed)
    O = cfg["encoder_stride"] ** 2 * cfg["num_channels"]
    Cl = cfg["embed_dim"] * 2 ** (len(cfg["depths"]) - 1)
    sd["swin.embeddings.mask_token"] = 0.02 * torch.randn(1, 1, cfg["embed_dim"], generator=g)
    sd["decoder.0.weight"] = 0.02 * torch.randn(O, Cl, 1, 1, generator=g)
    sd["decoder.0.bias"] = 0.02 * torch.randn(O, generator=g)
    x = synth.synth_tiles(batch, cfg["image_size"], seed=seed + 50, channels=cfg["num_channels"])
    side = cfg["image_size"] // cfg["patch_size"]
    mask = synth.synth_patch_mask(batch, side, seed=seed + 7).bool().reshape(batch, side * side)
    return cfg, {k: v.to(dtype) for k, v in sd.items()}, x.to(dtype), mask


def upstream(shape, seed=11):
    """The fixed random G of reconstruction.backward(G)."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _scaled_layer(sd, pre, x, H, heads, ws, shift, eps, scale):
    """SO.swin_layer on an unpadded grid with the attention branch scaled per image (SwinDropPath: branch / keep * mask)."""
    B, L, C = x.shape
    a = pre + "attention."
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_before.weight"], sd[pre + "layernorm_before.bias"], eps).view(B, H, H, C)
    if shift:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(y, ws).view(-1, ws * ws, C)
    q, k, v = [F.linear(win, sd[a + n + "_proj.weight"], sd[a + n + "_proj.bias"]).view(-1, ws * ws, heads, 32).transpose(1, 2)
               for n in "qkv"]
    table = sd[a + "relative_position_bias.relative_position_bias_table"]
    bias = table[SO.relative_position_index(ws).view(-1)].view(ws * ws, ws * ws, -1).permute(2, 0, 1).unsqueeze(0)
    mask = SO.shift_mask(H, H, ws, shift, x.dtype)
    if mask is not None:
        nW = mask.shape[0]
        bias = bias + mask.unsqueeze(1).unsqueeze(0).expand(win.shape[0] // nW, -1, -1, -1, -1).reshape(-1, 1, ws * ws, ws * ws)
    p = F.softmax(q @ k.transpose(2, 3) * 32 ** -0.5 + bias, dim=-1)
    o = F.linear((p @ v).transpose(1, 2).reshape(-1, ws * ws, C), sd[a + "o_proj.weight"], sd[a + "o_proj.bias"])
    o = SO.window_reverse(o.view(-1, ws, ws, C), ws, H, H)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    keep, m = scale
    x = x + o.reshape(B, L, C).div(keep) * m.view(B, 1, 1)
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_after.weight"], sd[pre + "layernorm_after.bias"], eps)
    return x + F.linear(F.gelu(F.linear(y, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])), sd[pre + "mlp.fc2.weight"],
                        sd[pre + "mlp.fc2.bias"])


def twin(sd, cfg, x, bool_masked_pos=None, scales=None):
    """SwinForMaskedImageModeling.forward (modeling_swin.py) in the dtype of sd and x -> dict(loss (None without a mask),
    reconstruction, last_hidden_state, hidden0 = the embeddings output after the mask-token select). `scales`: per layer None or
    (keep_prob, mask (B,)), the SwinDropPath draws (swin.draw_drop_path_masks); differentiable in sd."""
    e, eps, ws, p = "swin.embeddings.", cfg["layer_norm_eps"], cfg["window_size"], cfg["patch_size"]
    t = F.conv2d(x, sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"], stride=p)
    B, C0, H, _ = t.shape
    t = F.layer_norm(t.flatten(2).transpose(1, 2), (C0,), sd[e + "norm.weight"], sd[e + "norm.bias"], 1e-5)
    if bool_masked_pos is not None:  # SwinEmbeddings: embeddings * (1 - w) + mask_token * w
        w = bool_masked_pos.unsqueeze(-1).to(t.dtype)
        t = t * (1.0 - w) + sd[e + "mask_token"].expand(B, H * H, -1) * w
    hidden0 = t
    li = 0
    for s, (depth, heads) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
        for b in range(depth):
            pre = f"swin.encoder.layers.{s}.blocks.{b}."
            if scales is None or scales[li] is None:
                t = SO.swin_layer(sd, pre, t, H, H, heads, ws, 0 if b % 2 == 0 else ws // 2, eps)
            else:
                sc = (scales[li][0], scales[li][1].to(dtype=t.dtype, device=t.device))
                t = _scaled_layer(sd, pre, t, H, heads, ws, ws // 2 if b % 2 and H > ws else 0, eps, sc)
            li += 1
        if s + 1 < len(cfg["depths"]):
            t = SO.patch_merging(sd, f"swin.encoder.layers.{s}.downsample.", t, H, H)
            H //= 2
    seq = F.layer_norm(t, (t.shape[-1],), sd["swin.layernorm.weight"], sd["swin.layernorm.bias"], eps)
    fmap = seq.transpose(1, 2).reshape(B, -1, H, H)
    rec = F.pixel_shuffle(F.conv2d(fmap, sd["decoder.0.weight"], sd["decoder.0.bias"]), cfg["encoder_stride"])
    loss = None
    if bool_masked_pos is not None:
        side = cfg["image_size"] // p
        m = bool_masked_pos.reshape(-1, side, side).repeat_interleave(p, 1).repeat_interleave(p, 2).unsqueeze(1).contiguous()
        err = F.l1_loss(x, rec, reduction="none")
        # transformers adds 1e-5 to the integer count in torch's default dtype; here the sum is formed in the twin's own dtype
        loss = (err * m).sum() / (m.sum().to(err.dtype) + 1e-5) / cfg["num_channels"]
    return dict(loss=loss, reconstruction=rec, last_hidden_state=seq, hidden0=hidden0)


def twin_grads(name, what, bias_shift=0.0, scales=None, batch=BATCH):
    """float64 (outputs, gradients) of a case: what = "rec" -> reconstruction.backward(upstream), "loss" -> loss.backward()
    with the decoder bias moved by bias_shift."""
    cfg, sd, x, mask = case(name, batch, torch.float64)
    prm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    if bias_shift:
        with torch.no_grad():
            prm["decoder.0.bias"] += bias_shift
    out = twin(prm, cfg, x, mask, scales)
    if what == "rec":
        out["reconstruction"].backward(upstream(out["reconstruction"].shape))
    else:
        out["loss"].backward()
    return {k: (v.detach() if v is not None else None) for k, v in out.items()}, {k: v.grad for k, v in prm.items()}


# ---- ocm_op_mim_l1_loss ------------------------------------------------------------------------------------------------------
def shuffle(lin, B, hp, wp, c, s):
    """rec[b][ch][y*s+i][xx*s+j] = lin[b*hp*wp + y*wp + xx][ch*s*s + i*s + j] (numpy, any dtype)."""
    return lin.reshape(B, hp, wp, c, s, s).transpose(0, 3, 1, 4, 2, 5).reshape(B, c, hp * s, wp * s)


def unshuffle(img, B, hp, wp, c, s):
    return img.reshape(B, c, hp, s, wp, s).transpose(0, 2, 4, 1, 3, 5).reshape(B * hp * wp, c * s * s)


def mim_l1_ref(lin, x, mask, B, hp, wp, c, s, p):
    """ocm_op_mim_l1_loss restated: float32 lin (B*hp*wp, c*s*s) and x (B, c, S, S), uint8 mask (B, S/p, S/p) ->
    (rec float32, dlin float32, loss float64 (not rounded to float32), scale float32)."""
    rec = shuffle(lin, B, hp, wp, c, s)
    m = np.repeat(np.repeat(mask != 0, p, axis=1), p, axis=2)[:, None]  # (B, 1, S, S)
    count = float(p * p * np.count_nonzero(mask))
    scale = np.float32(1.0 / ((count + 1e-5) * c))
    d = rec.astype(np.float64) - x.astype(np.float64)
    loss = float((np.abs(d) * m).sum() / (count + 1e-5) / c)
    drec = (np.sign(d) * m).astype(np.float32) * scale
    return rec, unshuffle(np.ascontiguousarray(drec), B, hp, wp, c, s), loss, scale
