"""Torch twin of the ViT encoder with stochastic depth, for the tests: the reference's Block with its two DropPath sites,
x = x + s_a * attn(LN1 x); x = x + s_m * mlp(LN2 x), built from oracle.vit_oracle's layer_norm / attention / mlp / prepare_tokens
on requires_grad leaves, in whatever dtype the leaves have (float64 for the reference, float32 for torch's own fp32 error). The
per-image scale tables are given, not drawn: the tests redraw them from the seed the device forward used.

Error measure everywhere: max |a - a64| / max |a64| per tensor (rel)."""
import torch

from oracle import vit_oracle as O


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    denom = float(ref.abs().max())
    return float((a - ref).abs().max()) / (denom if denom > 0 else 1.0)


def _scaled(y, scale):
    return y if scale is None else y * scale.to(y.dtype).reshape(-1, 1, 1)


def blocks_and_norm(sd, cfg, t, scales):
    """Tokens (B, N, D) through every block and the final norm; scales: 2 * depth entries (attention, MLP per block), None or a
    (B,) table of 0 and 1 / keep."""
    assert len(scales) == 2 * cfg["depth"]
    for i in range(cfg["depth"]):
        y = O.attention(sd, cfg, i, O.layer_norm(sd, f"blocks.{i}.norm1", t, cfg["eps"]))[0]
        t = t + _scaled(y, scales[2 * i])
        t = t + _scaled(O.mlp(sd, i, O.layer_norm(sd, f"blocks.{i}.norm2", t, cfg["eps"])), scales[2 * i + 1])
    return O.layer_norm(sd, "norm", t, cfg["eps"])


def encoder_tokens(sd, cfg, x, scales):
    """The plain VisionTransformer: prepare_tokens at the input's own size, blocks, norm -> (B, N, D)."""
    return blocks_and_norm(sd, cfg, O.prepare_tokens(sd, cfg, x), scales)


def encoder_fmap(sd, cfg, x, img_size, scales, mask=None, mask_token=None):
    """VisionTransformerForSimMIM.forward (mask given) / VisionTransformerForFinetune.forward with drop-path: oracle.vit_oracle's
    encoder_fmap with the scaled blocks -> (B, D, H, W)."""
    p = cfg["patch_size"]
    t = O.patch_embed(sd, x, p)
    B, L, D = t.shape
    if mask is not None:
        tok = mask_token.expand(B, L, -1)
        w = mask.flatten(1).unsqueeze(-1).type_as(tok)
        t = t * (1 - w) + tok * w
    t = torch.cat((sd["cls_token"].expand(B, -1, -1), t), dim=1)
    t = t + (O.interpolate_pos_encoding(sd, L, img_size, img_size, p) if img_size != 224 else sd["pos_embed"])
    t = blocks_and_norm(sd, cfg, t, scales)[:, 1:]
    side = int(L ** 0.5)
    return t.permute(0, 2, 1).reshape(B, D, side, side)


def mim_forward(sd, cfg, x, mask, img_size, mask_token, dec_w, dec_b, stride, scales, in_chans=3):
    """MIM.forward with drop-path in its encoder -> (loss, x_rec)."""
    z = encoder_fmap(sd, cfg, x, img_size, scales, mask=mask, mask_token=mask_token)
    x_rec = O.conv1x1_pixel_shuffle(z, dec_w, dec_b, stride)
    p = cfg["patch_size"]
    m = mask.repeat_interleave(p, 1).repeat_interleave(p, 2).unsqueeze(1).contiguous()
    loss = ((x - x_rec).abs() * m).sum() / (m.sum() + 1e-5) / in_chans
    return loss, x_rec
