"""Float64 twin of the Swin backbone outputs — TEST INFRASTRUCTURE ONLY (tests/test_swin_outputs_*.py).

oracle/swin_oracle.py restates transformers' forward but returns neither the per-stage hidden states in transformers' order
nor the window softmax. This twin is built from that oracle's own pieces (window_partition, window_reverse, shift_mask,
relative_position_index, patch_merging) and returns what SwinModel returns with output_hidden_states=True and — from
attn_implementation="eager" with a hook on every block's attention — output_attentions=True:

  hidden_states           num_stages + 1 tensors (B, L, C): the embeddings output, each stage's output AFTER its patch merging,
                          the last stage's output BEFORE the final LayerNorm
  reshaped_hidden_states  hidden.transpose(1, 2).reshape(B, C, H, W)
  attentions              one (B * nW, heads, ws^2, ws^2) tensor per LAYER, nW counted on the grid padded to the window

It runs in the dtype of its inputs. tests/test_swin_outputs_host.py pins it on live transformers (whose eager softmax is
float32 even in a .double() model: agreement is ~1e-7 there, not 1e-12). `variants=True` also returns, per layer, the
probabilities the same q and k give with the bias table zeroed and without the shift mask: the conditioning checks.
"""
import torch
import torch.nn.functional as F

from oracle import swin_oracle as SO
from vit_ocm_wmsegmentation_amd import synth

# The geometries of the outputs tests: (config overrides, seed). embed_dim 32 / heads (1, 2) are the issue's transformers
# checks; g56w7c96 is the smallest shape on which split-bf16 takes the fused attention half at C = 96 and C = 192.
GEOMETRIES = {
    "g32w4": (dict(image_size=32, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=4), 11),  # shift; grid = window
    "g40w4": (dict(image_size=40, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=4), 12),  # padded 10->12, 5->8
    "g56w7": (dict(image_size=56, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=7), 13),  # window 7, 14-grid
    "g56w7c96": (dict(image_size=56, embed_dim=96, depths=(2, 2), num_heads=(3, 6), window_size=7), 14),
}
# Scale of the synthetic q / k projections and bias table (synth_swin_state_dict qk_gain: table std 0.5 * gain). The default
# init (table std 0.02, near-uniform softmax) would let a wrong bias bin or head order hide inside a tolerance;
# tests/test_swin_outputs_host.py asserts that with this gain a zeroed bias table or a dropped shift mask moves some
# probability of EVERY layer by >= 0.05 while no row saturates (max < 0.999).
QK_GAIN = 3.0


def case(name, dtype=torch.float32, batch=2):
    """(cfg, state_dict, pixel_values) of a GEOMETRIES entry, weights and tiles in `dtype`."""
    over, seed = GEOMETRIES[name]
    cfg = dict(synth.SWIN_TINY, **over)
    sd = {k: v.to(dtype) for k, v in synth.synth_swin_state_dict(cfg, seed=seed, qk_gain=QK_GAIN).items()}
    x = synth.synth_tiles(batch, cfg["image_size"], seed=seed + 50, channels=cfg["num_channels"]).to(dtype)
    return cfg, sd, x


def window_scores(q, k, table, ws, Hp, Wp, shift, zero_bias=False, no_mask=False):
    """q, k (nB, heads, ws^2, d) of the windows of the rolled, padded grid -> softmax input (nB, heads, ws^2, ws^2):
    q k^T / sqrt(d) + relative-position bias + shift mask (SwinSelfAttention.forward)."""
    A = ws * ws
    s = torch.matmul(q, k.transpose(2, 3)) * (q.shape[-1] ** -0.5)
    if not zero_bias:
        s = s + table[SO.relative_position_index(ws).view(-1)].view(A, A, -1).permute(2, 0, 1).contiguous().unsqueeze(0)
    mask = None if no_mask else SO.shift_mask(Hp, Wp, ws, shift, q.dtype)
    if mask is not None:
        nW = mask.shape[0]
        s = s + mask.unsqueeze(1).unsqueeze(0).expand(q.shape[0] // nW, -1, -1, -1, -1).reshape(-1, 1, A, A)
    return s


def window_probs(qkv, B, H, W, heads, ws, shift, table):
    """The probabilities of ocm_op_swin_window_probs: qkv (B * H * W, 3 * 32 * heads) token-major q | k | v rows of a grid that
    is a multiple of the window -> (B * nW, heads, ws^2, ws^2)."""
    C = heads * 32
    t = qkv.view(B, H, W, 3 * C)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(t, ws).view(-1, ws * ws, 3, heads, 32)
    q, k = win[:, :, 0].transpose(1, 2), win[:, :, 1].transpose(1, 2)
    return F.softmax(window_scores(q, k, table, ws, H, W, shift), dim=-1)


def layer(sd, pre, x, H, W, heads, ws, shift_cfg, eps, variants=False):
    """SwinLayer.forward as oracle.swin_oracle.swin_layer computes it -> (output, probabilities, variants or None)."""
    B, L, C = x.shape
    shift = shift_cfg if min(H, W) > ws else 0  # set_shift_and_window_size (a grid smaller than the window is not built)
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_before.weight"], sd[pre + "layernorm_before.bias"], eps).view(B, H, W, C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    Hp, Wp = H + pad_b, W + pad_r
    if pad_r or pad_b:
        y = F.pad(y, (0, 0, 0, pad_r, 0, pad_b))
    if shift > 0:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(y, ws).view(-1, ws * ws, C)
    d, a = C // heads, pre + "attention."
    q, k, v = (F.linear(win, sd[a + n + "_proj.weight"], sd[a + n + "_proj.bias"]).view(-1, ws * ws, heads, d).transpose(1, 2)
               for n in "qkv")
    table = sd[a + "relative_position_bias.relative_position_bias_table"]
    p = F.softmax(window_scores(q, k, table, ws, Hp, Wp, shift), dim=-1)
    var = None
    if variants:
        var = dict(zero_bias=F.softmax(window_scores(q, k, table, ws, Hp, Wp, shift, zero_bias=True), dim=-1),
                   no_mask=F.softmax(window_scores(q, k, table, ws, Hp, Wp, shift, no_mask=True), dim=-1), shift=shift)
    o = torch.matmul(p, v).transpose(1, 2).contiguous().reshape(-1, ws * ws, C)
    o = F.linear(o, sd[a + "o_proj.weight"], sd[a + "o_proj.bias"])
    o = SO.window_reverse(o.view(-1, ws, ws, C), ws, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    if pad_r or pad_b:
        o = o[:, :H, :W, :].contiguous()
    x = x + o.view(B, H * W, C)
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_after.weight"], sd[pre + "layernorm_after.bias"], eps)
    y = F.linear(F.gelu(F.linear(y, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])), sd[pre + "mlp.fc2.weight"],
                 sd[pre + "mlp.fc2.bias"])
    return y + x, p, var


def reshape_hidden(h, H, W):
    B, L, C = h.shape
    return h.transpose(1, 2).reshape(B, C, H, W)


@torch.no_grad()
def backbone_outputs(sd, cfg, pixel_values, variants=False):
    """-> dict(hidden_states, reshaped_hidden_states, attentions, last_hidden_state, pooled, logits[, variants])."""
    p, eps, ws = cfg["patch_size"], cfg["layer_norm_eps"], cfg["window_size"]
    e = "swin.embeddings."
    x = F.conv2d(pixel_values, sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"],
                 stride=p)
    H, W = x.shape[-2:]
    x = x.flatten(2).transpose(1, 2)
    x = F.layer_norm(x, (x.shape[-1],), sd[e + "norm.weight"], sd[e + "norm.bias"], 1e-5)
    hidden, reshaped, attn, var = [x], [reshape_hidden(x, H, W)], [], []
    ns = len(cfg["depths"])
    for s, (depth, heads) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
        for b in range(depth):
            x, pr, v = layer(sd, f"swin.encoder.layers.{s}.blocks.{b}.", x, H, W, heads, ws, 0 if b % 2 == 0 else ws // 2, eps,
                             variants)
            attn.append(pr)
            var.append(v)
        if s < ns - 1:
            x = SO.patch_merging(sd, f"swin.encoder.layers.{s}.downsample.", x, H, W)
            H, W = (H + 1) // 2, (W + 1) // 2
        hidden.append(x)
        reshaped.append(reshape_hidden(x, H, W))
    C = x.shape[-1]
    seq = F.layer_norm(x, (C,), sd["swin.layernorm.weight"], sd["swin.layernorm.bias"], eps)
    pooled = seq.transpose(1, 2).mean(-1)
    out = dict(hidden_states=hidden, reshaped_hidden_states=reshaped, attentions=attn, last_hidden_state=seq, pooled=pooled,
               logits=F.linear(pooled, sd["classifier.weight"], sd["classifier.bias"]))
    if variants:
        out["variants"] = var
    return out
