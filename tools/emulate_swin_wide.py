"""CPU emulation of the precision modes on a wide-window Swin test geometry (diagnostic, in the style of
tools/emulate_precision.py; never part of the product). Runs the forward of tests/swin_outputs_ref.py with every contraction
operand rounded the way the mode rounds it and prints max |emulated - float64 twin| of logits, pooler_output, last_hidden_state
and the hidden states — the number a bound of tests/test_swin_wide_gpu.py is derived from where the ws <= 7 bound does not hold:
  fp32 : the twin itself in float32 (torch's fp32 operators)
  x3   : x = hi + lo (two bf16), product = hi*hi + hi*lo + lo*hi, float64 accumulation, fp32 everywhere else
  bf16 : both operands rounded to bf16
Usage: python tools/emulate_swin_wide.py [geometry ...]     (default: swinb)"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import swin_oracle as SO  # noqa: E402
from tests import swin_outputs_ref as R  # noqa: E402
from tests import swin_wide_ref as WR  # noqa: E402
from tools.emulate_precision import mm  # noqa: E402


def lin(x, w, b, mode):
    y = mm(x, w.t(), mode)
    return y if b is None else y + b


def layer(sd, pre, x, H, W, heads, ws, shift_cfg, eps, mode):
    B, L, C = x.shape
    shift = shift_cfg if min(H, W) > ws else 0
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_before.weight"], sd[pre + "layernorm_before.bias"], eps).view(B, H, W, C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    Hp, Wp = H + pad_b, W + pad_r
    if pad_r or pad_b:
        y = F.pad(y, (0, 0, 0, pad_r, 0, pad_b))
    if shift > 0:
        y = torch.roll(y, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(y, ws).view(-1, ws * ws, C)
    d, a = C // heads, pre + "attention."
    q, k, v = (lin(win, sd[a + n + "_proj.weight"], sd[a + n + "_proj.bias"], mode).view(-1, ws * ws, heads, d).transpose(1, 2)
               for n in "qkv")
    if mode == "bf16":  # the q | k | v tensor is stored in the element format
        q, k, v = (t.to(torch.bfloat16).float() for t in (q, k, v))
    table = sd[a + "relative_position_bias.relative_position_bias_table"]
    A = ws * ws
    s = mm(q, k.transpose(2, 3), mode) * (d ** -0.5)
    s = s + table[SO.relative_position_index(ws).view(-1)].view(A, A, -1).permute(2, 0, 1).contiguous().unsqueeze(0)
    mask = SO.shift_mask(Hp, Wp, ws, shift, s.dtype)
    if mask is not None:
        nW = mask.shape[0]
        s = s + mask.unsqueeze(1).unsqueeze(0).expand(q.shape[0] // nW, -1, -1, -1, -1).reshape(-1, 1, A, A)
    p = F.softmax(s, dim=-1)
    o = mm(p, v, mode).transpose(1, 2).contiguous().reshape(-1, A, C)
    o = lin(o, sd[a + "o_proj.weight"], sd[a + "o_proj.bias"], mode)
    o = SO.window_reverse(o.view(-1, ws, ws, C), ws, Hp, Wp)
    if shift > 0:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    if pad_r or pad_b:
        o = o[:, :H, :W, :].contiguous()
    x = x + o.view(B, H * W, C)
    y = F.layer_norm(x, (C,), sd[pre + "layernorm_after.weight"], sd[pre + "layernorm_after.bias"], eps)
    y = lin(F.gelu(lin(y, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"], mode)), sd[pre + "mlp.fc2.weight"],
            sd[pre + "mlp.fc2.bias"], mode)
    return y + x


@torch.no_grad()
def forward(sd, cfg, pixel_values, mode):
    """tests/swin_outputs_ref.backbone_outputs with the mode's operand roundings (the patch embedding and the head are fp32 in
    every mode, as in the engine)."""
    if mode == "fp32":
        return R.backbone_outputs(sd, cfg, pixel_values)
    p, eps, ws = cfg["patch_size"], cfg["layer_norm_eps"], cfg["window_size"]
    e = "swin.embeddings."
    x = F.conv2d(pixel_values, sd[e + "patch_embeddings.projection.weight"], sd[e + "patch_embeddings.projection.bias"], stride=p)
    H, W = x.shape[-2:]
    x = x.flatten(2).transpose(1, 2)
    x = F.layer_norm(x, (x.shape[-1],), sd[e + "norm.weight"], sd[e + "norm.bias"], 1e-5)
    hidden = [x]
    ns = len(cfg["depths"])
    for s, (depth, heads) in enumerate(zip(cfg["depths"], cfg["num_heads"])):
        for b in range(depth):
            x = layer(sd, f"swin.encoder.layers.{s}.blocks.{b}.", x, H, W, heads, ws, 0 if b % 2 == 0 else ws // 2, eps, mode)
        if s < ns - 1:
            pre = f"swin.encoder.layers.{s}.downsample."
            B, L, C = x.shape
            t = x.view(B, H, W, C)
            if H % 2 or W % 2:
                t = F.pad(t, (0, 0, 0, W % 2, 0, H % 2))
            t = torch.cat([t[:, row::2, col::2, :] for col in range(2) for row in range(2)], dim=-1).view(B, -1, 4 * C)
            t = F.layer_norm(t, (4 * C,), sd[pre + "norm.weight"], sd[pre + "norm.bias"], 1e-5)
            x = lin(t, sd[pre + "reduction.weight"], None, mode)
            H, W = (H + 1) // 2, (W + 1) // 2
        hidden.append(x)
    C = x.shape[-1]
    seq = F.layer_norm(x, (C,), sd["swin.layernorm.weight"], sd["swin.layernorm.bias"], eps)
    pooled = seq.transpose(1, 2).mean(-1)
    return dict(hidden_states=hidden, last_hidden_state=seq, pooled=pooled,
                logits=F.linear(pooled, sd["classifier.weight"], sd["classifier.bias"]))


def main():
    torch.set_num_threads(16)
    for name in sys.argv[1:] or ["swinb"]:
        batch = 1 if name == "swinb" else 2
        cfg, sd64, x64 = WR.case(name, torch.float64, batch)
        want = R.backbone_outputs(sd64, cfg, x64)
        _, sd, x = WR.case(name, torch.float32, batch)
        for mode in ("fp32", "x3", "bf16"):
            got = forward(sd, cfg, x, mode)
            err = lambda a, b: float((a.double() - b).abs().max())  # noqa: E731
            eh = [err(a, b) for a, b in zip(got["hidden_states"], want["hidden_states"])]
            print(f"{name} {mode:5s}: logits {err(got['logits'], want['logits']):.2e}, pooled {err(got['pooled'], want['pooled']):.2e}, "
                  f"last {err(got['last_hidden_state'], want['last_hidden_state']):.2e}, hidden " + " ".join(f"{v:.2e}" for v in eh)
                  + f"; max |hidden| " + " ".join(f"{float(h.abs().max()):.1f}" for h in want["hidden_states"]))


if __name__ == "__main__":
    main()
