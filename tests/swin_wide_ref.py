"""Cases and float64 references of the wide-window Swin tests (windows of 8 to 12) — TEST INFRASTRUCTURE ONLY
(tests/test_swin_wide_*.py). The arbiter is oracle/swin_oracle.py and its float64 twin tests/swin_outputs_ref.py, both generic
in the window; this module only names the geometries, their seeds, and the stand-alone operators' inputs."""
import torch

from oracle import swin_oracle as SO
from tests import swin_outputs_ref as R
from vit_ocm_wmsegmentation_amd import synth

# (config overrides, seed). The seeds are conditioned by tests/test_swin_wide_host.py: a wrong bias bin, a swapped head or a
# dropped shift mask moves some probability of every layer it applies to by >= 0.05.
GEOMETRIES = {
    "w96": (dict(image_size=96, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=12), 21),    # shift; grid = window
    "w192": (dict(image_size=192, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=12), 22),  # shift in both stages
    "w80": (dict(image_size=80, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=8), 23),     # padded 20->24, 10->16
    "w72": (dict(image_size=72, embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=9), 24),     # odd window
    "w88": (dict(image_size=88, embed_dim=64, depths=(2, 2), num_heads=(2, 4), window_size=11), 25),    # odd window, more heads
}
TINY = tuple(GEOMETRIES)
# Swin-B widths (C = 128 .. 1024, 4 .. 32 heads) at two layers per stage: logits and hidden states only, B = 1
SWIN_B = (dict(image_size=384, embed_dim=128, depths=(2, 2, 2, 2), num_heads=(4, 8, 16, 32), window_size=12), 26)
# Swin-B/window12/384 itself (the checkpoint's depths): shapes only
SWIN_B_FULL = dict(synth.SWIN_TINY, image_size=384, embed_dim=128, depths=(2, 2, 18, 2), num_heads=(4, 8, 16, 32), window_size=12)


def config(name):
    over, seed = SWIN_B if name == "swinb" else GEOMETRIES[name]
    return dict(synth.SWIN_TINY, **over), seed


def case(name, dtype=torch.float32, batch=2):
    """(cfg, state_dict, pixel_values) of a geometry, weights and tiles in `dtype` (the scheme of swin_outputs_ref.case)."""
    cfg, seed = config(name)
    sd = {k: v.to(dtype) for k, v in synth.synth_swin_state_dict(cfg, seed=seed, qk_gain=R.QK_GAIN).items()}
    x = synth.synth_tiles(batch, cfg["image_size"], seed=seed + 50, channels=cfg["num_channels"]).to(dtype)
    return cfg, sd, x


def window_context(qkv, B, H, W, heads, ws, shift, table):
    """ocm_op_swin_window_attention in the dtype of its inputs: qkv (B * H * W, 3 * 32 * heads) -> ctx (B * H * W, 32 * heads)
    at each token's own row, and the probabilities (B * nW, heads, ws^2, ws^2) it is built from."""
    C = heads * 32
    t = qkv.view(B, H, W, 3 * C)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    win = SO.window_partition(t, ws).view(-1, ws * ws, 3, heads, 32)
    q, k, v = (win[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(R.window_scores(q, k, table, ws, H, W, shift), dim=-1)
    o = SO.window_reverse((p @ v).transpose(1, 2).reshape(-1, ws, ws, C), ws, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(B * H * W, C), p


def masked_entries(H, W, ws, shift, dtype=torch.float64):
    """Boolean (nW, ws^2, ws^2): the (query, key) pairs get_attn_mask separates; None without a shift."""
    m = SO.shift_mask(H, W, ws, shift, dtype)
    return None if m is None else m != 0
