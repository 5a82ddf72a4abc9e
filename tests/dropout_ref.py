"""Dropout's reference for the tests. (1) A vectorised numpy restatement of csrc/philox.h: Philox4x32-10, the threshold, the
keep mask and the factor of a dropout site. (2) A torch twin of the ViT encoder with dropout at the reference's four places
(pos_drop; per block proj_drop, Mlp.drop after the activation and after fc2) and DropPath behind them, in whatever dtype its
leaves have; it builds on tests/drop_path_ref.py and oracle.vit_oracle. The masks are handed in (SiteFactors), not drawn: the
tests make them from the seeds the device forward drew.

Sites: 0 pos_drop; 1 + 3 i, 2 + 3 i, 3 + 3 i block i's proj_drop, Mlp.drop after GELU, Mlp.drop after fc2."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O
from tests.drop_path_ref import _scaled, rel  # noqa: F401  (rel: the tests' error measure)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) of integers below 2^32 -> (..., 4) uint32. Salmon et al., ten rounds."""
    c = [np.asarray(ctr)[..., j].astype(np.uint64) for j in range(4)]
    k = [np.asarray(key)[..., j].astype(np.uint64) for j in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _LOW, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _LOW]
        k = [(k[0] + np.uint64(W0)) & _LOW, (k[1] + np.uint64(W1)) & _LOW]
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(p):
    """(thresh, inv_keep): uint32 floor(p 2^32 + 0.5) formed in double, and the fp32 rounding of the double 1 / (1 - p)."""
    assert 0.0 < p < 1.0
    return int(np.floor(np.float64(p) * 4294967296.0 + 0.5)), np.float32(1.0 / (1.0 - np.float64(p)))


def words(seed, first, count):
    """The uint32 word of elements first .. first + count - 1 of the site whose seed is `seed`."""
    g = np.arange(int(first) >> 2, ((int(first) + count - 1) >> 2) + 1, dtype=np.uint64)  # the groups of four they lie in
    ctr = np.stack([g & _LOW, g >> _S32, np.zeros_like(g), np.zeros_like(g)], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), (g.size, 2))
    out = philox4x32_10(ctr, key).reshape(-1)
    start = int(first) & 3
    return out[start:start + count]


def keep_mask(seed, count, thresh, first=0):
    """uint8 (count,): 1 where the element is kept (word >= thresh)."""
    return (words(int(seed), first, count) >= np.uint32(thresh)).astype(np.uint8)


def factors(seed, count, p):
    """fp32 (count,): inv_keep where kept, 0.0 where dropped."""
    thresh, inv_keep = threshold(p)
    return keep_mask(seed, count, thresh).astype(np.float32) * inv_keep


class SiteFactors:
    """factor(site, shape) of one encoder call: None at rate 0, else the site's factors as a tensor of `shape` (row-major, the
    unpadded tensor). seeds: the 1 + 3 depth int64 entries the forward drew; rates: one rate per site."""

    def __init__(self, seeds, rates):
        self.seeds = None if seeds is None else [int(s) for s in seeds]
        self.rates = list(rates)
        assert self.seeds is None or len(self.seeds) == len(self.rates)
        self._made = {}

    def __call__(self, site, shape):
        p = self.rates[site]
        if p == 0:
            return None
        key = (site, tuple(shape))
        if key not in self._made:
            n = int(np.prod(shape))
            self._made[key] = torch.from_numpy(factors(self.seeds[site], n, p).astype(np.float64)).reshape(*shape)
        return self._made[key]


def site_rates(depth, drop_rate):
    return [drop_rate] * (1 + 3 * depth)


def _drop(t, f):
    return t if f is None else t * f.to(t.dtype)


def blocks_and_norm(sd, cfg, t, scales, fac):
    """drop_path_ref.blocks_and_norm with dropout: tokens (already through pos_drop) -> normed tokens."""
    assert len(scales) == 2 * cfg["depth"]
    for i in range(cfg["depth"]):
        y = O.attention(sd, cfg, i, O.layer_norm(sd, f"blocks.{i}.norm1", t, cfg["eps"]))[0]
        t = t + _scaled(_drop(y, fac(1 + 3 * i, y.shape)), scales[2 * i])
        pre = f"blocks.{i}.mlp."
        h = F.gelu(F.linear(O.layer_norm(sd, f"blocks.{i}.norm2", t, cfg["eps"]), sd[pre + "fc1.weight"], sd[pre + "fc1.bias"]))
        h = _drop(h, fac(2 + 3 * i, h.shape))
        y = F.linear(h, sd[pre + "fc2.weight"], sd[pre + "fc2.bias"])
        t = t + _scaled(_drop(y, fac(3 + 3 * i, y.shape)), scales[2 * i + 1])
    return O.layer_norm(sd, "norm", t, cfg["eps"])


def encoder_tokens(sd, cfg, x, scales, fac):
    """The plain VisionTransformer: prepare_tokens at the input's own size, pos_drop, blocks, norm -> (B, N, D)."""
    t = O.prepare_tokens(sd, cfg, x)
    return blocks_and_norm(sd, cfg, _drop(t, fac(0, t.shape)), scales, fac)


def encoder_fmap(sd, cfg, x, img_size, scales, fac, mask=None, mask_token=None):
    """drop_path_ref.encoder_fmap with dropout -> (B, D, H, W)."""
    p = cfg["patch_size"]
    t = O.patch_embed(sd, x, p)
    B, L, D = t.shape
    if mask is not None:
        tok = mask_token.expand(B, L, -1)
        w = mask.flatten(1).unsqueeze(-1).type_as(tok)
        t = t * (1 - w) + tok * w
    t = torch.cat((sd["cls_token"].expand(B, -1, -1), t), dim=1)
    t = t + (O.interpolate_pos_encoding(sd, L, img_size, img_size, p) if img_size != 224 else sd["pos_embed"])
    t = blocks_and_norm(sd, cfg, _drop(t, fac(0, t.shape)), scales, fac)[:, 1:]
    side = int(L ** 0.5)
    return t.permute(0, 2, 1).reshape(B, D, side, side)


def mim_forward(sd, cfg, x, mask, img_size, mask_token, dec_w, dec_b, stride, scales, fac, in_chans=3):
    """MIM.forward with dropout and drop-path in its encoder -> (loss, x_rec)."""
    z = encoder_fmap(sd, cfg, x, img_size, scales, fac, mask=mask, mask_token=mask_token)
    x_rec = O.conv1x1_pixel_shuffle(z, dec_w, dec_b, stride)
    p = cfg["patch_size"]
    m = mask.repeat_interleave(p, 1).repeat_interleave(p, 2).unsqueeze(1).contiguous()
    loss = ((x - x_rec).abs() * m).sum() / (m.sum() + 1e-5) / in_chans
    return loss, x_rec
