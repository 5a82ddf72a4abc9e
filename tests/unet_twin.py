"""A CPU twin of model.build_unet for the tests: the same submodule tree and state_dict keys (one state_dict loads into both),
with the arithmetic written in torch (F.conv2d, F.batch_norm, F.max_pool2d, F.conv_transpose2d) in whatever dtype the module
holds. `rnd` (optional) rounds the input and the weight of every convolution that the HIP path runs on the MFMA (the 3x3
convolutions and the 2x2 up-convolutions; the 1x1 classifier is an fp32 dot there): the emulation the accuracy bound of
test_unet_gpu.py is measured from. Nothing here reads the reference tree.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


def round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def round_bf16x3(t):
    """hi + lo with hi = bf16(t), lo = bf16(t - hi): what a split-bf16 operand holds."""
    hi = round_bf16(t)
    return hi + round_bf16(t - hi)


ROUNDING = {"fp32": None, "bf16x3": round_bf16x3, "bf16": round_bf16}


def _conv(x, conv, rnd, **kw):
    if rnd is None:
        return F.conv2d(x, conv.weight, conv.bias, **kw)
    return F.conv2d(rnd(x), rnd(conv.weight), conv.bias, **kw)


def _bn(x, bn):
    return F.batch_norm(x, bn.running_mean, bn.running_var, bn.weight, bn.bias, training=bn.training, momentum=bn.momentum,
                        eps=bn.eps)


class convolution_block(nn.Module):
    def __init__(self, in_c, out_c):
        super().__init__()
        self.conv1 = nn.Conv2d(in_c, out_c, kernel_size=3, padding=1)
        self.bn1 = nn.BatchNorm2d(out_c)
        self.conv2 = nn.Conv2d(out_c, out_c, kernel_size=3, padding=1)
        self.bn2 = nn.BatchNorm2d(out_c)
        self.relu = nn.ReLU()

    def forward(self, x, rnd=None):
        x = F.relu(_bn(_conv(x, self.conv1, rnd, padding=1), self.bn1))
        return F.relu(_bn(_conv(x, self.conv2, rnd, padding=1), self.bn2))


class encoder_block(nn.Module):
    def __init__(self, in_c, out_c):
        super().__init__()
        self.conv = convolution_block(in_c, out_c)
        self.pool = nn.MaxPool2d((2, 2))

    def forward(self, x, rnd=None):
        x = self.conv(x, rnd)
        return x, F.max_pool2d(x, 2)


class decoder_block(nn.Module):
    def __init__(self, in_c, out_c):
        super().__init__()
        self.up = nn.ConvTranspose2d(in_c, out_c, kernel_size=2, stride=2, padding=0)
        self.conv = convolution_block(out_c + out_c, out_c)

    def forward(self, x, skip, rnd=None):
        if rnd is None:
            x = F.conv_transpose2d(x, self.up.weight, self.up.bias, stride=2)
        else:
            x = F.conv_transpose2d(rnd(x), rnd(self.up.weight), self.up.bias, stride=2)
        return self.conv(torch.cat([x, skip], dim=1), rnd)


class UNetTwin(nn.Module):
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

    def forward(self, x, rnd=None):
        s1, p1 = self.e1(x, rnd)
        s2, p2 = self.e2(p1, rnd)
        s3, p3 = self.e3(p2, rnd)
        s4, p4 = self.e4(p3, rnd)
        b = self.b(p4, rnd)
        d = self.d1(b, s4, rnd)
        d = self.d2(d, s3, rnd)
        d = self.d3(d, s2, rnd)
        d = self.d4(d, s1, rnd)
        return F.conv2d(d, self.outputs.weight, self.outputs.bias)


def restated_forward(sd, x, eps=1e-5):
    """The eval-mode forward written once more, from the state_dict alone, with no module and no loop over a tree: what the twin
    is checked against (test_unet_host.py)."""
    def block(p, x):
        for i in (1, 2):
            x = F.conv2d(x, sd[f"{p}.conv{i}.weight"], sd[f"{p}.conv{i}.bias"], padding=1)
            mean, var = sd[f"{p}.bn{i}.running_mean"], sd[f"{p}.bn{i}.running_var"]
            x = (x - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + eps)
            x = x * sd[f"{p}.bn{i}.weight"][None, :, None, None] + sd[f"{p}.bn{i}.bias"][None, :, None, None]
            x = x.clamp_min(0)
        return x

    def pool(x):
        return torch.maximum(torch.maximum(x[..., 0::2, 0::2], x[..., 0::2, 1::2]),
                             torch.maximum(x[..., 1::2, 0::2], x[..., 1::2, 1::2]))

    def up(p, x):
        w, b = sd[f"{p}.up.weight"], sd[f"{p}.up.bias"]  # (C, O, 2, 2)
        B, _, h, wd = x.shape
        y = torch.einsum("bchw,coij->bohiwj", x, w).reshape(B, w.shape[1], 2 * h, 2 * wd)
        return y + b[None, :, None, None]

    s1 = block("e1.conv", x)
    s2 = block("e2.conv", pool(s1))
    s3 = block("e3.conv", pool(s2))
    s4 = block("e4.conv", pool(s3))
    d = block("b", pool(s4))
    for name, skip in (("d1", s4), ("d2", s3), ("d3", s2), ("d4", s1)):
        d = block(f"{name}.conv", torch.cat([up(name, d), skip], dim=1))
    return torch.einsum("bchw,oc->bohw", d, sd["outputs.weight"][:, :, 0, 0]) + sd["outputs.bias"][None, :, None, None]


def make_case(seed, x):
    """A float64 twin for input x (B, 3, H, W) float64: torch's default init under `seed`, BatchNorm affine parameters drawn
    away from 1 / 0, running statistics from one training-mode pass over x with momentum 1.0 (so the folded scales are
    realistic and the activations stay O(1) through all 23 layers). Returned in eval mode."""
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    twin = UNetTwin()
    bns = [m for m in twin.modules() if isinstance(m, nn.BatchNorm2d)]
    with torch.no_grad():
        for bn in bns:
            bn.weight.copy_(0.5 + torch.rand(bn.weight.shape, generator=gen))
            bn.bias.copy_(0.3 * torch.randn(bn.bias.shape, generator=gen))
    twin = twin.double()
    for bn in bns:
        bn.momentum = 1.0
    twin.train()
    with torch.no_grad():
        twin(x)
    for bn in bns:
        bn.momentum = 0.1
    return twin.eval()
