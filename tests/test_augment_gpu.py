"""DINO's augmentation on the device (kernels_augment.hip: ocm_op_gaussian_blur_u8, ocm_op_color_u8; dino/utils.py's GaussianBlur,
Solarization, DataAugmentationDINO) against the numpy restatement tests/augment_ref.py, which tests/test_augment_host.py pins on
live Pillow. Every comparison is bit for bit: bytes, and float32 through its bits. Needs an MI355X."""
import functools
import random
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import augment_ref as A
from vit_ocm_wmsegmentation_amd import utils
from vit_ocm_wmsegmentation_amd.dino import utils as DU
from vit_ocm_wmsegmentation_amd.dino import vision_transformer as VT

pytestmark = pytest.mark.gpu

# sides 1, 2, 5, 63, 64, 65, 97: every pair with a side of 1 that the sizes allow, the pairs either side of the 64 lines a
# workgroup holds, two blocks on both axes (97), and 1024-pixel lines, of which a workgroup holds 7 (two workgroups for 8 lines)
BLUR_SHAPES = [(1, 1), (1, 97), (97, 1), (1, 64), (65, 1), (2, 5), (5, 2), (63, 64), (64, 65), (65, 63), (64, 64), (63, 97),
               (97, 65), (97, 97), (8, 1024), (1024, 8)]
BLUR_RADII = (0.0, 0.3, 1.1, 7.0, 2.0)  # one launch holds a copy, r = 0 twice (1.1: the larger edge weight), r = 6 above the
BLUR_SOLARIZE = (128, 256, 77, 0, 255)  # small sides, and r = 1


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _blur_case(h, w):
    imgs = np.stack([A.noise(h, w, seed=7 * h + w + b) if b % 2 else A.smooth(h, w, seed=7 * h + w + b) for b in range(len(BLUR_RADII))])
    want = np.stack([A.gaussian_blur(im, r) for im, r in zip(imgs, BLUR_RADII)])
    for a in (imgs, want):
        a.setflags(write=False)
    return imgs, want


@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_equals_the_restatement(dev, shape):
    h, w = shape
    assert [A.blur_table(r)[0] for r in BLUR_RADII] == [0, 0, 0, 6, 1]
    imgs, want = _blur_case(h, w)
    x = torch.tensor(imgs, device=dev)
    got = utils.pil_gaussian_blur(x, BLUR_RADII)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    u8, f32 = utils.pil_gaussian_blur(x, BLUR_RADII, to_tensor="both")
    assert np.array_equal(u8.cpu().numpy(), want)
    assert np.array_equal(_bits(f32), np.stack([A.normalize(im) for im in want]).view(np.int32))
    f32 = utils.pil_gaussian_blur(x, BLUR_RADII, to_tensor=True, mean=A.IMAGENET_MEAN, std=A.IMAGENET_STD)
    assert f32.shape == (len(BLUR_RADII), 3, h, w)
    assert np.array_equal(_bits(f32), np.stack([A.normalize(im, A.IMAGENET_MEAN, A.IMAGENET_STD) for im in want]).view(np.int32))
    sol = np.stack([A.solarize(im, t) for im, t in zip(want, BLUR_SOLARIZE)])
    u8, f32 = utils.pil_gaussian_blur(x, BLUR_RADII, solarize=BLUR_SOLARIZE, to_tensor="both", mean=A.IMAGENET_MEAN, std=A.IMAGENET_STD)
    assert np.array_equal(u8.cpu().numpy(), sol)
    assert np.array_equal(_bits(f32), np.stack([A.normalize(im, A.IMAGENET_MEAN, A.IMAGENET_STD) for im in sol]).view(np.int32))
    assert np.array_equal(x.cpu().numpy(), imgs)  # the source is left as it was


def test_normalize_equals_torch(dev):
    """ToTensor and Normalize as torch itself computes them: div(255), then sub_().div_()."""
    imgs, _ = _blur_case(63, 97)
    x = torch.tensor(imgs, device=dev)
    got = utils.pil_gaussian_blur(x, 0.0, to_tensor=True, mean=A.IMAGENET_MEAN, std=A.IMAGENET_STD)
    t = torch.tensor(imgs).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    t.sub_(torch.tensor(A.IMAGENET_MEAN).view(1, 3, 1, 1)).div_(torch.tensor(A.IMAGENET_STD).view(1, 3, 1, 1))
    assert np.array_equal(_bits(got), t.view(torch.int32).numpy())


B, C, S, H = A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE
# contrast in each of the four positions (its mean depends on what ran before), factors at 0, 1 and above 1 (3.0 clips), hue
# shifts 0, 13 and 243, grey and solarize on and off, an image nothing touches, and one with two contrasts
COLOR_OPS = [(C, B, S, H), (H, C, S, B), (B, S, C, H), (S, H, B, C), (0, 0, 0, 0), (C, C, 0, H)]
COLOR_FACTORS = [(1.4, 0.7, 1.2, 13), (243, 0.0, 3.0, 1.0), (1.4, 0.0, 1.0, 0), (0.8, 13, 3.0, 0.6), (0, 0, 0, 0), (1.4, 0.5, 0, 243)]
COLOR_GREY = [False, True, False, True, False, False]
COLOR_SOL = [False, False, True, True, False, True]
COLOR_THR = [128, 128, 128, 77, 128, 200]


@functools.lru_cache(maxsize=None)
def _color_case():
    imgs = np.stack([A.smooth(33, 47, seed=b) if b % 2 else A.noise(33, 47, seed=b) for b in range(6)])
    want = np.stack([A.color(imgs[b], COLOR_OPS[b], COLOR_FACTORS[b], COLOR_GREY[b], COLOR_SOL[b], COLOR_THR[b]) for b in range(6)])
    for a in (imgs, want):
        a.setflags(write=False)
    return imgs, want


def test_color_equals_the_restatement(dev):
    imgs, want = _color_case()
    assert np.array_equal(want[4], imgs[4]) and (want[:4] != imgs[:4]).any()
    x = torch.tensor(imgs, device=dev)
    got = utils.pil_color(x, COLOR_OPS, COLOR_FACTORS, COLOR_GREY, COLOR_SOL, COLOR_THR)
    assert got.data_ptr() != x.data_ptr() and np.array_equal(x.cpu().numpy(), imgs)
    diff = got.cpu().numpy() != want
    assert not diff.any(), [int(d.sum()) for d in diff]
    same = utils.pil_color(x, COLOR_OPS, COLOR_FACTORS, COLOR_GREY, COLOR_SOL, COLOR_THR, out=x)  # in place
    assert same.data_ptr() == x.data_ptr() and np.array_equal(x.cpu().numpy(), want)


def test_reference_classes_on_a_batch(dev):
    imgs, _ = _blur_case(63, 97)
    x = torch.tensor(imgs, device=dev)
    blur, sol = DU.GaussianBlur(0.5, rng=random.Random(4)), DU.Solarization(0.5, rng=random.Random(3))
    twin = DU.GaussianBlur(0.5, rng=random.Random(4))
    radii = [twin.draw() for _ in range(len(imgs))]
    assert 0 < sum(r == 0.0 for r in radii) < len(imgs)  # blurred and not, in one call
    assert np.array_equal(blur(x).cpu().numpy(), np.stack([A.gaussian_blur(im, np.float32(r)) for im, r in zip(imgs, radii)]))
    twin = random.Random(3)
    on = [twin.random() < 0.5 for _ in range(len(imgs))]
    assert 0 < sum(on) < len(imgs)
    assert np.array_equal(sol(x).cpu().numpy(), np.stack([A.solarize(im) if o else im for im, o in zip(imgs, on)]))


def test_multi_crop_augmentation(dev):
    """B = 3 tiles of 40 x 52 to two 32 x 32 and two 16 x 16 views from fixed seeds: every tensor equals the restatement's chain on
    the same tables, one view equals live Pillow's chain when Pillow is installed, and the list feeds MultiCropWrapper."""
    imgs = np.stack([A.smooth(40, 52, seed=20 + b) for b in range(3)])
    x = torch.tensor(imgs, device=dev)
    aug = DU.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 2, global_size=32, local_size=16,
                                  generator=torch.Generator().manual_seed(6), rng=random.Random(7))
    params = aug.params(3, 40, 52)
    assert any(v["ops"].any() for v in params) and any((v["radius"] == 0).any() for v in params[1:])
    views = aug(x, params)
    assert len(views) == 4 and [tuple(v.shape) for v in views] == [(3, 3, 32, 32)] * 2 + [(3, 3, 16, 16)] * 2
    for v, (view, got) in enumerate(zip(params, views)):
        assert got.dtype == torch.float32 and got.is_cuda
        size = 32 if v < 2 else 16
        want = np.stack([A.view_chain(imgs[b], view, b, size) for b in range(3)])
        assert np.array_equal(_bits(got), want.view(np.int32)), v
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        pass
    else:
        for v, b in ((1, 0), (2, 2)):
            want = A.pil_view_chain(imgs[b], params[v], b, 32 if v < 2 else 16)
            assert np.array_equal(_bits(views[v][b]), want.view(np.int32)), (v, b)
    # drawn by the transform itself: the same generators give the same views
    again = DU.DataAugmentationDINO((0.4, 1.0), (0.05, 0.4), 2, global_size=32, local_size=16,
                                    generator=torch.Generator().manual_seed(6), rng=random.Random(7))(x)
    assert all(torch.equal(a, b) for a, b in zip(again, views))
    backbone = VT.VisionTransformer(img_size=[32], patch_size=8, embed_dim=128, depth=1, num_heads=2, mlp_ratio=4, qkv_bias=True,
                                    norm_layer=partial(nn.LayerNorm, eps=1e-6))
    model = DU.MultiCropWrapper(backbone, VT.DINOHead(in_dim=128, out_dim=96, hidden_dim=128, bottleneck_dim=64)).to(dev).train()
    with torch.no_grad():
        out = model(views)
    assert out.shape == (4 * 3, 96) and bool(torch.isfinite(out).all())
