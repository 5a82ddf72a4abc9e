"""The reference's data.py transforms as batched device functions: the decoded uint8 images go to the GPU as they are (a quarter
of the bytes of the fp32 CHW tensor) and Pillow's resample, the crops, the flips and ToTensor run there in one
ocm_op_resample_u8 call per batch (utils.pil_resize, kernels_resample.hip), byte for byte what Pillow and ToTensor give.

  resize_to_tensor           data.py:18-32 (AIP_Dataset, with analyse_attention.py:102-105's Resize: BILINEAR) and :56-83
                             (AIP_Labeled_Dataset, with build_eval_loader's Resize(NEAREST), :296-299): Resize, ToTensor, the
                             cut to a multiple of 8
  cropped_batch              data.py:85-122 (AIP_Croped_Labeled_Dataset, eval.py --crop 4 / 16): .resize((S, S)) with Pillow's
                             default BICUBIC, r x r crops, ToTensor -> the (B, crops, C, s, s) input of eval.segment_images
  random_resized_crop_params torchvision's RandomResizedCrop.get_params on a torch.Generator
  simmim_images              data.py:189-198 (SimMIMTransform.transform_img): RandomResizedCrop, two random flips, ToTensor
  MaskGenerator              data.py:163-186, restated as is (a few integers per image: numpy on the host)

Decoding files stays on the host. torchvision is not installed here: random_resized_crop_params restates its get_params from
the source, and the parity of its random stream with a live torchvision is unpinned. The ROI masking of SimMIMTransform
(data.py:216-233) resizes with skimage's resize(order=0), which is not installed either, and stays out.
"""
import math

import numpy as np
import torch

from . import utils
from .utils import BICUBIC, BILINEAR, NEAREST  # noqa: F401


def _resize_size(height, width, image_size):
    """torchvision's Resize: (h, w) as given; an int matches the smaller edge and keeps the aspect ratio (the longer edge
    truncated)."""
    if isinstance(image_size, (tuple, list)):
        if len(image_size) == 2:
            return int(image_size[0]), int(image_size[1])
        if len(image_size) != 1:
            raise ValueError(f"image_size = {image_size!r} (an int, (size,) or (height, width))")
        image_size = image_size[0]
    s = int(image_size)
    short, long = (width, height) if width <= height else (height, width)
    new_short, new_long = s, int(s * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)


def resize_to_tensor(images_u8, image_size, resample=BILINEAR):
    """Resize(image_size, resample) + ToTensor + img[:, :h - h % 8, :w - w % 8] (data.py:28-30, :70-74) for a batch of decoded
    images: uint8 (B,H,W,C) / (H,W,C) / (H,W) on the HIP device -> float32 (B,C,h8,w8) / (C,h8,w8). image_size: (height,
    width) as torchvision takes it, or an int for the smaller edge. resample: BILINEAR is torchvision's default
    (analyse_attention.py), NEAREST what build_eval_loader asks for, for the images and for the single-channel labels."""
    _, H, W, _, _, _ = utils._u8_image_geometry(images_u8, None)
    h, w = _resize_size(H, W, image_size)
    out = utils.pil_resize(images_u8, (w, h), resample, to_tensor=True)
    return out[..., : h - h % 8, : w - w % 8]


def cropped_batch(images_u8, image_size, crop=4):
    """AIP_Croped_Labeled_Dataset's images (data.py:99-121) for a batch: every image resized to (image_size, image_size) with
    Pillow's default BICUBIC, cut into r x r crops of image_size // r pixels (r = sqrt(crop), rows first), each through
    croped_transform — a NEAREST Resize to its own size, which copies — and ToTensor. uint8 (B,H,W,C) -> float32
    (B, crop, C, s, s), what eval.segment_images takes as its 5-D input."""
    r = int(math.sqrt(int(crop)))
    if r < 1 or r * r != int(crop):
        raise ValueError(f"crop = {crop} (a square number: 4, 16)")
    S = int(image_size)
    s = S // r
    if s < 1:
        raise ValueError(f"image_size = {S} leaves no pixels for {r} x {r} crops")
    if images_u8.dim() != 4:
        raise ValueError(f"expected a (B,H,W,C) batch, got {tuple(images_u8.shape)}")
    full = utils.pil_resize(images_u8, (S, S), BICUBIC, to_tensor=True)  # (B,C,S,S)
    B, Cc = full.shape[:2]
    tiles = full[:, :, : r * s, : r * s].reshape(B, Cc, r, s, r, s)
    return tiles.permute(0, 2, 4, 1, 3, 5).reshape(B, r * r, Cc, s, s).contiguous()


def random_resized_crop_params(height, width, scale=(0.67, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """torchvision.transforms.RandomResizedCrop.get_params restated on a torch.Generator: ten tries of a uniform area in
    `scale` of the image, a log-uniform aspect ratio in `ratio`, w = int(round(sqrt(area * ratio))), h = int(round(sqrt(area /
    ratio))) and, when the rectangle fits, randint origins; then the central crop of the nearest allowed ratio.
    Returns (top, left, h, w). The draws follow torchvision's order (uniform_, uniform_, randint, randint); torchvision is not
    installed here, so the parity of the stream with a live torchvision is unpinned."""
    height, width = int(height), int(width)
    area = height * width
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=generator)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=generator).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=generator).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def simmim_params(batch, height, width, generator=None, scale=(0.67, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """The random choices of SimMIMTransform.transform_img for `batch` images, image after image in the transform's order:
    the crop rectangle, then torch.rand(1) < 0.5 for the horizontal and for the vertical flip.
    Returns (crops (batch,4) int64 as (x0, y0, x1, y1), hflip (batch,) bool, vflip (batch,) bool) numpy arrays."""
    crops, hf, vf = [], [], []
    for _ in range(int(batch)):
        i, j, h, w = random_resized_crop_params(height, width, scale, ratio, generator)
        crops.append((j, i, j + w, i + h))
        hf.append(bool(torch.rand(1, generator=generator).item() < 0.5))
        vf.append(bool(torch.rand(1, generator=generator).item() < 0.5))
    return np.asarray(crops, np.int64).reshape(-1, 4), np.asarray(hf, bool), np.asarray(vf, bool)


def simmim_images(images_u8, img_size, generator=None, return_params=False):
    """SimMIMTransform.transform_img (data.py:192-198) for a batch of decoded RGB tiles in one op call: every image gets its own
    RandomResizedCrop(img_size, scale=(0.67, 1), ratio=(3/4, 4/3)) rectangle, resized to img_size x img_size with torchvision's
    default BILINEAR, its own RandomHorizontalFlip and RandomVerticalFlip (the rows of the coefficient tables reversed: no
    work on the device) and ToTensor. uint8 (B,H,W,3) on the HIP device -> float32 (B,3,img_size,img_size)."""
    if images_u8.dim() != 4:
        raise ValueError(f"expected a (B,H,W,C) batch, got {tuple(images_u8.shape)}")
    B, H, W, _, _, _ = utils._u8_image_geometry(images_u8, None)
    crops, hf, vf = simmim_params(B, H, W, generator)
    S = int(img_size)
    out = utils.pil_resize(images_u8, (S, S), BILINEAR, crop=crops, hflip=hf, vflip=vf, to_tensor=True)
    return (out, (crops, hf, vf)) if return_params else out


class MaskGenerator:
    """data.py:163-186 as it stands: mask_count of the (input_size / mask_patch_size)^2 cells, chosen by
    np.random.permutation, repeated to the model's patch grid."""

    def __init__(self, input_size=192, mask_patch_size=32, model_patch_size=4, mask_ratio=0.6):
        self.input_size = input_size
        self.mask_patch_size = mask_patch_size
        self.model_patch_size = model_patch_size
        self.mask_ratio = mask_ratio
        assert self.input_size % self.mask_patch_size == 0
        assert self.mask_patch_size % self.model_patch_size == 0
        self.rand_size = self.input_size // self.mask_patch_size
        self.scale = self.mask_patch_size // self.model_patch_size
        self.token_count = self.rand_size ** 2
        self.mask_count = int(np.ceil(self.token_count * self.mask_ratio))

    def __call__(self):
        mask_idx = np.random.permutation(self.token_count)[:self.mask_count]
        mask = np.zeros(self.token_count, dtype=int)
        mask[mask_idx] = 1
        mask = mask.reshape((self.rand_size, self.rand_size))
        return mask.repeat(self.scale, axis=0).repeat(self.scale, axis=1)
