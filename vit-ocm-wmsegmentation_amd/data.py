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
  roi_mask                   data.py:216-233 (SimMIMTransform.__call__ with --roi_masking): the random masks of a batch kept only
                             on tissue — grey level > 10, get_ROIs, resize(order=0) onto the patch grid, mask * rois unless that
                             is empty — in five operator calls per batch (kernels_roi.hip, kernels_morph.hip)
  SimMIMTransform            data.py:189-253 for a batch: simmim_images, the MaskGenerator draws and, with args.roi_masking,
                             roi_mask -> (img, mask), what MIM.forward takes

Decoding files stays on the host. torchvision is not installed here: random_resized_crop_params restates its get_params from
the source, and the parity of its random stream with a live torchvision is unpinned.

To switch build_loader_simmim (data.py:271-280) over: let the dataset return the decoded uint8 (H,W,3) tile as it is (no
transform in the workers), collate with default_collate, and in the training loop call
    transform = SimMIMTransform(args)                  # once
    img, mask = transform(batch_u8.to(device))         # per step; mim(img, mask) as before
scikit-image is not installed here either, so the parity of roi_mask with skimage itself is unpinned; what is pinned on live
libraries (tests/test_roi_mask_host.py) is what skimage 0.19.3 calls and what the chain is made of: scipy.ndimage.zoom(order=0,
mode='mirror', grid_mode=True) for resize(order=0, anti_aliasing=False), scipy.ndimage's dilation, erosion and label, Pillow's
convert('L'), torch's mul(255).byte() and numpy's float64 -> uint8 cast.
"""
import functools
import math

import numpy as np
import torch

from . import _lib, utils
from .engine import _p, _require_hip, _stream, _ws
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


@functools.lru_cache(maxsize=16)
def _roi_tables(h, w, gh, gw, device):
    """utils.roi_sample_index of both axes as one int32 device tensor (rows, then columns): one upload per geometry and device."""
    return torch.from_numpy(np.concatenate([utils.roi_sample_index(h, gh), utils.roi_sample_index(w, gw)])).to(device)


def roi_mask(images, masks, level=10, min_size=20):
    """The ROI step of SimMIMTransform.__call__ (data.py:216-233) for a batch, nothing copied to the host. Per image:
      binary = 255 where ToPILImage()(img).convert('L') > level, else 0 (uint8)
      rois   = get_ROIs(binary): remove_small_objects -> binary_closing(disk(2)) -> label (8-connected)
      rois   = resize(rois, mask.shape, order=0, anti_aliasing=False, preserve_range=True).astype(np.uint8) != 0
      mask   = mask * rois, unless that is empty: then the mask stays as it was
    Two quirks of the reference are kept (utils.get_ROIs documents the first). remove_small_objects reads the uint8 image as a
    label image, so the white class is cleared as a whole, and only when it holds fewer than min_size pixels IN TOTAL — its
    components do not matter. And the uint8 cast of the float64 label image wraps modulo 256 (numpy on x86-64: 256.0 -> 0,
    257.0 -> 1, no warning), so a sampled label that is a multiple of 256 counts as background: (label & 255) != 0.
    images: float32 (B,C,S1,S2) on the HIP device, C in (1, 3), read through its image and channel strides (a batch slice is
    not copied). masks: (B,gh,gw) int64 / uint8 / bool on the same device. Returns (new_masks of the dtype and shape of masks,
    holding 0 / 1; used: bool (B,), whether image b got mask * rois). The sampling is utils.roi_sample_index."""
    _require_hip(images, "images")
    _require_hip(masks, "masks")
    if images.dim() != 4 or images.dtype != torch.float32 or images.shape[1] not in (1, 3):
        raise ValueError(f"expected float32 (B,C,H,W) images with C in (1,3), got {images.dtype} {tuple(images.shape)}")
    if masks.dim() != 3 or masks.dtype not in (torch.int64, torch.uint8, torch.bool) or masks.shape[0] != images.shape[0]:
        raise ValueError(f"expected int64 / uint8 / bool (B,gh,gw) masks for {images.shape[0]} images, got {masks.dtype} "
                         f"{tuple(masks.shape)}")
    if masks.device != images.device:
        raise ValueError(f"images on {images.device}, masks on {masks.device}: one device per call")
    B, Cc, h, w = images.shape
    gh, gw = int(masks.shape[1]), int(masks.shape[2])
    if B < 1 or gh < 1 or gw < 1 or h < 1 or w < 1:
        raise ValueError(f"empty batch, image or grid: images {tuple(images.shape)}, masks {tuple(masks.shape)}")
    if images.stride(3) != 1 or images.stride(2) != w or (Cc == 3 and images.stride(1) < h * w) or (
            B > 1 and images.stride(0) < h * w):
        images = images.contiguous()
    dev, lib = images.device, _lib.load()
    m = masks.contiguous()
    binary = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
    grown = torch.empty_like(binary)
    white = torch.empty(B, dtype=torch.int32, device=dev)
    labels = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.ocm_label8_workspace_bytes(B, h, w)
    ws = _ws(nbytes, dev)
    tables = _roi_tables(h, w, gh, gw, dev)
    out = torch.empty_like(m)
    used = torch.empty(B, dtype=torch.bool, device=dev)
    size, bits = utils.footprint_bits(utils.DISK2)
    with torch.cuda.device(dev):
        s = _stream()
        _lib.check(lib.ocm_op_roi_threshold(_p(images), int(images.stride(0)), int(images.stride(1)), Cc, B, h, w, int(level),
                                            _p(binary), _p(white), s))
        _lib.check(lib.ocm_op_binary_morph(_p(binary), _p(grown), B, h, w, bits, size, 0, 0, s))
        _lib.check(lib.ocm_op_binary_morph(_p(grown), _p(binary), B, h, w, bits, size, 1, 1, s))  # binary: now the closed mask
        _lib.check(lib.ocm_op_label8(_p(binary), _p(labels), _p(counts), B, h, w, _p(ws), nbytes, s))
        _lib.check(lib.ocm_op_roi_apply(_p(labels), _p(tables), tables.data_ptr() + 4 * gh, _p(white), int(min_size), _p(m),
                                        m.element_size(), _p(out), _p(used), B, h, w, gh, gw, s))
    return out, used


class SimMIMTransform:
    """data.py:189-253 for a batch of decoded tiles. args carries what the reference reads: DATA.IMG_SIZE, DATA.MASK_PATCH_SIZE,
    DATA.MASK_RATIO, MODEL.PATCH_SIZE and roi_masking. The cv2.imwrite calls of the reference (:234-250, debug PNGs to a fixed
    path) are not part of this."""

    def __init__(self, args):
        self.roi_masking = args.roi_masking
        self.image_size = args.DATA.IMG_SIZE
        self.mask_generator = MaskGenerator(
            input_size=args.DATA.IMG_SIZE,
            mask_patch_size=args.DATA.MASK_PATCH_SIZE,
            model_patch_size=args.MODEL.PATCH_SIZE,
            mask_ratio=args.DATA.MASK_RATIO,
        )

    def __call__(self, images_u8, generator=None):
        """uint8 (B,H,W,3) on the HIP device -> (img float32 (B,3,S,S) = simmim_images, mask int64 (B,G,G) on the device, G =
        IMG_SIZE / MODEL.PATCH_SIZE). The masks are drawn image after image by MaskGenerator from numpy's global stream (the
        crops and flips from `generator`, torch's stream: the two do not interleave); with roi_masking they go through
        roi_mask on the device."""
        _require_hip(images_u8, "images")
        img = simmim_images(images_u8, self.image_size, generator)
        draws = np.stack([self.mask_generator() for _ in range(img.shape[0])]).astype(np.int64)
        mask = torch.from_numpy(draws).to(img.device)
        if self.roi_masking:
            mask = roi_mask(img, mask)[0]
        return img, mask
