"""The per-image body of the reference's eval.py `validate` loop (eval.py:126-177) as a batched device pipeline:
ViT forward -> CLS-row attention of the last block -> head mean -> [median filter] -> [tiling of the crops] -> down /
up resize to the image size -> threshold() masks. The reference runs it one image (and, with --crop 4 / 16, one
crop) at a time at B = 1 with the maps going through numpy / scipy / cv2 on the host; here every image and crop of the
batch goes through ONE forward and only the final masks leave the GPU.
"""
import numpy as np
import torch

from . import _lib, utils
from .engine import _p, _stream
from .utils import (SCORE_NAMES, chan_vese_level_set, chan_vese_result_u8, image_to_gray_u8, kmeans_feature_labels, kmeans_pixels,
                    mask_scores, threshold)

METHODS = {"ours": 0, "otsu": 1, "heatmap_threshold": 2}  # index into threshold()'s (th, th2, th3)
KMEANS_FEATURE = "k-means_feature_clustering"
CHAN_VESE = ("chan-vese", "chan-vese_ours")  # chan_vese_segment
KMEANS_PIXELS = ("k-means", "k-means_ours")  # kmeans_pixels_segment


def _head_mean_small(model, tiles, median_filter):
    """(T,C,s,s) tiles -> (T, s/p, s/p) fp32: compute_attention(query 0) -> np.mean over heads -> scipy
    median_filter(size) -> cv2.resize down by p (eval.py:136-144,169). The median runs on the nearest-upsampled
    (T,s,s) map like the reference's; for size 1 (the default) that chain is the identity on the s/p x s/p map."""
    rows = model.get_last_attention_rows(tiles)  # (T, heads, 1, hf*wf) = attentions[0][:, :, 0, 1:]
    T, Hh, nr, P = rows.shape
    p = model.patch_embed.patch_size
    hf = wf = tiles.shape[-1] // p
    lib = _lib.load()
    small = torch.empty((T, hf, wf), dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(lib.ocm_op_head_mean(_p(rows), _p(small), T, Hh, nr, P, _stream()))
        k = int(median_filter)
        if k != 1:
            up = torch.empty((T, hf * p, wf * p), dtype=torch.float32, device=rows.device)  # nearest x p: index replication
            _lib.check(lib.ocm_op_nearest_upsample(_p(small), _p(up), T, hf, wf, p, _stream()))
            filt = torch.empty_like(up)
            _lib.check(lib.ocm_op_median_filter(_p(up), _p(filt), T, hf * p, wf * p, k, _stream()))
            _lib.check(lib.ocm_op_downscale_centre(_p(filt), _p(small), T, hf * p, wf * p, p, _stream()))
    return small


def _upsample(small, p):
    T, h, w = small.shape
    big = torch.empty((T, h * p, w * p), dtype=torch.float32, device=small.device)
    with torch.cuda.device(small.device):
        _lib.check(_lib.load().ocm_op_bilinear_upsample(_p(small.contiguous()), _p(big), T, h, w, p, _stream()))
    return big


@torch.no_grad()
def average_attention_maps(model, images, median_filter=1):
    """images: (B,C,S,S) float32 on the HIP device — or (B,crops,C,s,s) for the reference's --crop 4 / 16 datasets
    (eval.py:146-167: every crop through the model, the maps tiled by utils.concat_crops). Returns (B,S,S) fp32:
    eval.py:136-171 per image — compute_attention(query=0) -> np.mean over heads -> median_filter -> [tile] -> resize
    down by p -> cv2 INTER_LINEAR up to (S,S)."""
    p = model.patch_embed.patch_size
    if images.dim() == 5:
        B, n, Cc, s, s2 = images.shape
        r = int(round(n ** 0.5))
        if r * r != n or s != s2:
            raise ValueError("the crop path tiles a square grid of square crops (utils.concat_crops)")
        small = _head_mean_small(model, images.reshape(B * n, Cc, s, s), median_filter)  # ONE forward for all crops
        hs = small.shape[-1]
        small = small.reshape(B, r, r, hs, hs).permute(0, 1, 3, 2, 4).reshape(B, r * hs, r * hs)  # concat_crops
        return _upsample(small, p)
    if images.dim() != 4 or images.shape[-1] != images.shape[-2]:
        raise ValueError("eval's resize to (img.shape[-1], img.shape[-1]) assumes square images")
    return _upsample(_head_mean_small(model, images, median_filter), p)


def tile_crops_image(images):
    """eval.py:160-166: img = concat_crops(images[i, :, 0, :, :]) replicated to three planes — the (B,1,S,S) image the
    crop path thresholds (plane 0 of every crop, tiled)."""
    B, n, _, s, _ = images.shape
    r = int(round(n ** 0.5))
    return images[:, :, 0].reshape(B, r, r, s, s).permute(0, 1, 3, 2, 4).reshape(B, 1, r * s, r * s).contiguous()


@torch.no_grad()
def segment_images(model, images, method="ours", median_filter=1, as_numpy=False):
    """The mask eval.py scores for `method` in {"ours", "otsu", "heatmap_threshold"} for every image of a batch
    ((B,C,S,S), or (B,crops,C,s,s) for --crop 4 / 16), with --median_filter `median_filter`.
    With method "k-means_feature_clustering" (eval.py:185-202, (B,C,S,S) only) the mask is kmeans_feature's clustering
    of the last block's keys, upsampled to S x S, image by image (see kmeans_segment).
    Returns (masks (B,S,S) uint8 in {0,255}, average_attentions (B,S,S) fp32)."""
    if method not in METHODS and method != KMEANS_FEATURE:
        raise ValueError(f"method {method!r} is not on this path (k-means / chan-vese stay on the host in the reference; "
                         "chan_vese_segment runs the chan-vese methods on the device, kmeans_pixels_segment the k-means ones)")
    if not 1 <= int(median_filter) <= 15:
        raise ValueError("median_filter must be in 1..15")
    if method == KMEANS_FEATURE:
        if images.dim() != 4:
            raise ValueError("k-means_feature_clustering clusters whole images: the crop path (5-D input) is not supported")
        masks = kmeans_segment(model, images)
        maps = average_attention_maps(model, images, median_filter)
        return (masks.cpu().numpy(), maps.cpu().numpy()) if as_numpy else (masks, maps)
    maps = average_attention_maps(model, images, median_filter)
    gray_src = tile_crops_image(images) if images.dim() == 5 else images
    masks = torch.empty(maps.shape, dtype=torch.uint8, device=maps.device)
    for b in range(images.shape[0]):
        masks[b] = threshold(gray_src[b], maps[b], as_numpy=False)[METHODS[method]]
    return (masks.cpu().numpy(), maps.cpu().numpy()) if as_numpy else (masks, maps)


@torch.no_grad()
def kmeans_segment(model, images):
    """eval.py:185-202 for every image of a (B,C,S,S) batch: the keys of the last block (qkv of one forward, channel order
    (head, hd), CLS dropped) bilinearly upsampled to S x S on the device, then utils.kmeans_feature's z-score and
    KMeans(n_clusters=2, n_init=10, random_state=0), one image at a time as the reference does. The (S*S, D) feature
    matrix is allocated once and reused across the batch; it never leaves the device. Returns (B,S,S) uint8 {0, 255}."""
    from .cluster import key_features
    if images.dim() != 4 or images.shape[-1] != images.shape[-2]:
        raise ValueError("k-means_feature_clustering needs square (B,C,S,S) images")
    p = model.patch_embed.patch_size
    S = images.shape[-1]
    if images.shape[-2] % p or S % p:
        raise ValueError(f"image size {tuple(images.shape[-2:])} is not a multiple of the patch size {p}")
    qkv = model._run(images, flags=_lib.OCM_OUT_QKV, n_last=1)["qkv"][0]  # (3, B, H, N, hd)
    X = None
    masks = torch.empty((images.shape[0], S, S), dtype=torch.uint8, device=images.device)
    for b in range(images.shape[0]):
        X = key_features(qkv, b, S, out=X)
        labels = kmeans_feature_labels(X)["labels"]
        masks[b] = torch.from_numpy((labels.reshape(S, S) * 255).astype(np.uint8)).to(images.device)
    return masks


@torch.no_grad()
def chan_vese_segment(model, images, method="chan-vese_ours", median_filter=1, as_numpy=False):
    """The mask eval.py scores for `method` in {"chan-vese", "chan-vese_ours"} (eval.py:182-185, utils.py:199-225) for every
    image of a batch ((B,C,S,S), or (B,crops,C,s,s) for --crop 4 / 16): average_attention_maps once, the gray uint8 image and
    its attention-weighted version per image, then ONE ocm_op_chan_vese call for all 2 B level sets (as the reference computes
    both whichever method is asked for). Only the final masks leave the device.
    Returns (masks (B,S,S) uint8 in {0,255}, average_attentions (B,S,S) fp32)."""
    if method not in CHAN_VESE:
        raise ValueError(f"method {method!r}: chan_vese_segment runs {CHAN_VESE}")
    if not 1 <= int(median_filter) <= 15:
        raise ValueError("median_filter must be in 1..15")
    maps = average_attention_maps(model, images, median_filter)
    gray_src = tile_crops_image(images) if images.dim() == 5 else images
    gray = torch.stack([image_to_gray_u8(gray_src[b])[0] for b in range(gray_src.shape[0])])
    if tuple(gray.shape) != tuple(maps.shape):
        raise ValueError(f"images {tuple(gray.shape)} and attention maps {tuple(maps.shape)} differ in size")
    both = torch.cat([chan_vese_result_u8(gray, maps), gray])  # [0, B): "chan-vese_ours", [B, 2B): "chan-vese"
    B = gray.shape[0]
    masks = chan_vese_level_set(both)[0].view(torch.uint8) * 255
    masks = masks[:B] if method == "chan-vese_ours" else masks[B:]
    return (masks.cpu().numpy(), maps.cpu().numpy()) if as_numpy else (masks.contiguous(), maps)


def _image_side(images):
    """(H, W) of the image a batch is segmented at: the images' own, or the tiled crops'."""
    if images.dim() == 5:
        r = int(round(images.shape[1] ** 0.5))
        return r * images.shape[-2], r * images.shape[-1]
    return images.shape[-2], images.shape[-1]


@torch.no_grad()
def kmeans_pixels_segment(model, images, method="k-means_ours", median_filter=1, as_numpy=False, rng_state=None):
    """The mask eval.py scores for `method` in {"k-means", "k-means_ours"} (eval.py:178-181, utils.py:118-169) for every image
    of a batch ((B,C,S,S), or (B,crops,C,s,s) for --crop 4 / 16): average_attention_maps once, the gray uint8 image and its
    attention-weighted version per image, then ONE ocm_op_kmeans_px call for all 2 B problems, interleaved ours_0, image_0,
    ours_1, ... — the reference computes both whichever method is asked for, "ours" first, and that fixes the order of
    cv::RNG's draws. rng_state: the generator state the 2 B * 60 draws start from; None chains utils' module-level state, as
    OpenCV's thread-local generator runs on from image to image. An image whose pixel count is no multiple of 3 raises
    ValueError before the model is touched (numpy's reshape(-1, 3) raises there). Only the final masks leave the device.
    Returns (masks (B,S,S) uint8 in {0,255}, average_attentions (B,S,S) fp32)."""
    if method not in KMEANS_PIXELS:
        raise ValueError(f"method {method!r}: kmeans_pixels_segment runs {KMEANS_PIXELS}")
    if not 1 <= int(median_filter) <= 15:
        raise ValueError("median_filter must be in 1..15")
    if images.dim() not in (4, 5):
        raise ValueError(f"expected (B,C,S,S) images or (B,crops,C,s,s) crops, got {tuple(images.shape)}")
    H, W = _image_side(images)
    if (H * W) % 3:
        raise ValueError(f"cannot reshape {H} x {W} pixels into triples (numpy's reshape(-1, 3) raises as well)")
    maps = average_attention_maps(model, images, median_filter)
    gray_src = tile_crops_image(images) if images.dim() == 5 else images
    gray = torch.stack([image_to_gray_u8(gray_src[b])[0] for b in range(gray_src.shape[0])])
    if tuple(gray.shape) != tuple(maps.shape):
        raise ValueError(f"images {tuple(gray.shape)} and attention maps {tuple(maps.shape)} differ in size")
    B = gray.shape[0]
    both = torch.stack([chan_vese_result_u8(gray, maps), gray], dim=1).reshape((2 * B,) + tuple(gray.shape[1:]))
    r = kmeans_pixels(both, rng_state=utils._cv_rng_state if rng_state is None else rng_state)
    if rng_state is None:
        utils._cv_rng_state = r["rng_state"]
    masks = r["mask"].reshape((B, 2) + tuple(gray.shape[1:]))[:, 0 if method == "k-means_ours" else 1]
    return (masks.cpu().numpy(), maps.cpu().numpy()) if as_numpy else (masks.contiguous(), maps)


def _segmenter(method):
    return chan_vese_segment if method in CHAN_VESE else kmeans_pixels_segment if method in KMEANS_PIXELS else segment_images


@torch.no_grad()
def score_images(model, images, targets, method="ours", median_filter=1):
    """eval.py:126-221 for a batch: the mask of `method` (segment_images, chan_vese_segment for the chan-vese methods,
    kmeans_pixels_segment for the cv2.kmeans methods "k-means" / "k-means_ours", which chain utils' cv::RNG state from batch to
    batch) scored against `targets` ((B,S,S) or (B,1,S,S), any float, uint8 or bool dtype, classes > 0.5) by utils.mask_scores:
    the uint8 mask stands for output / 255.
    Returns (scores (B,7) float64 in utils.SCORE_NAMES order, masks (B,S,S) uint8, maps (B,S,S) fp32), all on the device: the
    scoring adds no copy and no host synchronisation to the segmentation, and only what the caller reads leaves the device."""
    masks, maps = _segmenter(method)(model, images, method=method, median_filter=median_filter)
    B, S = masks.shape[0], masks.shape[-1]
    if tuple(targets.shape) not in ((B, S, S), (B, 1, S, S)):
        raise ValueError(f"targets {tuple(targets.shape)}: expected {(B, S, S)} or {(B, 1, S, S)} for these images")
    return mask_scores(masks, targets)[0], masks, maps


@torch.no_grad()
def validate(model, batches, method="ours", median_filter=1):
    """eval.py's validate loop (:106-283) over an iterable of (images, targets) batches: every image scored by score_images,
    the sums of the scores kept on the device and read once at the end (the only host synchronisation the scores cost).
    Returns (acc_avg, f1_avg, loss_avg, means): the reference's three averages over all images, and a dict with the mean of each
    of utils.SCORE_NAMES, "images" (their number) and "auc_nan_images" — the ROC-AUC is undefined for a target with one class
    only; such images are left out of its mean (NaN when none is left) and counted here."""
    sums = n_nan = None
    n = 0
    for images, targets in batches:
        scores = score_images(model, images, targets, method, median_filter)[0]
        nan = torch.isnan(scores[:, 5])
        scores[:, 5] = torch.where(nan, torch.zeros_like(scores[:, 5]), scores[:, 5])
        sums = scores.sum(0) if sums is None else sums + scores.sum(0)
        n_nan = nan.sum() if n_nan is None else n_nan + nan.sum()
        n += scores.shape[0]
    if n == 0:
        raise ValueError("validate: no batches")
    host = torch.cat([sums, n_nan.to(torch.float64).reshape(1)]).cpu().numpy()
    nan_images = int(host[7])
    means = {name: float(host[k]) / n for k, name in enumerate(SCORE_NAMES)}
    means["auc"] = float(host[5]) / (n - nan_images) if n > nan_images else float("nan")
    means["images"], means["auc_nan_images"] = n, nan_images
    return means["accuracy"], means["f1"], means["dice_loss"], means
