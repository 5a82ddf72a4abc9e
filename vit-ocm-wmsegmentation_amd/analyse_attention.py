"""The region-query path of the reference's analyse_attention.py (--region_query, :183-223) as a batched device pipeline:
Yen mask of the image -> remove_small_objects / binary_closing / label -> region centroids -> one query token per centroid
-> attention rows of the last block at those tokens -> head mean per query, mean over the queries -> [median filter] ->
down / up resize -> threshold() masks. The reference runs it one image at a time with skimage on the host and one
compute_attention call per query; here the masks of a batch are labelled together, ONE forward returns the rows of every
image's query tokens, and only the query points (a few floats per image) and the final masks leave the GPU.
"""
import numpy as np
import torch

from . import _lib
from .engine import _p, _require_hip, _stream
from .eval import _upsample
from .utils import (binary_closing, image_to_gray_u8, label_regions, region_centroids, region_query_index,
                    remove_small_objects, skimage_yen_from_hist, threshold)


def region_query_points(images, patch_size=8):
    """images: (B,C,S,S) float32 on the HIP device (C in {1,3}); patch_size: the encoder's (the reference's default, 8).
    For every image: yen_threshold -> morphology_cleaning (analyse_attention.py:184-185), batched. Returns (points, tokens): per image the list of (x0, y0) = (centroid column,
    centroid row) float pairs in label order, and the list of their query tokens int(x0 // p * w_featmap + y0 // p) —
    x0 first, as analyse_attention.py:192 writes it."""
    _require_hip(images, "images")
    if images.dim() != 4 or images.dtype != torch.float32 or images.shape[-1] != images.shape[-2]:
        raise ValueError(f"expected float32 (B,C,S,S) images, got {images.dtype} {tuple(images.shape)}")
    B, S = images.shape[0], images.shape[-1]
    lib = _lib.load()
    grays, hists = zip(*(image_to_gray_u8(images[b]) for b in range(B)))
    levels = [skimage_yen_from_hist(h) for h in torch.stack(hists).cpu().numpy()]
    masks = torch.empty((B, S, S), dtype=torch.uint8, device=images.device)
    with torch.cuda.device(images.device):
        for b in range(B):
            _lib.check(lib.ocm_op_mask_ge_u8(_p(grays[b]), _p(masks[b]), S * S, levels[b], _stream()))
    labels, counts = label_regions(binary_closing(remove_small_objects(masks.view(torch.bool), 20)))
    points = region_centroids(labels, counts)
    w_featmap = S // patch_size
    tokens = [[region_query_index(x0, y0, patch_size, w_featmap) for x0, y0 in pts] for pts in points]
    return points, tokens


def query_mean(rows, selections):
    """rows: (T,H,R,P) fp32 attention rows; selections: per tile the list of row indices (into R, duplicates allowed) whose
    head-mean maps are averaged in that order (ocm_op_query_mean). Returns (T,P) fp32; NaN where a selection is empty."""
    _require_hip(rows, "rows")
    if rows.dim() != 4 or rows.dtype != torch.float32 or len(selections) != rows.shape[0]:
        raise ValueError(f"expected float32 (T,H,R,P) rows and one selection per tile, got {rows.dtype} {tuple(rows.shape)}")
    rows = rows.contiguous()
    T, H, R, P = rows.shape
    offsets = np.zeros(T + 1, np.int32)
    offsets[1:] = np.cumsum([len(s) for s in selections])
    flat = np.array([q for s in selections for q in s], np.int32)
    if flat.size and (flat.min() < 0 or flat.max() >= R):
        raise ValueError(f"selection index outside [0, {R})")
    sel = torch.from_numpy(np.concatenate([flat, np.zeros(1, np.int32)])).to(rows.device)  # never an empty allocation
    off = torch.from_numpy(offsets).to(rows.device)
    maps = torch.empty((T, P), dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(_lib.load().ocm_op_query_mean(_p(rows), _p(sel), _p(off), _p(maps), T, H, R, P, int(flat.size), _stream()))
    return maps


@torch.no_grad()
def region_queried_attention(model, images, median_filter=1):
    """analyse_attention.py:183-223 for a (B,C,S,S) batch: the region-queried average attention map of every image and
    its threshold() masks. One forward computes the last block's attention rows at the sorted union of all images'
    query tokens (the token number is used as the row index unchanged, as the reference does); per image the rows of its
    own tokens are head-averaged and averaged over the queries in label order, then median-filtered (size
    `median_filter`), resized down by the patch size and bilinearly up to (S,S) like eval.py's maps.
    Returns (masks (B,3,S,S) uint8 — threshold()'s (th, th2, th3) —, maps (B,S,S) fp32, n_points: list of B ints). An image
    without query points (the reference prints "No query points found." and skips the threshold) has n_points 0, a NaN
    map and zero masks."""
    if not 1 <= int(median_filter) <= 15:
        raise ValueError("median_filter must be in 1..15")
    p = model.patch_embed.patch_size
    points, tokens = region_query_points(images, p)
    B, S = images.shape[0], images.shape[-1]
    hf = wf = S // p
    dev = images.device
    n_points = [len(t) for t in tokens]
    masks = torch.zeros((B, 3, S, S), dtype=torch.uint8, device=dev)
    maps = torch.full((B, S, S), float("nan"), dtype=torch.float32, device=dev)
    union = sorted({q for t in tokens for q in t})
    if not union:
        return masks, maps, n_points
    rows = model.get_last_attention_rows(images, query_rows=torch.tensor(union, dtype=torch.int32, device=dev))
    where = {q: i for i, q in enumerate(union)}
    small = query_mean(rows, [[where[q] for q in t] for t in tokens]).reshape(B, hf, wf)
    k = int(median_filter)
    if k != 1:  # on the nearest-upsampled (S,S) map, like eval._head_mean_small
        lib = _lib.load()
        with torch.cuda.device(dev):
            up = torch.empty((B, hf * p, wf * p), dtype=torch.float32, device=dev)
            _lib.check(lib.ocm_op_nearest_upsample(_p(small), _p(up), B, hf, wf, p, _stream()))
            filt = torch.empty_like(up)
            _lib.check(lib.ocm_op_median_filter(_p(up), _p(filt), B, hf * p, wf * p, k, _stream()))
            _lib.check(lib.ocm_op_downscale_centre(_p(filt), _p(small), B, hf * p, wf * p, p, _stream()))
    big = _upsample(small, p)
    for b in range(B):
        if n_points[b]:
            maps[b] = big[b]
            masks[b] = torch.stack(threshold(images[b], big[b], as_numpy=False))
    return masks, maps, n_points
