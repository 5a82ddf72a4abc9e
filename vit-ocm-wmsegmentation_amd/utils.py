"""Output contract of the attention map: the hot-path part of the reference's utils.py and the
region-query index of analyse_attention.py, on device.

  compute_attention   reference utils.py:229-235
  region_query_index  reference analyse_attention.py:192-195, 234-236
  threshold           reference utils.py:55-115 (the three Otsu masks of eval.py's "ours" / "otsu" /
                      "heatmap_threshold" methods), on device
  kmeans_feature      reference utils.py:171-197 (eval.py's "k-means_feature_clustering"), clustered on device
  DiceLoss            reference utils.py:410-424 (finetune.py's loss), forward and backward on device
  yen_threshold, get_ROIs, morphology_cleaning
                      reference utils.py:237-281: the Yen mask, its clean-up (remove_small_objects -> binary_closing ->
                      label) and the region centroids that analyse_attention.py --region_query queries, on device
                      (kernels_morph.hip); label_regions / region_stats / remove_small_objects / binary_closing are
                      the skimage pieces they are made of
  chan_vese, chan_vese_level_set
                      reference utils.py:199-225 (eval.py's "chan-vese" / "chan-vese_ours"): skimage.segmentation.chan_vese
                      with the checkerboard start, every level set of a batch evolved on device (kernels_levelset.hip)
  kmeans, kmeans_pixels, cv_rng_uniform
                      reference utils.py:118-169 (eval.py's "k-means" / "k-means_ours"): cv2.kmeans on the pixel triples with
                      cv::RNG's random centres, and the Otsu mask of the painting, every problem of a batch on device
                      (kernels_kmeans_px.hip)
  mask_scores, calculate_metrics
                      reference utils.py:388-408 (the five sklearn scores of eval.py's table), the ROC-AUC that PGT.py:247-275
                      and finetune.py:209 add, and the per-image DiceLoss of eval.py:211, for a batch in one pass on device
                      (kernels_score.hip)
  pil_resize, ResamplePlan, resample_table
                      PIL.Image.resize / Image.crop(...).resize / ToTensor of uint8 images (sw_processing.py:217-231,
                      analyse_attention.py:102-120, data.py's transforms), byte for byte, for a batch in one call on device
                      (kernels_resample.hip); the transforms themselves are in data.py
  pil_color, pil_gaussian_blur, gaussian_blur_table
                      ImageEnhance.{Brightness, Contrast, Color}, the convert('HSV') round trip of adjust_hue, convert('L'),
                      ImageOps.solarize, ImageFilter.GaussianBlur and ToTensor + Normalize of uint8 RGB batches, byte for byte,
                      every image with its own parameters (kernels_augment.hip); DINO's transform itself is in dino/utils.py
  clip_grad_norm_, grad_norm, get_grad_norm
                      torch.nn.utils.clip_grad_norm_ (mim.py, train.py) and reference utils.py:363-373, the 2-norm of every
                      gradient in one multi-tensor pass with float64 sums and the scaling by a coefficient that never leaves
                      the device (kernels_optim.hip); the optimizers themselves are in optimizer.py
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .engine import _p, _require_hip, _stream, _ws
from .optimizer import _check_tensor, _table


def compute_attention(attentions, query, w_featmap, h_featmap, patch_size):
    """attentions: list whose first entry is the (B, H, N, N) fp32 attention of the last block
    (what get_intermediate_feat returns). Returns (maps, nh) with maps a numpy array
    (nh, w_featmap*p, h_featmap*p): row `query` of batch element 0 with the CLS column dropped,
    reshaped (w_featmap, h_featmap) row-major and nearest-neighbour upsampled by patch_size.
    The gather + upsample is one HIP kernel (ocm_op_attention_map); the D2H copy is the only
    device->host transfer of the inference path, as in the reference."""
    attn = attentions[0]
    _require_hip(attn, "attentions[0]")
    if attn.dim() != 4 or attn.dtype != torch.float32:
        raise ValueError(f"expected a float32 (B, H, N, N) tensor, got {attn.dtype} {tuple(attn.shape)}")
    attn = attn.contiguous()
    nh, n = attn.shape[1], attn.shape[2]
    query = int(query)
    maps = torch.empty((nh, w_featmap * patch_size, h_featmap * patch_size), dtype=torch.float32, device=attn.device)
    with torch.cuda.device(attn.device):
        _lib.check(_lib.load().ocm_op_attention_map(_p(attn), _p(maps), 0, nh, n, query, w_featmap, h_featmap,
                                                    patch_size, _stream()))
    return maps.cpu().numpy(), nh


def region_query_index(py, px, patch_size, w_featmap):
    """Token index (CLS excluded, i.e. the value passed as `query` minus nothing: the reference
    indexes attentions[..., query, 1:] with this number directly) of the patch containing pixel
    (py, px): int(py // p * w_featmap + px // p)  — analyse_attention.py:192. Pure integer math."""
    return int(py // patch_size * w_featmap + px // patch_size)


def grid_query_index(i, j, w_featmap, rate):
    """analyse_attention.py:234: query of grid cell (i, j) at sub-sampling `rate`."""
    return int(i * w_featmap * rate + j * rate)


def _otsu_from_hist(hist_dev, count):
    """256-bin device histogram -> OpenCV-style Otsu level (a 256-step scalar loop: done on the host)."""
    h = hist_dev.cpu().numpy().astype(np.uint64)
    level = int(_lib.load().ocm_otsu_threshold(h.ctypes.data_as(C.POINTER(C.c_uint64)), int(count)))
    if level < 0:
        raise ValueError("ocm_otsu_threshold failed")
    return level


def skimage_otsu_from_hist(hist_dev):
    """skimage.filters.threshold_otsu (0.19.3, sw_processing.py:57) from a 256-bin device histogram of a uint8 image:
    integer bins over [min, max], float64 class weights / means, first maximum of the between-class variance
    (a 256-step scalar computation: on the host, like the reference). scikit-image is not installable here:
    restated from its source, parity unpinned."""
    h = hist_dev.cpu().numpy().astype(np.float64)
    nz = np.nonzero(h)[0]
    if nz.size == 0:
        raise ValueError("empty histogram")
    lo, hi = int(nz[0]), int(nz[-1])
    if lo == hi:
        return lo
    counts, centers = h[lo:hi + 1], np.arange(lo, hi + 1)
    weight1 = np.cumsum(counts)
    weight2 = np.cumsum(counts[::-1])[::-1]
    mean1 = np.cumsum(counts * centers) / weight1
    mean2 = (np.cumsum((counts * centers)[::-1]) / weight2[::-1])[::-1]
    variance12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    return int(centers[int(np.argmax(variance12))])


def skimage_yen_from_hist(hist_dev):
    """skimage.filters.threshold_yen (0.19.3, reference utils.py:241) from a 256-bin device histogram of a uint8 image:
    integer bins over [min, max], pmf = counts / total, P1 = cumsum(pmf), P1_sq = cumsum(pmf^2), P2_sq = reversed
    cumsum of pmf^2, crit = log((P1_sq[:-1] * P2_sq[1:])^-1 * (P1[:-1] * (1 - P1[:-1]))^2), the bin at its first
    maximum; a constant image returns its value. Evaluated in float64 on the host (a 256-step scalar computation, like
    the reference). scikit-image is not installable here: restated from its source, parity unpinned."""
    h = hist_dev.cpu().numpy().astype(np.float64) if isinstance(hist_dev, torch.Tensor) else np.asarray(hist_dev, np.float64)
    nz = np.nonzero(h)[0]
    if nz.size == 0:
        raise ValueError("empty histogram")
    lo, hi = int(nz[0]), int(nz[-1])
    if lo == hi:
        return lo
    pmf = h[lo:hi + 1] / h[lo:hi + 1].sum()
    P1 = np.cumsum(pmf)
    P1_sq = np.cumsum(pmf ** 2)
    P2_sq = np.cumsum(pmf[::-1] ** 2)[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        crit = np.log(((P1_sq[:-1] * P2_sq[1:]) ** -1) * (P1[:-1] * (1.0 - P1[:-1])) ** 2)
    return lo + int(np.argmax(crit))


def histogram_u8(img_u8):
    """256-bin int64 histogram of a uint8 HIP tensor (ocm_op_histogram_u8)."""
    _require_hip(img_u8, "img")
    img_u8 = img_u8.contiguous()
    hist = torch.empty(256, dtype=torch.int64, device=img_u8.device)
    with torch.cuda.device(img_u8.device):
        _lib.check(_lib.load().ocm_op_histogram_u8(_p(img_u8), img_u8.numel(), _p(hist), _stream()))
    return hist


def image_to_gray_u8(img):
    """transform(img.squeeze(0)).convert("L") of eval.py:166 on device: (C,H,W) or (1,C,H,W) float tensor in
    [0,1] with C in {1,3} -> ((H,W) uint8 tensor, 256-bin int64 histogram)."""
    _require_hip(img, "img")
    if img.dim() == 4:
        img = img[0]
    if img.dim() != 3 or img.shape[0] not in (1, 3) or img.dtype != torch.float32:
        raise ValueError(f"expected a float32 (C,H,W) tensor with C in (1,3), got {img.dtype} {tuple(img.shape)}")
    if img.stride(2) != 1 or img.stride(1) != img.shape[2]:
        img = img.contiguous()
    out = torch.empty(img.shape[1:], dtype=torch.uint8, device=img.device)
    hist = torch.empty(256, dtype=torch.int64, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().ocm_op_image_to_gray_u8(_p(img), int(img.stride(0)), int(img.shape[0]), out.numel(),
                                                       _p(out), _p(hist), _stream()))
    return out, hist


def threshold(img, attention, output_directory="", save=False, name=None, as_numpy=True, return_levels=False):
    """utils.py:61-115 on device. img: the float (C,H,W) image tensor (what the reference turns into a PIL "L"
    image first) or an (H,W) uint8 tensor; attention: (H,W) float32 heat map. Returns (th, th2, th3):
    Otsu mask of the 0.6/0.4 image/attention blend, of the image, and of the attention — numpy uint8 arrays as
    the reference returns them (as_numpy=False keeps them on the device). Saving figures (save=True) is
    the reference's matplotlib side effect and is not part of this path."""
    if save:
        raise NotImplementedError("threshold(save=True) writes figures with matplotlib in the reference; not on this path")
    _require_hip(attention, "attention")
    if attention.dtype != torch.float32 or attention.dim() != 2:
        raise ValueError(f"expected a float32 (H,W) attention map, got {attention.dtype} {tuple(attention.shape)}")
    attention = attention.contiguous()
    lib, dev, n = _lib.load(), attention.device, attention.numel()
    if img.dtype == torch.uint8:
        _require_hip(img, "img")
        img_u8 = img.contiguous()
        hist_img = histogram_u8(img_u8)
    else:
        img_u8, hist_img = image_to_gray_u8(img)
    if tuple(img_u8.shape) != tuple(attention.shape):
        raise ValueError(f"image {tuple(img_u8.shape)} and attention {tuple(attention.shape)} differ in size")
    att_u8 = torch.empty(attention.shape, dtype=torch.uint8, device=dev)
    res_u8 = torch.empty(attention.shape, dtype=torch.uint8, device=dev)
    masks = torch.empty((3,) + tuple(attention.shape), dtype=torch.uint8, device=dev)
    scratch = torch.empty(2048, dtype=torch.uint8, device=dev)
    hist_att = torch.empty(256, dtype=torch.int64, device=dev)
    hist_res = torch.empty(256, dtype=torch.int64, device=dev)
    alpha = 0.4
    with torch.cuda.device(dev):
        st = _stream()
        _lib.check(lib.ocm_op_normalize_u8(_p(attention), n, _p(scratch), _p(att_u8), _p(hist_att), st))
        _lib.check(lib.ocm_op_blend_u8(_p(img_u8), _p(att_u8), n, alpha, 1 - alpha, _p(res_u8), _p(hist_res), st))
        levels = (_otsu_from_hist(hist_res, n), _otsu_from_hist(hist_img, n), _otsu_from_hist(hist_att, n))
        for k, src in enumerate((res_u8, img_u8, att_u8)):
            _lib.check(lib.ocm_op_threshold_u8(_p(src), _p(masks[k]), n, levels[k], st))
    out = tuple(m.cpu().numpy() for m in masks) if as_numpy else tuple(masks)
    return (out + (levels,)) if return_levels else out


def kmeans_feature_labels(X):
    """KMeans(n_clusters=2, n_init=10, random_state=0).fit of the z-scored rows of X, a contiguous fp32 (S*S, D) device
    tensor that is standardised IN PLACE (cluster.fit_two_means on the device backend). Returns the fit's dict."""
    from . import cluster
    return cluster.fit_two_means(cluster.DeviceBackend(X))


def kmeans_feature(img, features, output_directory="", save=False, name=None):
    """utils.py:171-197: z-score every channel of `features` (torch.mean / unbiased torch.std), cluster the rows with
    sklearn's KMeans(n_clusters=2, n_init=10, random_state=0) — replayed on the device by cluster.py — and return the
    labels times 255 as an int32 numpy array (S, S). features: the (1, S, S, D) map eval.py passes (any leading shape
    whose rows are the S*S pixels), on the device or on the host (then it goes to img's device, or the current one); it
    is not modified. img only picks the device: the reference does not use it either.
    The reference reshapes the labels with features.shape[-1] (the channel count), which works only when D == S; here the
    side is S = sqrt(rows). Saving a figure (save=True) is the reference's matplotlib side effect: not on this path."""
    if save:
        raise NotImplementedError("kmeans_feature(save=True) writes a figure with matplotlib in the reference; "
                                  "not on this path")
    if not isinstance(features, torch.Tensor):
        features = torch.as_tensor(np.asarray(features))
    D = features.shape[-1]
    rows = features.numel() // max(D, 1)
    S = int(round(rows ** 0.5))
    if S * S != rows:
        raise ValueError(f"features hold {rows} rows: not a square S x S pixel grid")
    if features.is_cuda:
        dev = features.device
    elif isinstance(img, torch.Tensor) and img.is_cuda:
        dev = img.device
    elif torch.cuda.is_available():
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        _require_hip(features, "features")  # there is no host k-means: the features need a device to go to
    X = features.reshape(rows, D).to(device=dev, dtype=torch.float32, copy=True).contiguous()
    labels = kmeans_feature_labels(X)["labels"]
    return labels.reshape(S, S) * 255


class _DiceLossFn(torch.autograd.Function):
    """loss = 1 - (2 sum(p t) + smooth) / (sum p + sum t + smooth), p = sigmoid(logits): two launches forward (per-workgroup
    partial sums, then their fixed-order sum and the loss, all in device memory), one elementwise launch backward."""

    @staticmethod
    def forward(ctx, logits, targets, smooth):
        lib, dev, n = _lib.load(), logits.device, logits.numel()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        sums = torch.empty(3, dtype=torch.float32, device=dev)
        nbytes = lib.ocm_dice_loss_workspace_bytes(n)
        ws = _ws(nbytes, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ocm_op_dice_loss(_p(logits), _p(targets), _p(loss), _p(sums), n, smooth, _p(ws), nbytes, _stream()))
        ctx.smooth = smooth
        ctx.save_for_backward(logits, targets, sums)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        logits, targets, sums = ctx.saved_tensors
        g = grad_loss.detach().to(device=logits.device, dtype=torch.float32).reshape(1).contiguous()
        dlogits = torch.empty_like(logits)
        with torch.cuda.device(logits.device):
            _lib.check(_lib.load().ocm_op_dice_loss_backward(_p(logits), _p(targets), _p(sums), _p(g), _p(dlogits),
                                                             logits.numel(), ctx.smooth, _stream()))
        return dlogits, None, None


class DiceLoss(nn.Module):
    """utils.py:410-424: sigmoid Dice loss over all elements, forward(inputs, targets, smooth=1) -> 0-dim fp32 tensor,
    differentiable into `inputs` (the gradient arrives in the inputs' own dtype and layout through torch's cast / contiguous
    nodes). Both tensors must live on a HIP device; they are made contiguous fp32 first. Works under torch.no_grad()."""

    def __init__(self):
        super().__init__()

    def forward(self, inputs, targets, smooth=1):
        if isinstance(targets, torch.Tensor) and targets.requires_grad:
            raise NotImplementedError("DiceLoss does not produce the gradient of the targets; pass targets that do not "
                                      "require grad")
        _require_hip(inputs, "inputs")
        _require_hip(targets, "targets")
        if inputs.numel() != targets.numel() or inputs.numel() == 0:
            raise ValueError(f"inputs {tuple(inputs.shape)} and targets {tuple(targets.shape)} must hold the same, non-zero "
                             "number of elements")
        x = inputs.to(torch.float32).contiguous().reshape(-1)
        t = targets.detach().to(device=inputs.device, dtype=torch.float32).contiguous().reshape(-1)
        return _DiceLossFn.apply(x, t, float(smooth))


# ---- the query points of analyse_attention.py --region_query (reference utils.py:237-281) ------------------------------------
DISK2 = ((0, 0, 1, 0, 0), (0, 1, 1, 1, 0), (1, 1, 1, 1, 1), (0, 1, 1, 1, 0), (0, 0, 1, 0, 0))  # skimage.morphology.disk(2)


def footprint_bits(footprint):
    """(size, bits) of a square 0/1 footprint with an odd side <= 7: bit dy * size + dx = footprint[dy][dx]."""
    fp = np.asarray(footprint)
    if fp.ndim != 2 or fp.shape[0] != fp.shape[1] or fp.shape[0] % 2 == 0 or fp.shape[0] > 7:
        raise ValueError(f"footprint must be square with an odd side <= 7, got shape {fp.shape}")
    size = int(fp.shape[0])
    return size, sum(1 << i for i, v in enumerate(fp.reshape(-1)) if v)


def _mask_batch(mask, what="mask"):
    """A bool / uint8 (H,W) or (B,H,W) HIP tensor as a contiguous uint8 (B,H,W) view (nonzero = foreground)."""
    _require_hip(mask, what)
    if mask.dtype not in (torch.bool, torch.uint8) or mask.dim() not in (2, 3):
        raise ValueError(f"expected a bool or uint8 (H,W) or (B,H,W) {what}, got {mask.dtype} {tuple(mask.shape)}")
    m = mask.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    return m.reshape((-1,) + tuple(m.shape[-2:]))


def _like(mask, out_u8):
    """A 0/1 uint8 (B,H,W) result in the shape of `mask`, as bool."""
    return out_u8.view(torch.bool).reshape(mask.shape)


def binary_morph(mask, footprint, op, border_value):
    """scipy.ndimage.binary_dilation (op 0) / binary_erosion (op 1) of a bool mask with a square odd footprint (side <= 7)
    and `border_value` outside the image (ocm_op_binary_morph). Returns a bool tensor of the mask's shape."""
    m = _mask_batch(mask)
    size, bits = footprint_bits(footprint)
    out = torch.empty_like(m)
    B, H, W = m.shape
    with torch.cuda.device(m.device):
        _lib.check(_lib.load().ocm_op_binary_morph(_p(m), _p(out), B, H, W, bits, size, int(op), int(border_value), _stream()))
    return _like(mask, out)


def binary_closing(mask, footprint=DISK2):
    """skimage.morphology.binary_closing (0.19.3): binary_dilation (scipy's default border_value 0), then binary_erosion
    with border_value=True — the image edge does not erode what the dilation grew against it."""
    return binary_morph(binary_morph(mask, footprint, 0, 0), footprint, 1, 1)


def remove_small_objects(mask, min_size=20):
    """skimage.morphology.remove_small_objects(mask, min_size, connectivity=2) of a bool mask: 8-connected components
    with fewer than min_size pixels are cleared (ocm_op_remove_small_objects)."""
    m = _mask_batch(mask)
    B, H, W = m.shape
    lib = _lib.load()
    out = torch.empty_like(m)
    nbytes = lib.ocm_remove_small_objects_workspace_bytes(B, H, W)
    ws = _ws(nbytes, m.device)
    with torch.cuda.device(m.device):
        _lib.check(lib.ocm_op_remove_small_objects(_p(m), _p(out), B, H, W, int(min_size), _p(ws), nbytes, _stream()))
    return _like(mask, out)


def label_regions(mask):
    """skimage.measure.label(mask, connectivity=2, return_num=True) on device for an (H,W) or (B,H,W) bool / uint8 mask:
    (labels int32 of the mask's shape — 0 background, 1..n in raster order of each component's first pixel —, counts:
    an int32 (B,) device tensor, or for an (H,W) mask a 0-dim one)."""
    m = _mask_batch(mask)
    B, H, W = m.shape
    lib = _lib.load()
    labels = torch.empty((B, H, W), dtype=torch.int32, device=m.device)
    counts = torch.empty(B, dtype=torch.int32, device=m.device)
    nbytes = lib.ocm_label8_workspace_bytes(B, H, W)
    ws = _ws(nbytes, m.device)
    with torch.cuda.device(m.device):
        _lib.check(lib.ocm_op_label8(_p(m), _p(labels), _p(counts), B, H, W, _p(ws), nbytes, _stream()))
    return labels.reshape(mask.shape), (counts[0] if mask.dim() == 2 else counts)


def region_stats(labels, max_regions):
    """Exact integer sums of an int32 (H,W) or (B,H,W) label image for the labels 1..max_regions (ocm_op_region_stats):
    dict(area, sum_row, sum_col: int64 (B, max_regions); bbox: int32 (B, max_regions, 4) = (min_row, min_col,
    max_row + 1, max_col + 1)) on the device. regionprops' centroid is (sum_row / area, sum_col / area) in float64."""
    _require_hip(labels, "labels")
    if labels.dtype != torch.int32 or labels.dim() not in (2, 3):
        raise ValueError(f"expected an int32 (H,W) or (B,H,W) label image, got {labels.dtype} {tuple(labels.shape)}")
    lab = labels.contiguous().reshape((-1,) + tuple(labels.shape[-2:]))
    B, H, W = lab.shape
    R = max(int(max_regions), 1)
    sums = torch.empty((3, B, R), dtype=torch.int64, device=lab.device)
    bbox = torch.empty((B, R, 4), dtype=torch.int32, device=lab.device)
    with torch.cuda.device(lab.device):
        _lib.check(_lib.load().ocm_op_region_stats(_p(lab), B, H, W, R, _p(sums[0]), _p(sums[1]), _p(sums[2]), _p(bbox),
                                                   _stream()))
    return dict(area=sums[0], sum_row=sums[1], sum_col=sums[2], bbox=bbox)


def yen_threshold(img, output_directory="", save=False, return_level=False):
    """utils.py:237-248 on device. img: an (H,W) uint8 tensor, or the float (C,H,W) image tensor (turned into the PIL
    "L" image the reference thresholds by image_to_gray_u8). Returns the bool mask `th <= img` with th =
    skimage_yen_from_hist of the image's device histogram (and th itself with return_level=True). Saving the figure
    (save=True) is the reference's matplotlib side effect and is not part of this path."""
    if save:
        raise NotImplementedError("yen_threshold(save=True) writes a figure with matplotlib in the reference; not on this path")
    _require_hip(img, "img")
    if img.dtype == torch.uint8:
        if img.dim() != 2:
            raise ValueError(f"expected an (H,W) uint8 image, got {tuple(img.shape)}")
        img_u8 = img.contiguous()
        hist = histogram_u8(img_u8)
    else:
        img_u8, hist = image_to_gray_u8(img)
    level = skimage_yen_from_hist(hist)
    mask = torch.empty_like(img_u8)
    with torch.cuda.device(img_u8.device):
        _lib.check(_lib.load().ocm_op_mask_ge_u8(_p(img_u8), _p(mask), img_u8.numel(), level, _stream()))
    mask = mask.view(torch.bool)
    return (mask, level) if return_level else mask


def get_ROIs(mask):
    """utils.py:250-254 on device: remove_small_objects(min_size=20, connectivity=2) -> binary_closing(disk(2)) -> label.
    A bool (H,W) or (B,H,W) mask goes through the component-wise chain. A uint8 {0, 255} mask — what data.py:222-224
    passes — gets skimage's integer-input behaviour: remove_small_objects reads the array as a label image, so the white
    class is cleared only when it holds fewer than 20 pixels IN TOTAL, whatever their components. Returns the int32
    label image."""
    _require_hip(mask, "mask")
    if mask.dtype == torch.uint8:
        if mask.dim() != 2:
            raise ValueError(f"a uint8 mask is one (H,W) image, got {tuple(mask.shape)}")
        hist = histogram_u8(mask).cpu().numpy()
        if int(hist[1:255].sum()):
            raise ValueError("a uint8 mask must hold only 0 and 255 (data.py:222-223)")
        if int(hist[255]) < 20:
            return torch.zeros(mask.shape, dtype=torch.int32, device=mask.device)
        cleaned = mask
    else:
        cleaned = remove_small_objects(mask, 20)
    return label_regions(binary_closing(cleaned))[0]


def roi_sample_index(in_size, out_size):
    """The source index of every output cell of skimage.transform.resize(order=0, anti_aliasing=False) along one axis (0.19.3:
    scipy.ndimage.zoom(order=0, mode='mirror', grid_mode=True)), an int32 (out_size,) numpy array, on the host. With z =
    in_size / out_size as a double, idx(i) = clamp(floor(((i + 0.5) * z - 0.5) + 0.5), 0, in_size - 1): the coordinate first,
    then the rounding of order 0, in two steps as scipy takes them — the shorter floor((i + 0.5) * in_size / out_size) lands on
    another pixel for some pairs, (30, 11) and (52, 23) among them."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"roi_sample_index({in_size}, {out_size}): both sizes must be at least 1")
    z = np.float64(in_size) / np.float64(out_size)
    coord = (np.arange(out_size, dtype=np.float64) + 0.5) * z - 0.5
    return np.clip(np.floor(coord + 0.5), 0, in_size - 1).astype(np.int32)


def region_centroids(labels, counts, min_area=10):
    """regionprops of int32 (B,H,W) label images with counts[b] regions each: per image the list of (x0, y0) =
    (centroid column, centroid row) float64 pairs of the regions with area >= min_area, in label order (utils.py:269-281)."""
    counts = [int(c) for c in counts.reshape(-1).cpu().tolist()]
    st = region_stats(labels, max(counts + [1]))
    area, sr, sc = (st[k].cpu().numpy() for k in ("area", "sum_row", "sum_col"))
    points = []
    for b, n in enumerate(counts):
        keep = np.nonzero(area[b, :n] >= min_area)[0]
        a = area[b, keep].astype(np.float64)
        points.append(list(zip((sc[b, keep] / a).tolist(), (sr[b, keep] / a).tolist())))
    return points


def morphology_cleaning(mask, output_directory="", save=False, as_numpy=True):
    """utils.py:256-281 on device: the get_ROIs chain on a bool (H,W) mask, then the (x0, y0) = (centroid column,
    centroid row) points of the regions with area >= 10 in label order — a list of float pairs as the reference returns
    it, or with as_numpy=False a float64 (n, 2) tensor on the mask's device. The centroids are exact integer sums
    divided in float64, which is what regionprops computes. Drawing the boxes (save=True) is the reference's matplotlib
    side effect and is not part of this path."""
    if save:
        raise NotImplementedError("morphology_cleaning(save=True) draws figures with matplotlib in the reference; "
                                  "not on this path")
    _require_hip(mask, "mask")
    if mask.dtype != torch.bool or mask.dim() != 2:
        raise ValueError(f"expected a bool (H,W) mask, got {mask.dtype} {tuple(mask.shape)}")
    labels, count = label_regions(binary_closing(remove_small_objects(mask, 20)))
    points = region_centroids(labels[None], count.reshape(1))[0]
    if as_numpy:
        return points
    return torch.tensor(points, dtype=torch.float64, device=mask.device).reshape(-1, 2)


# ---- Chan-Vese (reference utils.py:199-225; skimage.segmentation.chan_vese 0.19.x) -------------------------------------------
def chan_vese_checkerboard(h, w, square_size=5):
    """skimage's _cv_checkerboard: sin(pi / square_size * y)[:, None] * sin(pi / square_size * x)[None, :] in float64, computed
    with numpy on the host so that the start holds numpy's own bits. Returns an (h, w) numpy array."""
    sf = np.pi / square_size
    yv = np.arange(h, dtype=np.float64).reshape(h, 1) * sf
    xv = np.arange(w, dtype=np.float64) * sf
    return np.sin(yv) * np.sin(xv)


def chan_vese_normalize(images_u8):
    """skimage's preparation of a uint8 image, per image of a (B,H,W) batch, in float64: img - min, then / max of the result
    when that is not 0 (a constant image stays all zero). Torch's float64 subtraction and division are IEEE: numpy's bits."""
    img = images_u8.to(torch.float64)
    img = img - img.amin(dim=(1, 2), keepdim=True)
    mx = img.amax(dim=(1, 2), keepdim=True)
    return (img / torch.where(mx != 0, mx, torch.ones_like(mx))).contiguous()


def chan_vese_level_set(images_u8, mu=0.25, lambda1=1.0, lambda2=1.0, tol=1e-3, max_num_iter=200, dt=0.5,
                        init_level_set="checkerboard", return_phi=False):
    """skimage.segmentation.chan_vese(image, mu, lambda1, lambda2, tol, max_num_iter, dt, init_level_set)[0] for an (H,W) or
    (B,H,W) uint8 HIP tensor: every image is normalised as skimage does, all level sets evolve in one ocm_op_chan_vese call
    (float64, one launch per iteration, each image stopping on its own) and nothing is synchronised with the host.
    init_level_set: "checkerboard", or a float64 tensor of the images' shape (or (H,W), used for every image) taken as given.
    Returns (mask bool, iters int32) — (H,W) and 0-dim for an (H,W) image, (B,H,W) and (B,) for a batch — and the final
    float64 level set as a third element with return_phi=True."""
    _require_hip(images_u8, "images")
    if images_u8.dtype != torch.uint8 or images_u8.dim() not in (2, 3):
        raise ValueError(f"expected a uint8 (H,W) or (B,H,W) image tensor, got {images_u8.dtype} {tuple(images_u8.shape)}")
    x = images_u8.contiguous().reshape((-1,) + tuple(images_u8.shape[-2:]))
    B, H, W = x.shape
    dev = x.device
    if isinstance(init_level_set, str):
        if init_level_set != "checkerboard":
            raise ValueError(f"init_level_set {init_level_set!r}: only \"checkerboard\" or a float64 tensor")
        phi = torch.from_numpy(chan_vese_checkerboard(H, W)).to(dev).expand(B, H, W).contiguous()
    else:
        _require_hip(init_level_set, "init_level_set")
        if init_level_set.dtype != torch.float64 or tuple(init_level_set.shape) not in ((H, W), tuple(images_u8.shape), (B, H, W)):
            raise ValueError(f"init_level_set must be a float64 tensor of shape {(H, W)} or {tuple(images_u8.shape)}, got "
                             f"{init_level_set.dtype} {tuple(init_level_set.shape)}")
        phi = init_level_set.to(dev).expand(B, H, W).clone(memory_format=torch.contiguous_format)
    image = chan_vese_normalize(x)
    lib = _lib.load()
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.ocm_chan_vese_workspace_bytes(B, H, W)
    ws = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ocm_op_chan_vese(_p(image), _p(phi), _p(mask), _p(iters), B, H, W, float(mu), float(lambda1),
                                        float(lambda2), float(tol), int(max_num_iter), float(dt), _p(ws), nbytes, _stream()))
    single = images_u8.dim() == 2
    out = (mask.view(torch.bool).reshape(images_u8.shape), iters[0] if single else iters)
    return out + (phi.reshape(images_u8.shape),) if return_phi else out


def chan_vese_result_u8(img_u8, attention):
    """utils.py:202-208: (img * attention / np.max(attention)).astype(np.uint8) — float32 products and quotients of the uint8
    image and the float32 map, truncated — for (H,W) or (B,H,W) tensors, the maximum taken per image."""
    a = attention.to(torch.float32)
    mx = a.amax(dim=(-2, -1), keepdim=True)
    return (img_u8.to(torch.float32) * a / mx).to(torch.uint8)


def chan_vese(img, attention, output_directory="", save=False, name=None, as_numpy=True):
    """utils.py:199-225 on device. img: the float (C,H,W) image tensor (what the reference turns into a PIL "L" image first)
    or an (H,W) uint8 tensor; attention: (H,W) float32 heat map. Returns (res_ours, res): the Chan-Vese segmentation
    (checkerboard start, mu 0.25, lambda 1 / 1, tol 1e-3, 200 iterations at most, dt 0.5) of the image weighted by the
    attention and of the image itself, both level sets evolved as one batch of two — uint8 {0, 255} numpy arrays
    (as_numpy=False keeps them on the device). The reference returns bool * 255, an int64 array of the same values. Saving
    figures (save=True) is the reference's matplotlib side effect and is not part of this path."""
    if save:
        raise NotImplementedError("chan_vese(save=True) writes figures with matplotlib in the reference; not on this path")
    _require_hip(attention, "attention")
    if attention.dtype != torch.float32 or attention.dim() != 2:
        raise ValueError(f"expected a float32 (H,W) attention map, got {attention.dtype} {tuple(attention.shape)}")
    if img.dtype == torch.uint8:
        _require_hip(img, "img")
        img_u8 = img.contiguous()
    else:
        img_u8 = image_to_gray_u8(img)[0]
    if tuple(img_u8.shape) != tuple(attention.shape):
        raise ValueError(f"image {tuple(img_u8.shape)} and attention {tuple(attention.shape)} differ in size")
    pair = torch.stack([chan_vese_result_u8(img_u8, attention), img_u8])
    masks = chan_vese_level_set(pair)[0].view(torch.uint8) * 255
    return tuple(m.cpu().numpy() for m in masks) if as_numpy else tuple(masks)


# ---- pixel k-means (reference utils.py:118-169; cv2.kmeans of OpenCV 4.x; kernels_kmeans_px.hip) ------------------------------
CV_RNG_START = 0xffffffff  # cv::RNG's state in a fresh process, and what its seed 0 stands for
_cv_rng_state = CV_RNG_START  # kmeans(rng_state=None) chains it, as OpenCV's thread-local generator runs on across calls


def cv_rng_uniform(state, n):
    """n uniforms of cv::RNG from `state` (ocm_cv_rng_uniform; 0 stands for 0xffffffff), on the host. Returns
    (float32 numpy array (n,), the state after them)."""
    st = C.c_uint64(int(state) & 0xffffffffffffffff)
    out = np.empty(int(n), np.float32)
    _lib.check(_lib.load().ocm_cv_rng_uniform(C.byref(st), out.ctypes.data_as(C.c_void_p), int(n)))
    return out, int(st.value)


def kmeans_pixels(images_u8, rng_state=CV_RNG_START, attempts=10, max_iter=10, eps=1.0):
    """cv2.kmeans(np.float32(img.reshape(-1, 3)), 2, None, (EPS + MAX_ITER, max_iter, eps), attempts, KMEANS_RANDOM_CENTERS),
    np.uint8(centres)[labels] and its Otsu mask (utils.py:130-146) for an (H,W) or (P,H,W) uint8 HIP tensor: every image is
    one problem of N = H W / 3 pixel triples, all of them go through one ocm_op_kmeans_px call and nothing is synchronised
    with the host. The random centres are cv::RNG's: P * attempts * 6 uniforms drawn from `rng_state` on the host, the
    problems consuming the stream in order. OpenCV is not installable here: restated from its source, parity unpinned.
    Returns a dict: mask (…,H,W) uint8 {0, 255}, labels (…,N) uint8, centers (…,2,3) float32, compactness (…,attempts) float64,
    iters (…,attempts) int32, best (…) int32 — all on the device, without the leading axis for an (H,W) image — and rng_state,
    the state after the draws."""
    if isinstance(images_u8, torch.Tensor) and images_u8.dim() in (2, 3) and (images_u8.shape[-1] * images_u8.shape[-2]) % 3:
        raise ValueError(f"cannot reshape {tuple(images_u8.shape[-2:])} pixels into triples (numpy's reshape(-1, 3) raises as well)")
    _require_hip(images_u8, "images")
    if images_u8.dtype != torch.uint8 or images_u8.dim() not in (2, 3):
        raise ValueError(f"expected a uint8 (H,W) or (P,H,W) image tensor, got {images_u8.dtype} {tuple(images_u8.shape)}")
    x = images_u8.contiguous().reshape((-1,) + tuple(images_u8.shape[-2:]))
    P, H, W = x.shape
    N = H * W // 3
    attempts = int(attempts)
    if not 1 <= attempts <= 32:
        raise ValueError(f"attempts = {attempts} (1..32)")
    dev = x.device
    u, state = cv_rng_uniform(rng_state, P * attempts * 6)
    lib = _lib.load()
    uniforms = torch.from_numpy(u).to(dev)
    out = dict(mask=torch.empty((P, H, W), dtype=torch.uint8, device=dev), labels=torch.empty((P, N), dtype=torch.uint8, device=dev),
               centers=torch.empty((P, 2, 3), dtype=torch.float32, device=dev),
               compactness=torch.empty((P, attempts), dtype=torch.float64, device=dev),
               iters=torch.empty((P, attempts), dtype=torch.int32, device=dev), best=torch.empty(P, dtype=torch.int32, device=dev))
    nbytes = lib.ocm_kmeans_px_workspace_bytes(P, N, attempts)
    ws = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ocm_op_kmeans_px(_p(x), P, N, _p(uniforms), attempts, int(max_iter), float(eps), _p(out["labels"]),
                                        _p(out["centers"]), _p(out["compactness"]), _p(out["iters"]), _p(out["best"]),
                                        _p(out["mask"]), _p(ws), nbytes, _stream()))
    if images_u8.dim() == 2:
        out = {k: v[0] for k, v in out.items()}
    out["rng_state"] = state
    return out


def kmeans(img, attention, output_directory="", save=False, name=None, as_numpy=True, rng_state=None):
    """utils.py:118-169 on device. img: the float (C,H,W) image tensor (what the reference turns into a PIL "L" image first)
    or an (H,W) uint8 tensor; attention: (H,W) float32 heat map. Returns (res_ours, res): the Otsu mask of the two-means
    painting (cv2.kmeans on the pixel triples: 10 attempts, 10 iterations at most, eps 1.0, random centres) of the image
    weighted by the attention and of the image itself, one call with two problems, "ours" first as the reference computes
    them — uint8 {0, 255} numpy arrays (as_numpy=False keeps them on the device). rng_state: the cv::RNG state the 120 draws
    start from; None chains a module-level state that starts at 0xffffffff, as OpenCV's thread-local generator does across the
    reference's calls. Saving figures (save=True) is the reference's matplotlib side effect and is not part of this path."""
    global _cv_rng_state
    if save:
        raise NotImplementedError("kmeans(save=True) writes figures with matplotlib in the reference; not on this path")
    if (isinstance(attention, torch.Tensor) and attention.dim() == 2 and attention.numel() % 3):
        raise ValueError(f"cannot reshape {tuple(attention.shape)} pixels into triples (numpy's reshape(-1, 3) raises as well)")
    _require_hip(attention, "attention")
    if attention.dtype != torch.float32 or attention.dim() != 2:
        raise ValueError(f"expected a float32 (H,W) attention map, got {attention.dtype} {tuple(attention.shape)}")
    if img.dtype == torch.uint8:
        _require_hip(img, "img")
        img_u8 = img.contiguous()
    else:
        img_u8 = image_to_gray_u8(img)[0]
    if tuple(img_u8.shape) != tuple(attention.shape):
        raise ValueError(f"image {tuple(img_u8.shape)} and attention {tuple(attention.shape)} differ in size")
    pair = torch.stack([chan_vese_result_u8(img_u8, attention), img_u8])
    r = kmeans_pixels(pair, rng_state=_cv_rng_state if rng_state is None else rng_state)
    if rng_state is None:
        _cv_rng_state = r["rng_state"]
    masks = r["mask"]
    return tuple(m.cpu().numpy() for m in masks) if as_numpy else tuple(masks)


# ---- the scores eval.py's validate loop reports (reference eval.py:204-221, utils.py:388-424; kernels_score.hip) --------------
SCORE_NAMES = ("jaccard", "f1", "recall", "precision", "accuracy", "auc", "dice_loss")  # columns of mask_scores' scores
COUNT_NAMES = ("tp", "fp", "fn", "tn")                                                 # columns of its counts


def mask_scores(pred, target, smooth=1):
    """Every image of a batch scored against its target in one ocm_op_mask_scores call, nothing synchronised with the host.
    pred: (B, ...) HIP tensor, a uint8 mask whose value is v / 255 (eval.py's `output / 255`) or float32 used as is;
    target: the same number of elements per image, uint8, bool or any float dtype (made contiguous float32). The classes are
    value > 0.5 and target > 0.5 (NaN: class 0).
    Returns (scores (B,7) float64 in SCORE_NAMES order, counts (B,4) int64 in COUNT_NAMES order) on the device:
    calculate_metrics' five sklearn scores, the ROC-AUC of the 0/1 prediction (NaN when the target holds one class) and
    DiceLoss()(value, target, smooth) per image, with float64 sums."""
    if isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor) and (
            pred.dim() < 1 or pred.numel() == 0 or target.numel() != pred.numel()):
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must hold the same, non-zero number of "
                         "elements, pred as (B, ...)")
    _require_hip(pred, "pred")
    _require_hip(target, "target")
    if pred.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"expected a uint8 or float32 (B, ...) prediction, got {pred.dtype} {tuple(pred.shape)}")
    if not (target.is_floating_point() or target.dtype in (torch.uint8, torch.bool)):
        raise ValueError(f"expected a float, uint8 or bool target, got {target.dtype}")
    B = pred.shape[0]
    count = pred.numel() // B
    dev = pred.device
    x = pred.detach().contiguous()
    t = target.detach().to(device=dev, dtype=torch.float32).contiguous()
    lib = _lib.load()
    scores = torch.empty((B, len(SCORE_NAMES)), dtype=torch.float64, device=dev)
    counts = torch.empty((B, len(COUNT_NAMES)), dtype=torch.int64, device=dev)
    nbytes = lib.ocm_mask_scores_workspace_bytes(B, count)
    ws = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ocm_op_mask_scores(_p(x), int(x.dtype == torch.uint8), _p(t), B, count, float(smooth), _p(counts),
                                          _p(scores), _p(ws), nbytes, _stream()))
    return scores, counts


def calculate_metrics(y_true, y_pred, y_score=None):
    """utils.py:388-408, and with `y_score` the six-score variant of PGT.py:247-275 / finetune.py:209, scored on the device:
    [jaccard, f1, recall, precision, accuracy] (+ [roc_auc of y_score > 0.5]) as np.float64, all of y_true taken as one image.
    y_pred and y_score are values compared with 0.5 as they are (any dtype; a uint8 tensor holds 0 / 1 here, as in the
    reference), y_true likewise. Reading the scores synchronises with the host, as the reference's sklearn calls do."""
    def one_image(t):
        _require_hip(t, "calculate_metrics input")
        return t.detach().to(torch.float32).reshape(1, -1)

    true = one_image(y_true)
    out = list(mask_scores(one_image(y_pred), true)[0][0, :5].cpu().numpy())
    if y_score is not None:
        out.append(mask_scores(one_image(y_score), true)[0][0, 5].cpu().numpy()[()])
    return out


# ---- Pillow's 8-bit resample (Image.resize, Image.crop(...).resize, ToTensor; kernels_resample.hip) ---------------------------
NEAREST, BILINEAR, BICUBIC = 0, 2, 3  # Pillow's Image.Resampling values


def resample_ksize(resample, in_size, in0, in1, out_size):
    """Taps per output pixel of one axis (ocm_resample_ksize, host): in_size source pixels, the box in0 .. in1 -> out_size."""
    k = _lib.load().ocm_resample_ksize(int(resample), int(in_size), float(in0), float(in1), int(out_size))
    if k < 0:
        _lib.check(-k)
    return int(k)


def resample_table(resample, in_size, in0, in1, out_size, flip=False, ksize_padded=None):
    """Pillow's coefficient table of one axis (ocm_resample_table, host; include/ocm_vit.h states the arithmetic): returns
    (bounds (out_size, 2) int32 = first tap and tap count, coeffs (out_size, ksize_padded) int32 with 22 fraction bits).
    ksize_padded defaults to the axis' own ksize; flip stores the rows in reverse order."""
    k = resample_ksize(resample, in_size, in0, in1, out_size)
    kp = k if ksize_padded is None else int(ksize_padded)
    bounds = np.empty((int(out_size), 2), np.int32)
    coeffs = np.empty((int(out_size), max(kp, 1)), np.int32)
    _lib.check(_lib.load().ocm_resample_table(int(resample), int(in_size), float(in0), float(in1), int(out_size), int(bool(flip)), kp,
                                              bounds.ctypes.data_as(C.c_void_p), coeffs.ctypes.data_as(C.c_void_p)))
    return bounds, coeffs


def _u8_image_geometry(t, layout):
    """(B, H, W, C, (stride_b, stride_y, stride_x, stride_c), batched) of a uint8 image tensor: (H,W), (H,W,C) / (C,H,W),
    (B,H,W,C) / (B,C,H,W). Without `layout` a last axis of 1 or 3 means interleaved ("hwc"), otherwise planar ("chw")."""
    d = t.dim()
    if d == 2:
        return 1, t.shape[0], t.shape[1], 1, (0, t.stride(0), t.stride(1), 0), False
    if layout is None:
        layout = "hwc" if t.shape[-1] in (1, 3) else "chw"
    if layout not in ("hwc", "chw"):
        raise ValueError(f"layout = {layout!r} ('hwc' or 'chw')")
    sh, st = tuple(t.shape), tuple(t.stride())
    B, sb = (sh[0], st[0]) if d == 4 else (1, 0)
    if layout == "hwc":
        (H, W, Cc), (sy, sx, sc) = sh[-3:], st[-3:]
    else:
        (Cc, H, W), (sc, sy, sx) = sh[-3:], st[-3:]
    return B, H, W, Cc, (sb, sy, sx, sc), d == 4


def _per_image(value, B, what):
    """A flag for the whole batch, or one per image -> (list of B bools, whether it was per image)."""
    if value is None or isinstance(value, (bool, np.bool_)):
        return [bool(value)] * B, False
    flags = [bool(v) for v in (value.tolist() if hasattr(value, "tolist") else value)]
    if len(flags) != B:
        raise ValueError(f"{what}: {len(flags)} flags for {B} images")
    return flags, True


class ResamplePlan:
    """Everything of a pil_resize call that depends on the geometry alone: the two axes' coefficient tables (built on the host by
    ocm_resample_table, one upload for all of them), the crop rectangles and the sizes. A plan serves any image tensor of the
    shape, strides and device it was made for, call after call (run). The arguments are pil_resize's."""

    def __init__(self, images_u8, size, resample=BICUBIC, box=None, crop=None, hflip=None, vflip=None, layout=None):
        if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() not in (2, 3, 4):
            raise ValueError("expected a uint8 (H,W), (H,W,C), (B,H,W,C), (C,H,W) or (B,C,H,W) image tensor, got "
                             f"{getattr(images_u8, 'dtype', type(images_u8))} {tuple(getattr(images_u8, 'shape', ()))}")
        if resample not in (NEAREST, BILINEAR, BICUBIC):
            raise ValueError(f"resample = {resample!r} (NEAREST 0, BILINEAR 2, BICUBIC 3)")
        B, H, W, Cc, strides, batched = _u8_image_geometry(images_u8, layout)
        if Cc not in (1, 3):
            raise ValueError(f"{Cc} channels (1 or 3)")
        out_w, out_h = int(size[0]), int(size[1])
        if out_w < 1 or out_h < 1:
            raise ValueError(f"size = {tuple(size)} (width, height >= 1)")
        hf, hf_each = _per_image(hflip, B, "hflip")
        vf, vf_each = _per_image(vflip, B, "vflip")
        rects, crop_each = None, False
        if crop is not None:
            rects = np.asarray(crop, dtype=np.int64)
            crop_each = rects.ndim == 2
            rects = rects if crop_each else np.broadcast_to(rects.reshape(-1, 4), (B, 4))
            if rects.shape != (B, 4):
                raise ValueError(f"crop: {rects.shape[0]} rectangles for {B} images")
            if (rects[:, 0] < 0).any() or (rects[:, 1] < 0).any() or (rects[:, 2] > W).any() or (rects[:, 3] > H).any() or (
                    rects[:, 2] <= rects[:, 0]).any() or (rects[:, 3] <= rects[:, 1]).any():
                raise ValueError(f"crop rectangles must be non-empty and inside the {W} x {H} image")
        per_image = crop_each or hf_each or vf_each
        _require_hip(images_u8, "images")

        def axis_tables(sizes, lo, hi, out, flips):
            spans = [(n, 0.0 if box is None else float(box[lo]), float(n) if box is None else float(box[hi])) for n in sizes]
            ks = [resample_ksize(resample, n, a, b, out) for n, a, b in spans]
            tabs = [resample_table(resample, n, a, b, out, f, max(ks)) for (n, a, b), f in zip(spans, flips)]
            return np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), max(ks)

        T = B if per_image else 1
        widths = [W] * T if rects is None else [int(r[2] - r[0]) for r in rects[:T]]
        heights = [H] * T if rects is None else [int(r[3] - r[1]) for r in rects[:T]]
        xb, xc, self.xk = axis_tables(widths, 0, 2, out_w, hf[:T])
        yb, yc, self.yk = axis_tables(heights, 1, 3, out_h, vf[:T])
        parts = [xb, xc, yb, yc]
        if rects is not None:  # (y0, x0, h, w) per image
            parts.append(np.stack([rects[:, 1], rects[:, 0], rects[:, 3] - rects[:, 1], rects[:, 2] - rects[:, 0]], 1).astype(np.int32))
        self.device = images_u8.device
        self.tables = torch.from_numpy(np.concatenate([p.reshape(-1) for p in parts])).to(self.device)
        offs = np.cumsum([0] + [p.size for p in parts])
        self.ptr = [C.c_void_p(self.tables.data_ptr() + 4 * int(o)) for o in offs[:-1]] + [None] * (5 - len(parts))
        self.tmp_rows = H if rects is None else int((rects[:, 3] - rects[:, 1]).max())
        self.per_image, self.batched, self.dims = int(per_image), batched, images_u8.dim()
        self.geometry = (tuple(images_u8.shape), tuple(images_u8.stride()))
        self.B, self.H, self.W, self.C, self.strides, self.out_h, self.out_w = B, H, W, Cc, strides, out_h, out_w
        self.workspace_bytes = int(_lib.load().ocm_resample_u8_workspace_bytes(B, Cc, self.tmp_rows, out_w))

    def run(self, images_u8, to_tensor=False):
        """One ocm_op_resample_u8 call on the current stream: see pil_resize for what comes back."""
        if to_tensor not in (False, True, "both"):
            raise ValueError(f"to_tensor = {to_tensor!r} (False, True or 'both')")
        _require_hip(images_u8, "images")
        if images_u8.dtype != torch.uint8 or (tuple(images_u8.shape), tuple(images_u8.stride())) != self.geometry or (
                images_u8.device != self.device):
            raise ValueError("the plan was made for a uint8 tensor of another shape, other strides or another device")
        dev, B, Cc = self.device, self.B, self.C
        want_u8, want_f32 = to_tensor in (False, "both"), to_tensor in (True, "both")
        out_u8 = torch.empty((B, self.out_h, self.out_w, Cc), dtype=torch.uint8, device=dev) if want_u8 else None
        out_f32 = torch.empty((B, Cc, self.out_h, self.out_w), dtype=torch.float32, device=dev) if want_f32 else None
        ws = _ws(self.workspace_bytes, dev)
        p = self.ptr
        with torch.cuda.device(dev):
            _lib.check(_lib.load().ocm_op_resample_u8(_p(images_u8), *(int(s) for s in self.strides), B, Cc, self.H, self.W, p[4],
                                                      self.tmp_rows, p[0], p[1], self.xk, p[2], p[3], self.yk, self.per_image,
                                                      self.out_h, self.out_w, _p(out_u8), _p(out_f32), _p(ws), self.workspace_bytes,
                                                      _stream()))
        if not self.batched:
            out_u8 = None if out_u8 is None else (out_u8[0, :, :, 0] if self.dims == 2 else out_u8[0])
            out_f32 = None if out_f32 is None else out_f32[0]
        return (out_u8, out_f32) if to_tensor == "both" else out_f32 if to_tensor else out_u8


def pil_resize(images_u8, size, resample=BICUBIC, box=None, crop=None, hflip=None, vflip=None, to_tensor=False, layout=None):
    """PIL.Image.resize(size, resample, box) of every image of a uint8 HIP tensor in one ocm_op_resample_u8 call, byte for byte
    (Pillow's integer passes, horizontal first; pinned on the live library by tests/test_resample_host.py), nothing
    synchronised with the host. images_u8: (H,W) ("L"), (H,W,C), (B,H,W,C) or the planar (C,H,W) / (B,C,H,W), C in (1, 3),
    read through its strides (a view with a wider row pitch is not copied); see _u8_image_geometry for `layout`.
    size: (width, height) as Pillow takes it; resample: NEAREST, BILINEAR or BICUBIC (Pillow's default for resize).
    box: (x0, y0, x1, y1) floats, Pillow's box= (taps read outside it). crop: (x0, y0, x1, y1) integers inside the image, or
    one rectangle per image ((B,4)): Image.crop(rect).resize(...), taps stop at the rectangle (a box then counts inside it).
    hflip / vflip: a flag or one per image: the resized image mirrored, as RandomHorizontalFlip / RandomVerticalFlip after
    RandomResizedCrop do (the rows of the coefficient tables reversed: no work on the device).
    Returns uint8 (h,w) / (h,w,C) / (B,h,w,C); with to_tensor=True float32 (C,h,w) / (B,C,h,w) = ToTensor (u8 / 255.0f);
    with to_tensor="both" the pair (uint8, float32). The tables are built on the host for every call: ResamplePlan keeps them
    for callers that resize one geometry again and again."""
    if to_tensor not in (False, True, "both"):
        raise ValueError(f"to_tensor = {to_tensor!r} (False, True or 'both')")
    return ResamplePlan(images_u8, size, resample, box, crop, hflip, vflip, layout).run(images_u8, to_tensor)


# ---- Pillow's point operations and Gaussian blur for a batch (ImageEnhance, convert('HSV' / 'L'), ImageOps.solarize,
# ImageFilter.GaussianBlur, ToTensor + Normalize; kernels_augment.hip) -------------------------------------------------------------
COLOR_NONE, COLOR_BRIGHTNESS, COLOR_CONTRAST, COLOR_SATURATION, COLOR_HUE = range(5)  # the slots of pil_color


def gaussian_blur_table(radius):
    """(r, ww, fw) of every radius as Pillow's box blur forms them (ocm_gaussian_blur_table, host): uint32 (n, 3)."""
    radii = np.atleast_1d(np.asarray(radius, dtype=np.float32))
    table = np.empty((radii.size, 3), np.uint32)
    lib = _lib.load()
    for i, r in enumerate(radii.reshape(-1)):
        _lib.check(lib.ocm_gaussian_blur_table(float(r), table[i].ctypes.data_as(C.c_void_p)))
    return table


def _u8_batch_rgb(images_u8, what):
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"{what}: expected a uint8 (B,H,W,3) batch, got {getattr(images_u8, 'dtype', type(images_u8))} "
                         f"{tuple(getattr(images_u8, 'shape', ()))}")
    _require_hip(images_u8, what)
    return images_u8.contiguous()


def _per_image_table(value, shape, dtype, what):
    """One value for the whole batch, or one per image -> a contiguous array of `shape`."""
    if isinstance(value, torch.Tensor):
        value = value.cpu().numpy()
    try:
        return np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=dtype), shape))
    except ValueError:
        raise ValueError(f"{what}: shape {np.shape(value)} for {shape}") from None


def pil_color(images_u8, ops, factors, grey=False, solarize=False, threshold=128, out=None):
    """The point operations of torchvision's ColorJitter / RandomGrayscale on PIL images and ImageOps.solarize for a uint8
    (B,H,W,3) HIP batch in one ocm_op_color_u8 call, byte for byte what Pillow gives (tests/test_augment_host.py), every image
    with its own parameters. ops (B,4): COLOR_* slots run in order; factors (B,4) float32: the enhancement factor of
    ImageEnhance.{Brightness, Contrast, Color}, or for COLOR_HUE the byte shift uint8(hue_factor * 255). grey / solarize: a flag
    or one per image (grey, then solarize with `threshold`, after the slots). out: the batch itself for an in-place call."""
    x = _u8_batch_rgb(images_u8, "images")
    B, H, W, _ = x.shape
    ops = _per_image_table(ops, (B, 4), np.int32, "ops")
    if ((ops < COLOR_NONE) | (ops > COLOR_HUE)).any():
        raise ValueError("ops: slots are COLOR_NONE .. COLOR_HUE (0..4)")
    fac = _per_image_table(factors, (B, 4), np.float32, "factors")
    if not np.isfinite(fac).all():
        raise ValueError("factors must be finite")
    flags = np.stack([_per_image_table(grey, (B,), np.int32, "grey"), _per_image_table(solarize, (B,), np.int32, "solarize"),
                      _per_image_table(threshold, (B,), np.int32, "threshold")], 1)
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.uint8 or out.shape != x.shape or out.device != x.device or not out.is_contiguous():
        raise ValueError("out: a contiguous uint8 tensor of the batch's shape on its device")
    dev, lib = x.device, _lib.load()
    tables = torch.from_numpy(np.concatenate([ops.reshape(-1), fac.view(np.int32).reshape(-1), flags.reshape(-1)])).to(dev)
    base = tables.data_ptr()
    nbytes = lib.ocm_color_u8_workspace_bytes(B)
    ws = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ocm_op_color_u8(_p(x), _p(out), B, H, W, C.c_void_p(base), C.c_void_p(base + 16 * B), C.c_void_p(base + 32 * B),
                                       _p(ws), nbytes, _stream()))
    return out


def pil_gaussian_blur(images_u8, radius, solarize=None, to_tensor=False, mean=None, std=None):
    """Image.filter(ImageFilter.GaussianBlur(radius)) of every image of a uint8 (B,H,W,3) HIP batch in one
    ocm_op_gaussian_blur_u8 call (two launches), byte for byte. radius: one value or one per image; 0 copies the image.
    solarize: None, or per image a threshold applied after the blur (256: not solarized). Returns uint8 (B,H,W,3); with
    to_tensor=True float32 (B,3,H,W) = ToTensor, then Normalize(mean, std) when the two are given; with "both" the pair."""
    if to_tensor not in (False, True, "both"):
        raise ValueError(f"to_tensor = {to_tensor!r} (False, True or 'both')")
    if (mean is None) != (std is None):
        raise ValueError("mean and std come together")
    x = _u8_batch_rgb(images_u8, "images")
    B, H, W, _ = x.shape
    dev, lib = x.device, _lib.load()
    cap = lib.ocm_gaussian_blur_max_axis()
    if H > cap or W > cap:
        raise ValueError(f"a {H} x {W} image: the blur holds an axis of up to {cap} pixels")
    parts = [gaussian_blur_table(_per_image_table(radius, (B,), np.float32, "radius")).view(np.int32).reshape(-1)]
    if solarize is not None:
        parts.append(_per_image_table(solarize, (B,), np.int32, "solarize"))
    tables = torch.from_numpy(np.concatenate(parts)).to(dev)
    want_u8, want_f32 = to_tensor in (False, "both"), to_tensor in (True, "both")
    out_u8 = torch.empty_like(x) if want_u8 else None
    out_f32 = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_f32 else None
    norm = [None, None] if mean is None else [(C.c_float * 3)(*(float(v) for v in m)) for m in (mean, std)]
    nbytes = lib.ocm_gaussian_blur_u8_workspace_bytes(B, H, W)
    ws = _ws(nbytes, dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ocm_op_gaussian_blur_u8(_p(x), B, H, W, C.c_void_p(tables.data_ptr()),
                                               None if solarize is None else C.c_void_p(tables.data_ptr() + 12 * B), _p(out_u8),
                                               _p(out_f32), *(None if m is None else C.cast(m, C.c_void_p) for m in norm), _p(ws),
                                               nbytes, _stream()))
    return (out_u8, out_f32) if to_tensor == "both" else out_f32 if to_tensor else out_u8


# ---- the gradient norm and its clipping (torch.nn.utils.clip_grad_norm_, reference utils.py:363-373; kernels_optim.hip) -----------
def _grad_norm_launch(parameters, max_norm, norm_type, scale, error_if_nonfinite=False):
    """ocm_op_grad_norm (and, with `scale`, ocm_op_grad_scale) over the gradients of `parameters`, which may be a tensor or any
    iterable (it is walked once); returns the norm as a 0-dim float32 tensor on the gradients' device. Nothing synchronises with
    the host unless `error_if_nonfinite` asks for the norm between the two launches."""
    if float(norm_type) != 2.0:
        raise ValueError(f"norm_type = {norm_type}: the HIP path computes the 2-norm only")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)  # what torch returns for no gradients
    device, grads = None, []
    for p in params:
        g = p.grad
        device = _check_tensor(g, "a gradient", device)
        if not g.is_contiguous():
            g = g.contiguous()
            if scale:
                p.grad = g  # scaled in place below: the parameter keeps the copy
        grads.append(g)  # a copy that is only read lives until the launches are queued; the allocator is stream-ordered
    zeros = [0] * len(grads)
    table = _table((zeros, [g.data_ptr() for g in grads], zeros, zeros, [g.numel() for g in grads]))
    lib = _lib.load()
    tab, n = table.ctypes.data, table.shape[0]
    nbytes = lib.ocm_grad_norm_workspace_bytes(tab, n)
    if not nbytes:
        raise ValueError("a gradient holds more than 2^36 elements")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    out = torch.empty(4, dtype=torch.float32, device=device)  # [sum of squares: float64][norm][coefficient]
    base = out.data_ptr()
    with torch.cuda.device(device):
        stream = _stream()
        _lib.check(lib.ocm_op_grad_norm(tab, n, float(max_norm), base, base + 8, base + 12, _p(ws), nbytes, stream))
        if error_if_nonfinite and not bool(torch.isfinite(out[2])):
            raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it "
                               "cannot be clipped. To disable this error and scale the gradients by the non-finite norm anyway, "
                               "set `error_if_nonfinite=False`")
        if scale:
            _lib.check(lib.ocm_op_grad_scale(tab, n, base + 12, stream))
            torch.autograd.graph.increment_version(grads)
    return out[2]


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for fp32 gradients on one HIP device: every gradient is multiplied in place by
    clamp(max_norm / (norm + 1e-6), max=1), formed on the device in float32 as torch forms it (a NaN or infinite norm does what
    torch's does). `parameters` is a tensor or any iterable of tensors, a generator such as model.parameters() included. Returns
    the norm before clipping, a 0-dim float32 device tensor, without synchronising; `error_if_nonfinite` reads it back once, before
    anything is scaled, as torch's does. A non-contiguous gradient is replaced by a contiguous copy and that is scaled. The norm
    is the float32 rounding of a float64 sum of squares: the same bits on every call. `foreach` is accepted and ignored."""
    return _grad_norm_launch(parameters, max_norm, norm_type, scale=True, error_if_nonfinite=error_if_nonfinite)


def grad_norm(parameters, norm_type=2.0):
    """The 2-norm of all gradients of `parameters` as clip_grad_norm_ returns it, the gradients left as they are (the norm of a
    non-contiguous gradient is taken on a temporary contiguous copy)."""
    return _grad_norm_launch(parameters, float("inf"), norm_type, scale=False)


def get_grad_norm(parameters, norm_type=2):
    """reference utils.py:363-373 as a Python float: one synchronisation instead of one .item() per parameter."""
    return float(grad_norm(parameters, norm_type))
