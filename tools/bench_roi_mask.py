"""Times the ROI-guided SimMIM masks (data.roi_mask: kernels_roi.hip around ocm_op_binary_morph and ocm_op_label8) with device
events at the two geometries of the reference's sweep, B = 128 each:
  * S = 320, patch 8 (G = 40) and S = 224, patch 16 (G = 14), on synthetic tiles (smooth bright blobs on a near-black ground)
    that went through simmim_images;
  * roi_mask per batch, and its four stages on their own (threshold, closing, label8, apply) — the closing's share is what a
    fused threshold + closing kernel could win at most;
  * simmim_images on the same batch, for scale;
  * on the CPU, per image: the chain on scipy.ndimage (what skimage 0.19.3 calls in the reference's data loader) and the
    pure-numpy restatement of tests/roi_mask_ref.py.
Every device figure is the median of `--repeat` runs after `--warmup` runs. Prints one JSON object.
    python tools/bench_roi_mask.py [--repeat 20] [--warmup 3] [--batch 128]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import roi_mask_ref as R  # noqa: E402
from vit_ocm_wmsegmentation_amd import _lib, data, utils  # noqa: E402


def tissue_tiles(batch, side, seed, cell=24):
    """uint8 (batch, side, side, 3): grey blobs of about `cell` pixels (levels 30..255) on a ground of levels 0..8."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((batch, 1, side // cell + 2, side // cell + 2), generator=g)
    fine = torch.nn.functional.interpolate(coarse, size=(side, side), mode="bilinear", align_corners=False)[:, 0]
    bright = (30 + 225 * torch.rand((batch, side, side), generator=g)).to(torch.uint8)
    ground = (9 * torch.rand((batch, side, side), generator=g)).to(torch.uint8)
    return torch.where(fine > 0.3, bright, ground)[..., None].expand(-1, -1, -1, 3).contiguous()


def _time(fn, repeat, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def scipy_chain(img, mask):
    """data.py:216-233 with the scipy.ndimage calls skimage 0.19.3 makes; None without scipy."""
    try:
        import scipy.ndimage as ndi
    except ImportError:
        return None
    binary = R.gray_u8(img) > 10
    if np.count_nonzero(binary) < 20:
        binary[:] = False
    closed = ndi.binary_erosion(ndi.binary_dilation(binary, R.M.DISK2), R.M.DISK2, border_value=1)
    rois = ndi.label(closed, structure=np.ones((3, 3)))[0].astype(np.float64)
    rois = ndi.zoom(rois, (mask.shape[0] / rois.shape[0], mask.shape[1] / rois.shape[1]), order=0, mode="mirror", grid_mode=True)
    rois = rois.astype(np.uint8) != 0
    new = mask * rois
    return new if new.sum() else mask


def bench(dev, side, patch, batch, repeat, warmup):
    tiles = tissue_tiles(batch, 384, side).to(dev)
    gen = data.MaskGenerator(side, 32, patch, 0.6)
    np.random.seed(side)
    masks_np = np.stack([gen() for _ in range(batch)]).astype(np.int64)
    masks = torch.from_numpy(masks_np).to(dev)
    g = torch.Generator().manual_seed(side)
    img = data.simmim_images(tiles, side, g)
    G = side // patch
    out = {"batch": batch, "image": side, "grid": G}
    out["simmim_images_ms"] = _time(lambda: data.simmim_images(tiles, side, g), repeat, warmup)
    out["roi_mask_ms"] = _time(lambda: data.roi_mask(img, masks), repeat, warmup)
    new, used = data.roi_mask(img, masks)
    out["used_images"] = int(used.sum())
    out["masked_cells_before_after"] = [int(masks.sum()), int(new.sum())]

    # the four stages on their own, on buffers of their own
    lib = _lib.load()
    B, h, w = batch, side, side
    binary = torch.empty((B, h, w), dtype=torch.uint8, device=dev)
    grown, closed = torch.empty_like(binary), torch.empty_like(binary)
    white = torch.empty(B, dtype=torch.int32, device=dev)
    labels = torch.empty((B, h, w), dtype=torch.int32, device=dev)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    nbytes = lib.ocm_label8_workspace_bytes(B, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tables = torch.from_numpy(np.concatenate([utils.roi_sample_index(h, G), utils.roi_sample_index(w, G)])).to(dev)
    res, flag = torch.empty_like(masks), torch.empty(B, dtype=torch.bool, device=dev)
    size, bits = utils.footprint_bits(utils.DISK2)
    s = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def threshold():
        _lib.check(lib.ocm_op_roi_threshold(p(img), img.stride(0), img.stride(1), 3, B, h, w, 10, p(binary), p(white), s()))

    def closing():
        _lib.check(lib.ocm_op_binary_morph(p(binary), p(grown), B, h, w, bits, size, 0, 0, s()))
        _lib.check(lib.ocm_op_binary_morph(p(grown), p(closed), B, h, w, bits, size, 1, 1, s()))

    def label():
        _lib.check(lib.ocm_op_label8(p(closed), p(labels), p(counts), B, h, w, p(ws), nbytes, s()))

    def apply():
        _lib.check(lib.ocm_op_roi_apply(p(labels), p(tables), tables.data_ptr() + 4 * G, p(white), 20, p(masks), 8, p(res), p(flag),
                                        B, h, w, G, G, s()))

    for name, fn in (("threshold", threshold), ("closing", closing), ("label8", label), ("apply", apply)):
        out[f"stage_{name}_ms"] = _time(fn, repeat, warmup)
    assert torch.equal(res, new) and torch.equal(flag, used)
    out["components_per_image_max"] = int(counts.max())

    # the host chains, per image
    img_np = img[:8].cpu().numpy()
    scipy_chain(img_np[0], masks_np[0])  # the import and the first call's set-up are not the loader's steady state
    t0 = time.perf_counter()
    got = [scipy_chain(i, m) for i, m in zip(img_np, masks_np)]
    t1 = time.perf_counter()
    if got[0] is not None:
        out["host_scipy_ms_per_image"] = round((t1 - t0) * 1e3 / len(img_np), 3)
        assert all(np.array_equal(a, b) for a, b in zip(got, new[:8].cpu().numpy()))
    t0 = time.perf_counter()
    ref = [R.roi_mask(i, m)[0] for i, m in zip(img_np[:2], masks_np)]
    out["host_numpy_restatement_ms_per_image"] = round((time.perf_counter() - t0) * 1e3 / 2, 1)
    assert all(np.array_equal(a, b) for a, b in zip(ref, new[:2].cpu().numpy()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_roi_mask.py needs a HIP device: nothing here can be timed without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "repeat": args.repeat}
    res["S320_p8"] = bench(dev, 320, 8, args.batch, args.repeat, args.warmup)
    res["S224_p16"] = bench(dev, 224, 16, args.batch, args.repeat, args.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
