"""The post-processing operators of csrc/kernels_post.hip at every geometry they accept. Needs an MI355X.

tests/test_post_gpu.py holds each of these kernels to its reference at the one geometry the pipelines use (windows of
3 x stride, one query row, square maps at scale 8, median sizes <= 7 on 24 x 20 maps, one image size per u8 operator);
tests/test_memcheck_gpu.py shows that they stay inside their buffers. This module holds the VALUES at the shapes where
such kernels go wrong: strides that do not divide the window, two-window folds, one-element ramps, distinct R / G / B
planes and strided slabs in the stitchers; n_rows > 1, pixel counts off a multiple of 256, 1 and 12 heads and flat
windows in the head mean / min-max; non-square maps, one-pixel sides and scales with an inexact reciprocal in the
bilinear upsample; every parity of the centre down-scale; the median filter on maps of height / width 1 with windows
reflecting through several periods, at eval.py's size 13 and the cap 15; grid-stride loops past one trip of the grid;
u8 counts of 1, 255, 257, ...; blend_u8 / weighted_u8 over all 256 x 256 input pairs.

The C ABI is called directly (n_rows, strides and scratch are arguments the Python wrappers hide). Every output is an
exactly sized payload between 64 KiB guard bands (tests/memcheck.Guarded) and is poisoned before the call; every case
runs twice, on two different poisons (floats: two NaN patterns; u8 images and histograms: 0x7F.. and 0xFF..), and the
two results must be the same bits, so an element the kernel leaves unwritten shows as well. All comparisons are
bit-exact except the bilinear upsample's, whose bound is derived in its test's docstring.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vit_oracle as O
from tests.golden_cases import (BILINEAR_SHAPES, MEDIAN_EDGE_SHAPES, MEDIAN_EDGE_SIZES, STITCH_GEOMETRIES,
                                STITCH_U8_GEOMETRIES, median_edge_inputs)
from tests.helpers import load_golden
from tests.memcheck import Guarded, assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL = _lib.OCM_EINVAL
F32, U8, I64 = torch.float32, torch.uint8, torch.int64
POISONS = {True: ("nan", "ones"), False: ("big", "ones")}  # by is_floating_point: first and second run
U8_COUNTS = (1, 255, 256, 257, 65535, 1024 * 256 + 3)  # the last: three elements into a second trip of 1024 workgroups


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_twice(lib, what, call, specs, scratch_bytes=None):
    """`call(ptrs, scratch_ptr) -> rc` on guarded, poisoned outputs, twice. specs: {name: (shape, dtype)}. Asserts rc 0,
    untouched guards and the same bits from both runs; returns {name: numpy array} of the first."""
    runs = []
    for rnd in range(2):
        outs = {}
        for name, (shape, dtype) in specs.items():
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            outs[name] = Guarded(nbytes, "cuda", POISONS[dtype.is_floating_point][rnd])
        scratch = Guarded(scratch_bytes, "cuda", ("nan", "big")[rnd]) if scratch_bytes else None
        torch.cuda.synchronize()
        rc = call({k: g.ptr for k, g in outs.items()}, scratch.ptr if scratch else None)
        assert rc == 0, f"{what}: rc {rc} ({lib.ocm_last_error().decode(errors='replace')})"
        torch.cuda.synchronize()
        for name, g in list(outs.items()) + ([("scratch", scratch)] if scratch else []):
            bad = g.check()
            assert bad is None, f"{what}: {name}: {bad}"
        runs.append({k: g.payload().clone() for k, g in outs.items()})
    res = {}
    for name, (shape, dtype) in specs.items():
        assert_same_bits(runs[0][name], runs[1][name], f"{what}: {name}, first vs second run (bytes)")
        res[name] = runs[0][name].view(dtype).view(tuple(shape)).cpu().numpy()
    return res


def _hist_of(u8):
    return np.bincount(np.asarray(u8, dtype=np.uint8).ravel(), minlength=256).astype(np.int64)


def _ramp(window, stride, dev):
    return torch.from_numpy(np.linspace(1, 0, window - stride)).to(dev)  # float64, as the reference builds it


# ---------------------------------------------------------------------------------------------------------------------
# stitchers
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,window,stride", STITCH_GEOMETRIES)
def test_stitch_every_window_to_stride_ratio(dev, lib, n, window, stride):
    """ocm_op_stitch == oracle.concat_crops bit for bit (float64 blend, rounded to float32 once per fold) on windows of
    rng.random * 255 with a few negative and a few 1e6-sized entries, which a swapped or reversed ramp weight cannot hide."""
    rng = np.random.default_rng(1000 * n + 31 * window + stride)
    crops = rng.random((n * n, window, window), dtype=np.float32) * 255
    flat = crops.reshape(-1)
    odd = rng.choice(flat.size, max(6, flat.size // 40), replace=False)
    flat[odd[::2]] = (flat[odd[::2]] + 1) * np.float32(-8)
    flat[odd[1::2]] = (flat[odd[1::2]] + 1) * np.float32(4e3)  # up to 1e6
    want = O.concat_crops(crops, stride, window)
    S = window + (n - 1) * stride
    assert want.shape == (S, S) and want.dtype == np.float32 and (want < 0).any() and (want > 3e5).any()
    d, ramp = torch.from_numpy(crops).to(dev), _ramp(window, stride, dev)
    got = run_twice(lib, f"stitch n={n} window={window} stride={stride}",
                    lambda p, sc: lib.ocm_op_stitch(d.data_ptr(), p["out"], ramp.data_ptr(), n, window, stride, _s()),
                    {"out": ((S, S), F32)})["out"]
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} pixels differ"


def test_stitch_rejects_geometries_outside_its_fold(dev, lib):
    """The closed form folds at most three windows per axis: stride < window <= 3 * stride, n >= 1, and a ramp."""
    crops = torch.zeros((4, 16, 16), device=dev)
    out = torch.zeros((64, 64), device=dev)
    ramp = _ramp(16, 4, dev)
    args = lambda n, window, stride, r=ramp: lib.ocm_op_stitch(crops.data_ptr(), out.data_ptr(), r.data_ptr() if r is not None  # noqa: E731
                                                               else None, n, window, stride, _s())
    assert args(2, 4, 4) == EINVAL       # window == stride: nothing to blend over
    assert args(2, 13, 4) == EINVAL      # window == 3 * stride + 1: a fourth window would cover a pixel
    assert args(0, 12, 4) == EINVAL
    assert args(2, 12, 0) == EINVAL
    assert args(2, 12, 4, None) == EINVAL
    assert args(2, 12, 4) == 0
    u8 = torch.zeros((64, 64), dtype=U8, device=dev)
    slab = torch.zeros((3, 20, 20), device=dev)
    args8 = lambda n, window, stride: lib.ocm_op_stitch_image_u8(slab.data_ptr(), 400, 20, 3, 20, 20, u8.data_ptr(),  # noqa: E731
                                                                 ramp.data_ptr(), n, window, stride, None, _s())
    assert args8(3, 4, 4) == EINVAL and args8(3, 13, 4) == EINVAL and args8(0, 12, 4) == EINVAL and args8(3, 12, 4) == 0
    torch.cuda.synchronize()


def test_uint8_levels_survive_the_float_slab():
    """The u8 stitcher reads the windows back from the ToTensor slab x = u / 255 as rint(x * 255): that is u for all 256
    levels in float32."""
    u = np.arange(256, dtype=np.float32)
    x = u / np.float32(255)
    assert x.dtype == np.float32 and np.array_equal(np.rint(x * np.float32(255)), u)
    assert np.array_equal(torch.round(torch.arange(256, dtype=F32).div(255) * 255).numpy(), u)


U8_STITCH_CASES = [g + ("planes",) for g in STITCH_U8_GEOMETRIES] + [(21, 23, 4, 12, "strided"), (21, 23, 4, 12, "one_plane"),
                                                                      (25, 27, 7, 10, "strided")]


@pytest.mark.parametrize("H,W,stride,window,layout", U8_STITCH_CASES)
def test_stitch_image_u8_distinct_planes(dev, lib, H, W, stride, window, layout):
    """ocm_op_stitch_image_u8 == oracle.stitched_gray_image bit for bit on three INDEPENDENT random uint8 planes (the
    R, G, B weights of PIL's "L" and the plane stride are invisible on identical planes). `strided`: the slab is a view
    of a larger NaN-filled tensor (stride_y > W, stride_c > H * W), so a read outside the slab's rows or planes, where
    PIL crop's zeros belong, turns up as garbage. The histogram is np.bincount of the expected image."""
    rng = np.random.default_rng(7 * H + W + stride)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if layout == "one_plane":
        img = img[:, :, :1]
    chans = img.shape[2]
    n = len(range(0, H - 2 * stride, stride))  # sliding_window's origins per axis
    assert n >= 1 and n == len(range(0, W - 2 * stride, stride)) and n * n == len(O.sliding_window_origins(H, W, stride))
    S = window + (n - 1) * stride
    want = O.stitched_gray_image(img[:, :, 0] if chans == 1 else img, stride, window)
    assert want.shape == (S, S)
    planes = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(F32).div(255)  # ToTensor
    if layout == "strided":
        big = torch.full((chans, H + 3, W + 5), float("nan"), device=dev)
        slab = big[:, 1:1 + H, 2:2 + W]
        slab.copy_(planes)
        assert slab.stride(1) > W and slab.stride(0) > H * W and slab.stride(2) == 1
    else:
        slab = planes.to(dev)
    ramp = _ramp(window, stride, dev)
    got = run_twice(lib, f"stitch_image_u8 {H}x{W} stride={stride} window={window} {layout}",
                    lambda p, sc: lib.ocm_op_stitch_image_u8(slab.data_ptr(), slab.stride(0), slab.stride(1), chans, H, W, p["out"],
                                                             ramp.data_ptr(), n, window, stride, p["hist"], _s()),
                    {"out": ((S, S), U8), "hist": ((256,), I64)})
    assert np.array_equal(got["out"], want), f"{int((got['out'] != want).sum())} of {want.size} pixels differ"
    assert np.array_equal(got["hist"], _hist_of(want)) and int(got["hist"].sum()) == S * S


# ---------------------------------------------------------------------------------------------------------------------
# head mean and per-window min-max
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,heads,n_rows,P", [(3, 1, 1, 1), (2, 6, 3, 255), (2, 12, 8, 257), (4, 3, 2, 256), (1, 6, 1, 2304)])
def test_tile_postprocess_and_head_mean_use_row_zero(dev, lib, T, heads, n_rows, P):
    """ocm_op_tile_postprocess == oracle.tile_postprocess and ocm_op_head_mean == np.mean(axis=0), float32, bit for bit,
    on (T, heads, n_rows, P) rows whose rows 1.. hold NaN: a head stride of P instead of n_rows * P reads them. The last
    window of every multi-window case is flat (each head constant): the reference's 0 / 0 is NaN on every pixel, and so
    must the kernel's be; a window of one pixel is flat by construction."""
    rng = np.random.default_rng(100 * T + heads + P)
    rows = np.full((T, heads, n_rows, P), np.nan, np.float32)
    rows[:, :, 0] = rng.random((T, heads, P), dtype=np.float32) * np.float32(0.01)
    flat = [T - 1] if (T > 1 and P > 1) else (list(range(T)) if P == 1 else [])
    for t in flat:
        rows[t, :, 0, :] = rows[t, :, 0, :1]
    with np.errstate(invalid="ignore", divide="ignore"):
        want = O.tile_postprocess(rows[:, :, 0])
    want_mean = np.stack([np.mean(rows[t, :, 0], axis=0) for t in range(T)])
    assert want.dtype == np.float32 and want_mean.dtype == np.float32
    for t in range(T):
        assert np.isnan(want[t]).all() if t in flat else (want[t].min() == 0 and want[t].max() == 255)
    d = torch.from_numpy(rows).to(dev)
    tag = f"T={T} heads={heads} n_rows={n_rows} P={P}"
    got = run_twice(lib, f"tile_postprocess {tag}",
                    lambda p, sc: lib.ocm_op_tile_postprocess(d.data_ptr(), p["maps"], T, heads, n_rows, P, _s()), {"maps": ((T, P), F32)})
    assert np.array_equal(got["maps"], want, equal_nan=True), tag
    got = run_twice(lib, f"head_mean {tag}",
                    lambda p, sc: lib.ocm_op_head_mean(d.data_ptr(), p["maps"], T, heads, n_rows, P, _s()), {"maps": ((T, P), F32)})
    assert np.array_equal(got["maps"], want_mean), tag


# ---------------------------------------------------------------------------------------------------------------------
# resizes
# ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24  # unit round-off of float32


def bilinear_bound(src, h, w, scale):
    """Per-map bound of test_bilinear_upsample_within_derived_bound, in the units it is derived in."""
    M = np.abs(src).max(axis=(1, 2)).astype(np.float64)
    R = (src.max(axis=(1, 2)) - src.min(axis=(1, 2))).astype(np.float64)
    units = 4 * M
    if scale & (scale - 1):  # 1 / scale is inexact
        units = units + (M + R) + (2 * w + 2 * h + 1) * R
    return units * U * (1 + 2.0 ** -10), M, R


@pytest.mark.parametrize("T,h,w,scale", BILINEAR_SHAPES)
def test_bilinear_upsample_within_derived_bound(dev, lib, T, h, w, scale):
    """ocm_op_bilinear_upsample against oracle.bilinear_upsample_f64 (the same geometry in float64, pinned to double
    F.interpolate on the CPU). With u = 2^-24, M = max|src| and R = max - min of a map, the kernel's rounding points are:

      coordinate  f = fl(fl((X + 0.5) * fl(1 / scale)) - 0.5). X + 0.5 is exact. For a power-of-two scale everything else
                  is too (an exponent shift of a short mantissa). Otherwise fl(1 / scale) and the product each err by <= u
                  relative on a value below the side n, and the subtraction is exact unless the product is below 0.25,
                  where it errs by <= u / 4: |df| <= (2 n + 1/2) u per axis. The kernel takes taps AND weights from
                  this one f, so it evaluates the border-replicated bilinear surface at a shifted point; the surface is
                  continuous and piecewise linear with slope <= R per pixel along either axis (also where floor(f) flips),
                  so the value moves by <= (2 w + 2 h + 1) u R.
      weights     a = f - floor(f) is exact for f >= 0; for f < 0 it errs by <= u / 2 but both taps are the same pixel.
                  1 - a is rounded: <= u / 2. Counted per blend as <= u / 2 * (M + R); the horizontal blends' errors
                  pass through the vertical blend's convex combination once: <= u (M + R). Zero for power-of-two scales.
      blends      each of the three two-term blends rounds two products (<= u * (|p| w0 + |q| w1) <= u M) and one sum
                  (<= u M): 2 u M. The two horizontal ones are averaged by the vertical one: <= 4 u M in all.

    Bound: u * (4 M) for power-of-two scales, u * (4 M + (M + R) + (2 w + 2 h + 1) R) otherwise, times 1 + 2^-10 for the
    second-order terms (products of the above, each below 200 u). At scale 1 every weight is 0 or 1: the source itself."""
    rng = np.random.default_rng(100 * h + w + scale)
    src = (rng.standard_normal((T, h, w)) * 40 + 100).astype(np.float32)
    want = O.bilinear_upsample_f64(src, scale)
    d = torch.from_numpy(src).to(dev)
    got = run_twice(lib, f"bilinear_upsample T={T} {h}x{w} x{scale}",
                    lambda p, sc: lib.ocm_op_bilinear_upsample(d.data_ptr(), p["out"], T, h, w, scale, _s()),
                    {"out": ((T, h * scale, w * scale), F32)})["out"]
    bound, M, R = bilinear_bound(src, h, w, scale)
    err = np.abs(got.astype(np.float64) - want).max(axis=(1, 2))
    worst = int(np.argmax(err / bound))
    print(f"GPUTEST bilinear upsample T={T} {h}x{w} x{scale}: max|d| = {err[worst]:.3e} = {err[worst] / (U * M[worst]):.2f} u*M "
          f"(bound {bound[worst]:.3e} = {bound[worst] / (U * M[worst]):.2f} u*M; M = {M[worst]:.1f}, R = {R[worst]:.1f})")
    assert (err <= bound).all(), (err, bound)
    if scale == 1:
        assert np.array_equal(got, src)


@pytest.mark.parametrize("T,h,w,f", [(2, 6, 10, 1), (2, 6, 10, 2), (1, 9, 15, 3), (3, 8, 12, 4), (1, 16, 48, 16), (9, 512, 512, 1)])
def test_downscale_centre_every_parity(dev, lib, T, h, w, f):
    """ocm_op_downscale_centre == oracle.cv2_downscale bit for bit (the same fp32 operations; contraction is off in the
    kernels' file): odd factors take the centre pixel, even ones the 2 x 2 centre average, horizontal pass first.
    (9, 512, 512, 1) is a copy of 2 359 296 elements, one trip more than the launch's 8192 workgroups hold."""
    rng = np.random.default_rng(10 * h + f)
    src = (rng.standard_normal((T, h, w)) * 3).astype(np.float32)
    want = O.cv2_downscale(src, f)
    assert want.shape == (T, h // f, w // f) and want.dtype == np.float32
    d = torch.from_numpy(src).to(dev)
    got = run_twice(lib, f"downscale_centre T={T} {h}x{w} /{f}",
                    lambda p, sc: lib.ocm_op_downscale_centre(d.data_ptr(), p["out"], T, h, w, f, _s()),
                    {"out": ((T, h // f, w // f), F32)})["out"]
    assert np.array_equal(got, want)


def test_downscale_centre_rejects_partial_blocks(dev, lib):
    src, dst = torch.zeros((1, 9, 16), device=dev), torch.zeros((1, 9, 16), device=dev)
    assert lib.ocm_op_downscale_centre(src.data_ptr(), dst.data_ptr(), 1, 9, 16, 2, _s()) == EINVAL  # h % f
    assert lib.ocm_op_downscale_centre(src.data_ptr(), dst.data_ptr(), 1, 9, 16, 3, _s()) == EINVAL  # w % f
    assert lib.ocm_op_downscale_centre(src.data_ptr(), dst.data_ptr(), 1, 9, 16, 0, _s()) == EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# median filter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def median_edges():
    gold = load_golden("median_edges")
    return gold, median_edge_inputs(int(gold["seed"]))


@pytest.mark.parametrize("size", MEDIAN_EDGE_SIZES)
@pytest.mark.parametrize("which", range(len(MEDIAN_EDGE_SHAPES)), ids=["x".join(map(str, s)) for s in MEDIAN_EDGE_SHAPES])
def test_median_filter_edges_vs_scipy_fixture(dev, lib, median_edges, which, size):
    """ocm_op_median_filter == scipy.ndimage.median_filter's own outputs (tests/golden/median_edges.npz) bit for bit:
    maps of height / width 1, windows reflecting through several periods of the map (size // 2 >= 2 h), the identity
    (size 1), eval.py's size 13, the cap 15 and the even 14; ties planted, no NaN, no signed zeros."""
    gold, maps = median_edges
    x = maps[which]
    T, h, w = x.shape
    want = gold[f"map{which}_size{size}"]
    d = torch.from_numpy(x).to(dev)
    got = run_twice(lib, f"median_filter {T}x{h}x{w} size {size}",
                    lambda p, sc: lib.ocm_op_median_filter(d.data_ptr(), p["out"], T, h, w, size, _s()), {"out": ((T, h, w), F32)})["out"]
    assert np.array_equal(got, want)
    if size == 1:
        assert np.array_equal(got, x)


def test_median_filter_past_one_grid_trip(dev, lib):
    """3 maps of 1024 x 700 at size 3: 2 150 400 outputs against the 8192 x 256 threads of one trip of the grid-stride
    loop, with heavy ties (values on a 1 / 64 grid). Against oracle.median_filter, which tests/test_oracle_golden.py holds
    to scipy (a scipy fixture of this size would not fit the repository)."""
    rng = np.random.default_rng(12)
    x = (rng.integers(1, 65, (3, 1024, 700)) / 64).astype(np.float32)
    want = O.median_filter(x, 3)
    d = torch.from_numpy(x).to(dev)
    got = run_twice(lib, "median_filter 3x1024x700 size 3",
                    lambda p, sc: lib.ocm_op_median_filter(d.data_ptr(), p["out"], 3, 1024, 700, 3, _s()), {"out": ((3, 1024, 700), F32)})["out"]
    assert x.size > 8192 * 256 and np.array_equal(got, want)


def test_median_filter_rejects_aliasing_and_sizes(dev, lib):
    src, dst = torch.zeros((1, 4, 4), device=dev), torch.zeros((1, 4, 4), device=dev)
    assert lib.ocm_op_median_filter(src.data_ptr(), src.data_ptr(), 1, 4, 4, 3, _s()) == EINVAL  # in place: neighbours overwritten
    assert lib.ocm_op_median_filter(src.data_ptr(), dst.data_ptr(), 1, 4, 4, 0, _s()) == EINVAL
    assert lib.ocm_op_median_filter(src.data_ptr(), dst.data_ptr(), 1, 4, 4, 16, _s()) == EINVAL
    assert lib.ocm_op_median_filter(src.data_ptr(), dst.data_ptr(), 1, 4, 4, 15, _s()) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the u8 chain
# ---------------------------------------------------------------------------------------------------------------------
def _heat(count, kind="normal"):
    """A heat map with negative values whose extremes normalise to exactly 0 and 1 (each planted twice where there is
    room); `flat`: one value inside [0, 1] (min_max_normalize returns a flat map unchanged, and numpy leaves the uint8
    conversion of a value outside [0, 255] undefined, so no flat value outside it)."""
    if kind == "flat" or count == 1:
        return np.full(count, 0.625 if kind == "flat" else 0.25, np.float32)
    heat = np.random.default_rng(count).normal(0, 50, count).astype(np.float32)
    heat[[0, count // 2]] = heat.min()
    heat[[1, count - 1]] = heat.max()
    assert heat.min() < 0 < heat.max()
    return heat


def _u8(count, seed):
    return np.random.default_rng(seed + count).integers(0, 256, count, dtype=np.uint8)


HEATS = [(c, "normal") for c in U8_COUNTS] + [(257, "flat")]


@pytest.mark.parametrize("count,kind", HEATS)
def test_normalize_u8_counts(dev, lib, count, kind):
    """ocm_op_normalize_u8 == oracle.heatmap_mask's image ((heat - min) / (max - min) * 255, truncated) bit for bit, on a
    poisoned 2048-byte scratch, at counts far below the 256 x 256 elements the min-max grid is sized for."""
    heat = _heat(count, kind)
    want = O.heatmap_mask(heat)[0]
    if kind == "normal" and count > 1:
        assert want.min() == 0 and want.max() == 255
    d = torch.from_numpy(heat).to(dev)
    got = run_twice(lib, f"normalize_u8 {count} {kind}",
                    lambda p, sc: lib.ocm_op_normalize_u8(d.data_ptr(), count, sc, p["out"], p["hist"], _s()),
                    {"out": ((count,), U8), "hist": ((256,), I64)}, scratch_bytes=2048)
    assert np.array_equal(got["out"], want)
    assert np.array_equal(got["hist"], _hist_of(want)) and int(got["hist"].sum()) == count


def _check_weighted(dev, lib, what, img, heat):
    count = heat.size
    (_, _, _), _, want_res = O.sw_threshold_masks(img, heat)
    want_att = O.heatmap_mask(heat)[0]
    di, dh = torch.from_numpy(img).to(dev), torch.from_numpy(heat).to(dev)
    h = ((256,), I64)
    got = run_twice(lib, what, lambda p, sc: lib.ocm_op_weighted_u8(dh.data_ptr(), di.data_ptr(), count, sc, p["res"], p["att"],
                                                                    p["hres"], p["hatt"], _s()),
                    {"res": ((count,), U8), "att": ((count,), U8), "hres": h, "hatt": h}, scratch_bytes=2048)
    assert np.array_equal(got["res"], want_res), f"{int((got['res'] != want_res).sum())} of {count} results differ"
    assert np.array_equal(got["att"], want_att)
    assert np.array_equal(got["hres"], _hist_of(want_res)) and int(got["hres"].sum()) == count
    assert np.array_equal(got["hatt"], _hist_of(want_att)) and int(got["hatt"].sum()) == count


@pytest.mark.parametrize("count,kind", HEATS)
def test_weighted_u8_counts(dev, lib, count, kind):
    """ocm_op_weighted_u8 == oracle.sw_threshold_masks' result ((img * attention / max(attention)) truncated, float32)
    and the attention image, with both histograms."""
    _check_weighted(dev, lib, f"weighted_u8 {count} {kind}", _u8(count, 1), _heat(count, kind))


def test_weighted_u8_every_level_times_a_heat_ramp(dev, lib):
    """All 256 image levels x a 256-step heat ramp (negative to positive, normalising to 0 .. 1): every float32 product
    the truncation can meet on such a map."""
    ramp = np.arange(256, dtype=np.float32) * np.float32(0.37) - np.float32(11)
    _check_weighted(dev, lib, "weighted_u8 256 levels x 256-step ramp", np.repeat(np.arange(256, dtype=np.uint8), 256), np.tile(ramp, 256))


def _check_blend(dev, lib, what, img, att, alpha):
    count = img.size
    want = ((img / 2) * (1 - alpha) + (att / 2) * alpha).astype(np.uint8)  # utils.py:79-80: float64, truncated
    di, da = torch.from_numpy(img).to(dev), torch.from_numpy(att).to(dev)
    got = run_twice(lib, what, lambda p, sc: lib.ocm_op_blend_u8(di.data_ptr(), da.data_ptr(), count, alpha, 1 - alpha, p["out"],
                                                                 p["hist"], _s()), {"out": ((count,), U8), "hist": ((256,), I64)})
    assert np.array_equal(got["out"], want), f"{int((got['out'] != want).sum())} of {count} differ"
    assert np.array_equal(got["hist"], _hist_of(want)) and int(got["hist"].sum()) == count


def test_blend_u8_all_level_pairs(dev, lib):
    """All 65 536 (image, attention) level pairs at alpha = 0.4 with 1 - alpha as Python computes it: the float64
    formula of utils.py:79-80, truncated. Settles the truncation for good."""
    lv = np.arange(256, dtype=np.uint8)
    _check_blend(dev, lib, "blend_u8 all pairs", np.repeat(lv, 256), np.tile(lv, 256), 0.4)


@pytest.mark.parametrize("count", U8_COUNTS)
def test_blend_histogram_threshold_u8_counts(dev, lib, count):
    """blend_u8, histogram_u8 and threshold_u8 (levels 0, 127, 254, 255; cv2.THRESH_BINARY: > level) at every count."""
    img, att = _u8(count, 2), _u8(count, 3)
    _check_blend(dev, lib, f"blend_u8 {count}", img, att, 0.4)
    img[:: max(1, count // 7)] = np.resize(np.array([0, 127, 128, 254, 255], np.uint8), img[:: max(1, count // 7)].size)
    d = torch.from_numpy(img).to(dev)
    got = run_twice(lib, f"histogram_u8 {count}", lambda p, sc: lib.ocm_op_histogram_u8(d.data_ptr(), count, p["hist"], _s()),
                    {"hist": ((256,), I64)})["hist"]
    assert np.array_equal(got, _hist_of(img)) and int(got.sum()) == count
    for level in (0, 127, 254, 255):
        got = run_twice(lib, f"threshold_u8 {count} level {level}",
                        lambda p, sc: lib.ocm_op_threshold_u8(d.data_ptr(), p["out"], count, level, _s()), {"out": ((count,), U8)})["out"]
        assert np.array_equal(got, np.where(img > level, 255, 0).astype(np.uint8)), level


def _check_gray(dev, lib, what, img, strided):
    chans, count = img.shape
    want = O.to_pil_gray_u8(img.reshape(chans, 1, count))[0]
    if strided:
        big = torch.full((chans, count + 7), float("nan"), device=dev)
        d = big[:, :count]
        d.copy_(torch.from_numpy(img))
    else:
        d = torch.from_numpy(img).to(dev)
    got = run_twice(lib, what, lambda p, sc: lib.ocm_op_image_to_gray_u8(d.data_ptr(), d.stride(0), chans, count, p["out"], p["hist"], _s()),
                    {"out": ((count,), U8), "hist": ((256,), I64)})
    assert np.array_equal(got["out"], want), f"{int((got['out'] != want).sum())} of {count} differ"
    assert np.array_equal(got["hist"], _hist_of(want)) and int(got["hist"].sum()) == count


@pytest.mark.parametrize("count", U8_COUNTS)
def test_image_to_gray_u8_counts(dev, lib, count):
    """ocm_op_image_to_gray_u8 == oracle.to_pil_gray_u8 (mul(255) truncated, PIL's integer "L") with 1 and 3 planes."""
    img = np.random.default_rng(count).random((3, count), dtype=np.float32)
    _check_gray(dev, lib, f"image_to_gray_u8 {count} 3 planes", img, False)
    _check_gray(dev, lib, f"image_to_gray_u8 {count} 1 plane", img[1:2].copy(), False)


@pytest.mark.parametrize("strided", [False, True])
def test_image_to_gray_u8_every_level_per_channel(dev, lib, strided):
    """A (3, 256, 256) image with R = row / 255, G = column / 255 and B a random permutation of the levels: every (R, G)
    pair with unrelated B, so each channel's weight and plane offset is visible; `strided` takes it through a view whose
    channel stride exceeds the pixel count (NaN in the gap)."""
    lv = np.arange(256, dtype=np.float32) / np.float32(255)
    r = np.repeat(lv[:, None], 256, 1)
    g = np.repeat(lv[None, :], 256, 0)
    b = lv[np.random.default_rng(5).permutation(256 * 256) % 256].reshape(256, 256)
    img = np.stack([r, g, b]).reshape(3, -1)
    planes = img.reshape(3, 256, 256)
    want = O.to_pil_gray_u8(planes)
    for order in ([0, 2, 1], [1, 0, 2], [2, 1, 0]):  # no two channels are interchangeable on this image
        assert (O.to_pil_gray_u8(planes[order]) != want).mean() > 0.9
    _check_gray(dev, lib, f"image_to_gray_u8 level planes strided={strided}", img, strided)
