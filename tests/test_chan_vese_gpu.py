"""ocm_op_chan_vese (kernels_levelset.hip) and its Python surface against the float64 numpy restatement tests/chan_vese_ref.py.
Every case is a batch of three different images. Needs an MI355X.

Tolerances:
  one step     max |phi - ref| <= 1e-13: both sides evaluate the same float64 expression on the same inputs, the sharp Heaviside
               makes the counts exact; what differs is the summation order of c1 / c2 (a few ulp on values of order 1).
  few steps    FEW_STEPS_BOUND = 16 x the maximum measured over every case of test_few_steps (MEASURED_FEW_STEPS): a
               2e-16 perturbation of c1 / c2 grows by about 1.15 x per step. Above 1e-9 something other than rounding differs.
  full runs    masks agree on every pixel with |phi_ref| >= band, band = 16 x the measured final max |phi - phi_ref| of that case
               (MEASURED_FULL), at least 1e-12; iters equal the reference's.
Measured on an MI355X: one step at most 2.2e-16; 7 / 8 steps at most 2.442e-15 (the 67 x 97 random start; the bound is
3.9e-14); the chunked run at most 1.010e-14 over its 13 restarts; the final differences of the full runs are in MEASURED_FULL
(on the CPU, the restatement against itself with one-ulp changes of the start ends 1e-11 .. 3e-9 apart on the same images).
Every test prints its figures before it asserts them."""
import numpy as np
import pytest
import torch

from tests import chan_vese_ref as R
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import utils

pytestmark = pytest.mark.gpu

T = 32  # ocm_chan_vese_tile()
SHAPES = [(1, 1), (5, 7), (T - 1, T + 1), (2 * T + 3, 3 * T + 1), (37, 53)]
ONE_STEP_BOUND = 1e-13
MEASURED_FEW_STEPS = 2.442e-15  # measured maximum over test_few_steps (7 and 8 steps, every shape and start)
FEW_STEPS_BOUND = 16 * MEASURED_FEW_STEPS
ROUNDING_CEILING = 1e-9  # a difference above this is not rounding
# final max |phi - phi_ref| of the runs to convergence, measured; the band of a case is 16 x its value (at least 1e-12)
MEASURED_FULL = {(9, 9): 2.119e-11, (37, 53): 2.612e-11, (96, 96): 1.828e-09, "flat": 6.763e-12}
FULL_SEEDS = {(9, 9): (6, 10, 25), (37, 53): (7, 9, 6), (96, 96): (0, 6, 1)}  # different stopping iterations, both parities


def band_of(key):
    return max(16 * MEASURED_FULL[key], 1e-12)


SURFACE_BAND = max(band_of(k) for k in MEASURED_FULL)


def trio(h, w, start):
    """Three different images of one size with their starts: blobs, noise and the two-level step. -> [(img, phi0)] * 3"""
    out = []
    for kind, seed in (("blobs", 3), ("noise", 5), ("step", 0)):
        img = {"blobs": R.blobs, "noise": R.noise}[kind](h, w, seed) if kind != "step" else R.step_image(h, w)
        out.append((img, R.checkerboard(h, w) if start == "checkerboard" else R.random_start(h, w, 100 + seed)))
    return out


def run(dev, imgs, phi0s=None, **kw):
    """utils.chan_vese_level_set on a batch -> (phi, mask, iters) as numpy. phi0s None: the checkerboard built by the package."""
    x = torch.from_numpy(np.stack(imgs)).to(dev)
    init = "checkerboard" if phi0s is None else torch.from_numpy(np.stack(phi0s)).to(dev)
    mask, iters, phi = utils.chan_vese_level_set(x, init_level_set=init, return_phi=True, **kw)
    assert mask.dtype == torch.bool and iters.dtype == torch.int32 and phi.dtype == torch.float64
    return phi.cpu().numpy(), mask.cpu().numpy(), iters.cpu().numpy()


@pytest.mark.parametrize("start", ["checkerboard", "random"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_one_step(dev, h, w, start):
    cases = trio(h, w, start)
    phi, mask, iters = run(dev, [c[0] for c in cases], None if start == "checkerboard" else [c[1] for c in cases], max_num_iter=1)
    err = 0.0
    for b, (img, phi0) in enumerate(cases):
        ref = R.evolve(R.normalize(img), phi0, max_num_iter=1)
        err = max(err, float(np.abs(phi[b] - ref["phi"]).max()))
        assert np.array_equal(mask[b], ref["mask"]) and np.array_equal(mask[b], phi[b] > 0), b
    print(f"one step {h}x{w} {start}: max |phi - ref| = {err:.3e}")
    assert err <= ONE_STEP_BOUND
    assert iters.tolist() == [1, 1, 1]


@pytest.mark.parametrize("steps", [7, 8])
@pytest.mark.parametrize("start", ["checkerboard", "random"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_few_steps(dev, h, w, start, steps):
    cases = trio(h, w, start)
    phi, mask, iters = run(dev, [c[0] for c in cases], None if start == "checkerboard" else [c[1] for c in cases],
                           max_num_iter=steps, tol=0.0)
    err, want_iters = 0.0, []
    for b, (img, phi0) in enumerate(cases):
        ref = R.evolve(R.normalize(img), phi0, max_num_iter=steps, tol=0.0)
        assert ref["iters"] == steps or h * w == 1  # a single pixel can stand still: phivar == 0 ends the loop even at tol 0
        want_iters.append(ref["iters"])
        err = max(err, float(np.abs(phi[b] - ref["phi"]).max()))
        assert np.array_equal(mask[b], phi[b] > 0)
    print(f"few steps {steps} {h}x{w} {start}: max |phi - ref| = {err:.3e}")
    assert FEW_STEPS_BOUND <= ROUNDING_CEILING
    assert err <= FEW_STEPS_BOUND
    assert iters.tolist() == want_iters


def test_chunked_long_run(dev):
    """96 x 96: the device restarts every 10 iterations from the reference's own phi and must land on the reference 10
    iterations later (or at its convergence, when that comes first, with the iteration count to match)."""
    h = w = 96
    refs = [R.cached("blobs", h, w, s) for s in FULL_SEEDS[(h, w)]]
    errs, counts = [], []
    for j in range(0, max(r[2]["iters"] for r in refs), 10):
        js = [min(j, 10 * ((r[2]["iters"] - 1) // 10)) for r in refs]  # a finished image repeats its last chunk
        phi, mask, iters = run(dev, [r[0] for r in refs], [r[2]["phis"][jb] for r, jb in zip(refs, js)], max_num_iter=10)
        ends = [min(jb + 10, r[2]["iters"]) for r, jb in zip(refs, js)]
        errs.append([float(np.abs(phi[b] - r[2]["phis"][end]).max()) for b, (r, end) in enumerate(zip(refs, ends))])
        counts.append((iters.tolist(), [end - jb for end, jb in zip(ends, js)]))
    print("chunked long run, max |phi - ref| per restart and image:")
    for j, e in enumerate(errs):
        print(f"  from iteration {10 * j}: " + " ".join(f"{v:.3e}" for v in e))
    print(f"chunked long run: max |phi - ref| over all restarts = {max(map(max, errs)):.3e}")
    for got, want in counts:
        assert got == want
    assert max(map(max, errs)) <= FEW_STEPS_BOUND


def check_reference_conditions(refs, band, excluded=0.01):
    """What the full-run comparison relies on, asserted on the reference alone: at most `excluded` of the pixels inside the
    band, no phivar within a relative 1e-6 of tol."""
    its = [r["iters"] for r in refs]
    for r in refs:
        assert np.mean(np.abs(r["phi"]) < band) <= excluded
        pv = np.array(r["phivars"])
        assert np.min(np.abs(pv - 1e-3) / 1e-3) > 1e-6
    return its


@pytest.mark.parametrize("h,w", list(FULL_SEEDS))
def test_full_run_to_convergence(dev, h, w):
    refs = [R.cached("blobs", h, w, s) for s in FULL_SEEDS[(h, w)]]
    band = band_of((h, w))
    its = check_reference_conditions([r[2] for r in refs], band)
    assert len(set(its)) == 3 and len({i & 1 for i in its}) == 2 and max(its) < 200, its
    phi, mask, iters = run(dev, [r[0] for r in refs])
    err = max(float(np.abs(phi[b] - r[2]["phi"]).max()) for b, r in enumerate(refs))
    print(f"full run {h}x{w}: iters {iters.tolist()} (reference {its}), final max |phi - ref| = {err:.3e}, band {band:.3e}")
    assert iters.tolist() == its
    for b, r in enumerate(refs):
        keep = np.abs(r[2]["phi"]) >= band
        assert np.array_equal(mask[b][keep], r[2]["mask"][keep]), b
        assert np.array_equal(mask[b], phi[b] > 0)
    assert err <= band


def test_cap_reached_and_zero_iterations(dev):
    h, w = 37, 53
    refs = [R.cached("step", h, w, 0)] + [R.cached("blobs", h, w, s) for s in (1, 7)]
    assert refs[0][2]["iters"] == 200 and all(25 < r[2]["iters"] < 200 for r in refs[1:])  # the step image never converges
    imgs = [r[0] for r in refs]
    phi, mask, iters = run(dev, imgs, max_num_iter=25)
    err = max(float(np.abs(phi[b] - r[2]["phis"][25]).max()) for b, r in enumerate(refs))
    print(f"cap 25: iters {iters.tolist()}, max |phi - ref| = {err:.3e}")
    assert iters.tolist() == [25, 25, 25]
    assert err <= ROUNDING_CEILING  # 25 steps of rounding-only growth stay far below what a real difference gives
    # the cap on one image while the others stop on their own
    phi, mask, iters = run(dev, imgs)
    print(f"cap 200: iters {iters.tolist()}")
    assert iters.tolist() == [r[2]["iters"] for r in refs]
    assert np.array_equal(mask[0], refs[0][2]["mask"])  # the edge at the step: no pixel of this run is near zero
    assert np.abs(refs[0][2]["phi"]).min() > 1e-3
    # max_num_iter = 0: phi comes back untouched
    starts = [R.random_start(h, w, 40 + b) for b in range(3)]
    phi, mask, iters = run(dev, imgs, starts, max_num_iter=0)
    assert iters.tolist() == [0, 0, 0]
    assert np.array_equal(phi, np.stack(starts)) and np.array_equal(mask, np.stack(starts) > 0)


def test_flat_image(dev):
    h, w = 37, 53
    refs = [R.cached("flat", h, w, 0), R.cached("blobs", h, w, 9), R.cached("noise", h, w, 1)]
    band = band_of("flat")
    # the flat image normalises to zero: no data term, the checkerboard only diffuses, and a third of its pixels end within
    # 1e-9 of zero (the zero lines of the start stay zero lines); the mask rule holds on the others
    its = check_reference_conditions([r[2] for r in refs[1:]], band) and [r[2]["iters"] for r in refs]
    check_reference_conditions([refs[0][2]], band, excluded=1.0)
    assert not R.normalize(refs[0][0]).any()
    phi, mask, iters = run(dev, [r[0] for r in refs])
    err = max(float(np.abs(phi[b] - r[2]["phi"]).max()) for b, r in enumerate(refs))
    print(f"flat batch: iters {iters.tolist()} (reference {its}), final max |phi - ref| = {err:.3e}, band {band:.3e}")
    assert np.isfinite(phi).all()
    assert iters.tolist() == its
    for b, r in enumerate(refs):
        keep = np.abs(r[2]["phi"]) >= band
        assert np.array_equal(mask[b][keep], r[2]["mask"][keep]), b
    assert err <= band


def test_two_runs_give_the_same_bits(dev):
    h, w = 2 * T + 3, 3 * T + 1
    x = torch.from_numpy(np.stack([R.blobs(h, w, 2), R.noise(h, w, 4), R.flat(h, w)])).to(dev)
    a = utils.chan_vese_level_set(x, return_phi=True)
    b = utils.chan_vese_level_set(x, return_phi=True)
    torch.cuda.synchronize()
    for name, u, v in zip(("mask", "iters", "phi"), a, b):
        assert_same_bits(u, v, f"{name}: first vs second call")
    assert len(set(a[1].cpu().tolist())) > 1  # the images stopped at different iterations


# ---- the Python surface ------------------------------------------------------------------------------------------------------------
def _expected_masks(gray, result, band):
    """The restatement on the device's own uint8 images -> [(mask, keep)] for (result, gray)."""
    out = []
    for img in (result, gray):
        r = R.chan_vese(img)
        out.append((r["mask"], np.abs(r["phi"]) >= band))
    return out


def _check_pair(got, gray, att, res_dev):
    want_res = (gray * att / np.max(att)).astype(np.uint8)  # utils.py:202-208: uint8 * float32 / float32 -> float32, truncated
    assert want_res.dtype == np.uint8 and np.array_equal(res_dev, want_res)
    for g, (m, keep) in zip(got, _expected_masks(gray, res_dev, SURFACE_BAND)):
        assert g.dtype == np.uint8 and set(np.unique(g)) <= {0, 255}
        assert keep.mean() >= 0.99
        assert np.array_equal((g > 0)[keep], m[keep])


def _images(B, S, seed):
    g = np.stack([R.blobs(S, S, seed + b) for b in range(B)]).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(np.repeat(g[:, None], 3, axis=1))


def test_utils_chan_vese(dev):
    from oracle import vit_oracle as O
    S = 48
    img = _images(1, S, 0)[0]
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    att = (0.02 + np.exp(-((yy - 20) ** 2 + (xx - 30) ** 2) / 200.0)).astype(np.float32)
    x, a = torch.from_numpy(img).to(dev), torch.from_numpy(att).to(dev)
    gray = utils.image_to_gray_u8(x)[0]
    assert np.array_equal(gray.cpu().numpy(), O.to_pil_gray_u8(img))
    res_dev = utils.chan_vese_result_u8(gray, a).cpu().numpy()
    got = utils.chan_vese(x, a)
    _check_pair(got, gray.cpu().numpy(), att, res_dev)
    on_dev = utils.chan_vese(gray, a, as_numpy=False)  # a uint8 image is taken as it is
    assert all(np.array_equal(t.cpu().numpy(), g) for t, g in zip(on_dev, got))
    with pytest.raises(NotImplementedError):
        utils.chan_vese(x, a, save=True)
    with pytest.raises(ValueError):
        utils.chan_vese(x, a[:-1])


@pytest.mark.parametrize("layout", ["images", "crops"])
def test_chan_vese_segment(dev, layout):
    from oracle import vit_oracle as O
    from tests.helpers import CASES, build_module
    from vit_ocm_wmsegmentation_amd import eval as E
    model = build_module(CASES["tiny_p8"], dev)
    B, s = 2, 48
    if layout == "images":
        x = torch.from_numpy(_images(B, s, 20)).to(dev)
        gray_src = x
    else:
        x = torch.from_numpy(_images(B * 4, s, 30)).reshape(B, 4, 3, s, s).to(dev)
        gray_src = E.tile_crops_image(x)
    maps = E.average_attention_maps(model, x).cpu().numpy()
    S = maps.shape[-1]
    assert S == (s if layout == "images" else 2 * s)
    ours, maps2 = E.chan_vese_segment(model, x, method="chan-vese_ours", as_numpy=True)
    plain, _ = E.chan_vese_segment(model, x, method="chan-vese")
    assert np.array_equal(maps2, maps) and ours.shape == (B, S, S) and plain.dtype == torch.uint8 and plain.is_cuda
    for b in range(B):
        gray = utils.image_to_gray_u8(gray_src[b])[0]
        assert np.array_equal(gray.cpu().numpy(), O.to_pil_gray_u8(gray_src[b].cpu().numpy()))
        res_dev = utils.chan_vese_result_u8(gray, torch.from_numpy(maps[b]).to(dev)).cpu().numpy()
        _check_pair((ours[b], plain[b].cpu().numpy()), gray.cpu().numpy(), maps[b], res_dev)
