"""Pixel k-means on the device (kernels_kmeans_px.hip, utils.kmeans_pixels / kmeans, eval.kmeans_pixels_segment with the methods
"k-means" / "k-means_ours") against the numpy restatement tests/kmeans_px_ref.py fed the same uniforms. Exactly equal: labels,
centres (as bits), the iteration count of every attempt, the best attempt and the mask. The compactness is a float64 sum in
another fixed order than numpy's: rtol 1e-12 while the reference's two summation orders agree to 2.5e-13, else 4 x their spread
(the rule of tests/test_cluster_shapes_gpu.py). Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kmeans_px_ref as R
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import _lib, utils

pytestmark = pytest.mark.gpu

T = 512     # the workgroup size (tests/test_kmeans_px_host.py asserts it against the source)
CHUNK = 16  # samples a thread takes at a time: N < 16 is all tail, a thread takes a second chunk from N = 16 T + 16 on


def run_op(dev, problems, uniforms, max_iter=10, eps=1.0):
    """ocm_op_kmeans_px on `problems` (P, 3 N) uint8 and `uniforms` (P, A, 2, 3) -> dict of numpy arrays."""
    lib = _lib.load()
    px = torch.from_numpy(np.ascontiguousarray(problems)).to(dev)
    P, n3 = px.shape
    N, A = n3 // 3, uniforms.shape[1]
    u = torch.from_numpy(np.ascontiguousarray(uniforms, np.float32)).to(dev)
    out = dict(labels=torch.empty((P, N), dtype=torch.uint8, device=dev), centers=torch.empty((P, 2, 3), dtype=torch.float32, device=dev),
               compactness=torch.empty((P, A), dtype=torch.float64, device=dev), iters=torch.empty((P, A), dtype=torch.int32, device=dev),
               best=torch.empty(P, dtype=torch.int32, device=dev), mask=torch.empty((P, n3), dtype=torch.uint8, device=dev))
    nbytes = lib.ocm_kmeans_px_workspace_bytes(P, N, A)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.ocm_op_kmeans_px(px.data_ptr(), P, N, u.data_ptr(), A, max_iter, eps, *(out[k].data_ptr() for k in
                              ("labels", "centers", "compactness", "iters", "best", "mask")), ws.data_ptr(), nbytes,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ocm_last_error().decode()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_problem(got, p, ref, what, decided=True):
    """Problem p of a device result against its restatement."""
    runs = ref["attempts"]
    assert got["iters"][p].tolist() == [r["iters"] for r in runs], what
    for a, r in enumerate(runs):
        rtol = R.compactness_rtol(r)
        g, w = float(got["compactness"][p, a]), r["compactness"]
        print(f"{what} attempt {a}: compactness {g!r} (restatement {w!r}), rtol {rtol:.2e}, {r['iters']} iterations")
        assert abs(g - w) <= rtol * abs(w), (what, a, g, w)
    if decided and len(runs) > 1:
        R.assert_best_is_decided(ref)
    assert int(got["best"][p]) == ref["best"], what
    assert np.array_equal(got["labels"][p], ref["labels"]), what
    assert np.array_equal(got["centers"][p].view(np.uint32), ref["centers"].view(np.uint32)), (what, got["centers"][p], ref["centers"])
    assert np.array_equal(got["mask"][p], ref["mask"]), what


def check_batch(dev, lib, problems, attempts, what, state=R.RNG_START, **kw):
    problems = np.stack(problems)
    u, _ = R.uniforms_for(len(problems), attempts, state)
    got = run_op(dev, problems, u, **kw)
    refs = [R.segment(px, u[p], lib, **kw) for p, px in enumerate(problems)]
    for p, ref in enumerate(refs):
        check_problem(got, p, ref, f"{what}[{p}]")
    return got, refs


# N < 16: element accesses only; 16 T: one whole chunk per thread; 16 T + 17: a second chunk and a tail; 2 x 16 T + 21: a third
SHAPES = [2, 3, 15, 16, 17, 63, 65, T - 1, T, T + 1, 4 * T + 5, CHUNK * T - 1, CHUNK * T, CHUNK * T + 17, 2 * CHUNK * T + 21]


@pytest.mark.parametrize("n", SHAPES)
def test_shapes(dev, lib, n):
    """Three problems per shape: with an N that is no multiple of 16 the second and third start unaligned."""
    got, refs = check_batch(dev, lib, [R.plateaus(n, n), R.noise(n, n + 1), R.plateaus(n, n + 2)], 3, f"N={n}")
    if n >= 63:
        assert refs[1]["iters"].max() > refs[0]["iters"].max()  # the noise runs longer than the plateaus


@pytest.mark.parametrize("problems", [1, 2, 5])
@pytest.mark.parametrize("attempts", [1, 3, 10])
def test_problem_and_attempt_counts(dev, lib, problems, attempts):
    n = 4 * T + 5  # odd: problem p starts at byte 3 p N, aligned for p = 0 only
    makers = [R.plateaus, R.noise, R.bright, R.noise, R.plateaus]
    check_batch(dev, lib, [makers[p](n, 10 * attempts + p) for p in range(problems)], attempts, f"P={problems} A={attempts}")


def test_noise_reaches_the_cap(dev, lib):
    n = 128 * 128 // 3 + 1
    got, refs = check_batch(dev, lib, [R.noise(n, 7)], 10, "noise")
    assert got["iters"].max() == 10 and len(set(got["compactness"][0].tolist())) == 10
    got, refs = check_batch(dev, lib, [R.noise(n, 7), R.plateaus(n, 8)], 3, "max_iter 1 runs two passes", max_iter=1)
    assert got["iters"].tolist() == [[2] * 3] * 2
    check_batch(dev, lib, [R.noise(n, 7), R.plateaus(n, 8)], 3, "eps 0", max_iter=25, eps=0.0)


def test_sums_beyond_2_to_24(dev, lib):
    """450 x 450 pixels near 255: N = 67 500 and column sums of 1.6e7 .. 1.7e7, past 2^24, where a sequential float32 sum would
    round along the way; the integer sums stay exact and round once."""
    px = R.bright(450 * 450 // 3, 3)
    assert px.reshape(-1, 3).astype(np.int64).sum(0).max() > 1 << 24
    check_batch(dev, lib, [px], 3, "bright 450x450")


@pytest.mark.parametrize("value", [200, 0, 255, 7])
def test_constant_image(dev, lib, value):
    """Both centres start equal, every label is 0: each attempt relocates the last sample at iteration 1 and stops at 2."""
    n = 4 * T + 5
    got, refs = check_batch(dev, lib, [R.constant(n, value), R.constant(n, value)], 10, f"constant {value}")
    for r in refs:
        assert all(a["relocations"] == [1] for a in r["attempts"])
    assert got["iters"].tolist() == [[2] * 10] * 2 and got["best"].tolist() == [0, 0]
    assert got["labels"][0].tolist() == [0] * (n - 1) + [1]
    assert np.array_equal(got["centers"], np.full((2, 2, 3), value, np.float32))
    assert np.array_equal(got["mask"], np.full((2, 3 * n), 255 if value else 0, np.uint8))


@pytest.mark.parametrize("n,low_at,high_at", [(4, 0, 3), (4, 3, 0), (1024, 5, 900), (1024, 900, 5), (8192, 4100, 77), (8192, 1, 8191),
                                            (16384, 9000, 300)])
@pytest.mark.parametrize("swap", [False, True])
def test_relocation_takes_the_larger_index_on_a_tie(dev, lib, n, low_at, high_at, swap):
    """A hand-made start: one centre outside the data, so its cluster is empty at iteration 1 on non-constant data whose two
    farthest samples lie at one distance (300.0) from the exact mean (10, 10, 10), in different threads and waves."""
    u = np.array([[0.32, 0.32, 0.32], [0.0, 0.0, 0.0]], np.float32)
    u = (u[::-1] if swap else u).reshape(1, 1, 2, 3)
    px = R.tie_case(n, low_at, high_at)
    ref = R.segment(px, u[0], lib)
    assert ref["attempts"][0]["relocations"] == [1]
    assert np.flatnonzero(ref["labels"] == (0 if swap else 1)).tolist() == [max(low_at, high_at)]
    check_problem(run_op(dev, px[None], u), 0, ref, f"tie N={n} swap={swap}")


def test_alone_and_inside_a_batch(dev, lib):
    """A problem gives the same bits alone, first in a batch and at an unaligned place inside one."""
    n, A = CHUNK * T + 17, 3
    imgs = [R.noise(n, 1), R.plateaus(n, 2), R.noise(n, 3), R.bright(n, 4)]
    u, _ = R.uniforms_for(len(imgs), A)
    batch = run_op(dev, np.stack(imgs), u)
    for p in range(len(imgs)):
        alone = run_op(dev, imgs[p][None], u[p:p + 1])
        for k in batch:  # compared as bytes: the floats bit for bit
            assert np.ascontiguousarray(alone[k][0]).tobytes() == np.ascontiguousarray(batch[k][p]).tobytes(), (k, p)
    again = run_op(dev, np.stack(imgs), u)
    for k in batch:
        assert np.array_equal(batch[k].view(np.uint8), again[k].view(np.uint8)), k


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_kmeans_pixels(dev, lib):
    H, W = 33, 47  # 1551 pixels = 517 triples: rows do not hold whole samples
    imgs = np.stack([R.plateaus(H * W // 3, 1), R.noise(H * W // 3, 2)]).reshape(2, H, W)
    x = torch.from_numpy(imgs).to(dev)
    state = 0x0123456789abcdef
    r = utils.kmeans_pixels(x, rng_state=state)
    u, end = R.uniforms_for(2, 10, state)
    assert r["rng_state"] == end == utils.cv_rng_uniform(state, 120)[1]  # the host generator's state after P * attempts * 6 draws
    assert r["mask"].shape == (2, H, W) and r["labels"].shape == (2, H * W // 3) and r["centers"].shape == (2, 2, 3)
    assert r["compactness"].shape == (2, 10) and r["iters"].dtype == torch.int32 and r["best"].shape == (2,)
    got = {k: v.cpu().numpy() for k, v in r.items() if k != "rng_state"}
    got["mask"] = got["mask"].reshape(2, -1)
    for p in range(2):
        check_problem(got, p, R.segment(imgs[p].reshape(-1), u[p], lib), f"kmeans_pixels[{p}]")
    # the second problem consumed the second half of the stream: alone, from the state after the first, it gives the same
    mid = R.uniforms_for(1, 10, state)[1]
    one = utils.kmeans_pixels(x[1], rng_state=mid)
    assert one["rng_state"] == end and one["mask"].shape == (H, W) and one["best"].dim() == 0
    assert torch.equal(one["mask"], r["mask"][1]) and torch.equal(one["labels"], r["labels"][1])
    few = utils.kmeans_pixels(x, rng_state=state, attempts=3, max_iter=4, eps=0.5)
    u3, end3 = R.uniforms_for(2, 3, state)
    assert few["rng_state"] == end3 and int(few["iters"].max()) <= 4
    want = R.segment(imgs[1].reshape(-1), u3[1], lib, max_iter=4, eps=0.5)
    assert np.array_equal(few["mask"][1].cpu().numpy().reshape(-1), want["mask"])
    with pytest.raises(ValueError):
        utils.kmeans_pixels(x.float())
    with pytest.raises(ValueError):
        utils.kmeans_pixels(x, attempts=0)


def _images(B, S, seed):
    from tests import chan_vese_ref as CV
    g = np.stack([CV.blobs(S, S, seed + b) for b in range(B)]).astype(np.float32) / np.float32(255)
    return np.ascontiguousarray(np.repeat(g[:, None], 3, axis=1))


def _expected_pair(gray, res_dev, lib, state):
    """The restatement on the device's own uint8 images: (res_ours, res) and the state after, "ours" drawing first."""
    u, end = R.uniforms_for(2, 10, state)
    return [R.segment(img.reshape(-1), u[k], lib)["mask"].reshape(gray.shape) for k, img in enumerate((res_dev, gray))], end


def test_utils_kmeans(dev, lib):
    from oracle import vit_oracle as O
    S = 48
    img = _images(1, S, 0)[0]
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    att = (0.02 + np.exp(-((yy - 20) ** 2 + (xx - 30) ** 2) / 200.0)).astype(np.float32)
    x, a = torch.from_numpy(img).to(dev), torch.from_numpy(att).to(dev)
    gray = utils.image_to_gray_u8(x)[0]
    assert np.array_equal(gray.cpu().numpy(), O.to_pil_gray_u8(img))
    res_dev = utils.chan_vese_result_u8(gray, a).cpu().numpy()
    assert np.array_equal(res_dev, (gray.cpu().numpy() * att / np.max(att)).astype(np.uint8))  # utils.py:121-127
    state = 0xfeedfacecafebeef
    got = utils.kmeans(x, a, rng_state=state)
    want, end = _expected_pair(gray.cpu().numpy(), res_dev, lib, state)
    for g, w in zip(got, want):
        assert g.dtype == np.uint8 and g.shape == (S, S) and np.array_equal(g, w)
    assert len(np.unique(got[1])) == 2
    on_dev = utils.kmeans(gray, a, as_numpy=False, rng_state=state)  # a uint8 image is taken as it is
    assert all(t.is_cuda and np.array_equal(t.cpu().numpy(), g) for t, g in zip(on_dev, got))
    # rng_state=None chains the module's state, as OpenCV's thread-local generator runs on from call to call
    utils._cv_rng_state = state
    first = utils.kmeans(x, a)
    assert utils._cv_rng_state == end and all(np.array_equal(f, g) for f, g in zip(first, got))
    second = utils.kmeans(x, a)
    want2, end2 = _expected_pair(gray.cpu().numpy(), res_dev, lib, end)
    assert utils._cv_rng_state == end2 and all(np.array_equal(s, w) for s, w in zip(second, want2))
    utils.kmeans(x, a, rng_state=state)
    assert utils._cv_rng_state == end2  # an explicit state leaves the chained one alone
    with pytest.raises(NotImplementedError):
        utils.kmeans(x, a, save=True)
    with pytest.raises(ValueError):
        utils.kmeans(x, a[:-3])


@pytest.fixture(scope="module")
def model(dev):
    from tests.helpers import CASES, build_module
    return build_module(CASES["tiny_p8"], dev)


def _expected_batch(E, model, x, lib, state, median_filter):
    """The restatement on the device's own maps and gray images, in the reference's loop order: ours_0, image_0, ours_1, ..."""
    maps = E.average_attention_maps(model, x, median_filter)
    gray_src = E.tile_crops_image(x) if x.dim() == 5 else x
    B = x.shape[0]
    u, end = R.uniforms_for(2 * B, 10, state)
    ours, plain = [], []
    for b in range(B):
        gray = utils.image_to_gray_u8(gray_src[b])[0]
        res = utils.chan_vese_result_u8(gray, maps[b]).cpu().numpy()
        gray = gray.cpu().numpy()
        ours.append(R.segment(res.reshape(-1), u[2 * b], lib)["mask"].reshape(gray.shape))
        plain.append(R.segment(gray.reshape(-1), u[2 * b + 1], lib)["mask"].reshape(gray.shape))
    return {"k-means_ours": np.stack(ours), "k-means": np.stack(plain)}, maps, end


@pytest.mark.parametrize("layout,s,median_filter", [("images", 48, 1), ("images", 96, 3), ("crops", 48, 1), ("crops", 48, 3)])
def test_kmeans_pixels_segment(dev, lib, model, layout, s, median_filter):
    from vit_ocm_wmsegmentation_amd import eval as E
    B = 2
    if layout == "images":
        x = torch.from_numpy(_images(B, s, 20)).to(dev)
    else:
        x = torch.from_numpy(_images(B * 4, s, 30)).reshape(B, 4, 3, s, s).to(dev)
    state = 0x1357924680acebdf
    want, maps, end = _expected_batch(E, model, x, lib, state, median_filter)
    S = s if layout == "images" else 2 * s
    for method in E.KMEANS_PIXELS:
        masks, maps2 = E.kmeans_pixels_segment(model, x, method=method, median_filter=median_filter, rng_state=state)
        assert masks.dtype == torch.uint8 and masks.is_cuda and masks.shape == (B, S, S) and torch.equal(maps2, maps)
        assert np.array_equal(masks.cpu().numpy(), want[method]), method
        assert len(np.unique(want[method])) == 2
    utils._cv_rng_state = state
    as_np, _ = E.kmeans_pixels_segment(model, x, method="k-means", median_filter=median_filter, as_numpy=True)
    assert utils._cv_rng_state == end and isinstance(as_np, np.ndarray) and np.array_equal(as_np, want["k-means"])


@pytest.mark.parametrize("method", ["k-means", "k-means_ours"])
def test_score_images_and_validate(dev, lib, model, method):
    from vit_ocm_wmsegmentation_amd import eval as E
    xa, xb = torch.from_numpy(_images(2, 48, 20)).to(dev), torch.from_numpy(_images(3, 48, 40)).to(dev)
    ta, tb = (xa[:, 0] > 0.5).float(), (xb[:, :1] > 0.5).to(torch.uint8)  # (B,S,S) and (B,1,S,S)
    state = 0x0fedcba987654321
    want_a, _, mid = _expected_batch(E, model, xa, lib, state, 1)
    want_b, _, end = _expected_batch(E, model, xb, lib, mid, 1)
    utils._cv_rng_state = state
    scores, masks, maps = E.score_images(model, xa, ta, method=method)
    assert utils._cv_rng_state == mid and np.array_equal(masks.cpu().numpy(), want_a[method])
    assert_same_bits(scores.view(torch.int64), utils.mask_scores(masks, ta)[0].view(torch.int64), "score_images vs mask_scores")
    # validate chains the generator from batch to batch, as the reference's loop over the dataset does
    utils._cv_rng_state = state
    acc, f1, loss, means = E.validate(model, [(xa, ta), (xb, tb)], method=method)
    assert utils._cv_rng_state == end and means["images"] == 5
    per_image = torch.cat([utils.mask_scores(torch.from_numpy(w[method]).to(dev), t)[0] for w, t in ((want_a, ta), (want_b, tb))])
    per_image = per_image.cpu().numpy()
    for k, name in enumerate(utils.SCORE_NAMES):  # float64 sums of five values in [0, 1] in another order: a few 2^-53
        assert abs(means[name] - np.nanmean(per_image[:, k])) <= 8 * 2.0 ** -53, name
    assert (acc, f1, loss) == (means["accuracy"], means["f1"], means["dice_loss"])
