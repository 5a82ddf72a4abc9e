"""The k-means kernels (kernels_cluster.hip) at every shape class they dispatch on: each `kdist_kernel<CPL, K>` /
`lloyd_kernel<CPL, ASSIGN>` instantiation with full and partial last chunks, the row splits past their block and chunk caps,
the grid-stride loop of `kfeat_kernel` and the status outputs at non-trivial values. Distances and sums against direct
float64 numpy, the feature map against CPU F.interpolate, the driver against its float64 numpy backend.

Exact label equality is asked only of inputs without near-ties: every case first asserts, on the float64 reference alone, that
|d1 - d0| / (d0 + d1) >= 1e-9 on all rows (fp64 distance sums are good to ~1e-13). The seeds below were picked on the CPU so
that this holds. Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import (KMEANS_WIDE_FITS, check_key_features, check_kmeans_dist, check_kmeans_lloyd, kmeans_matrix,
                           lloyd_reference, sq_dist64, tie_margin)
from vit_ocm_wmsegmentation_amd import _lib, cluster, synth
from vit_ocm_wmsegmentation_amd.engine import _p

pytestmark = pytest.mark.gpu

MIN_MARGIN = 1e-9


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the dispatch of kernels_cluster.hip, restated ----------------------------------------------------------------------------
def cpl_for(D):
    need = -(-(D // 4) // 32)
    return next(c for c in (1, 2, 3, 4, 6, 8) if c >= need)


def lloyd_split(rows):
    """(blocks, rows per wave): 4 waves per block."""
    nb = min((rows + 127) // 128, 1024)
    return nb, -(-rows // (nb * 4))


def kdist_split(rows):
    nb = min((rows + 255) // 256, 1024)
    return nb, -(-rows // (nb * 4))


def zs_split(rows):
    """(chunks, rows per chunk)."""
    R = min((rows + 255) // 256, 512)
    return R, -(-rows // R)


# ---- A. every CPL instantiation, full and partial -----------------------------------------------------------------------------
#   D    D/4  need  CPL
#   132   33   2     2   only lane 0 has a second chunk
#   192   48   2     2   ViT-T
#   256   64   2     2   full
#   400  100   4     4   partial
#   512  128   4     4   full
#   516  129   5     6   lane 0 alone has a fifth chunk; the sixth is zero on every lane
#   640  160   5     6   the sixth chunk is zero on every lane
#   768  192   6     6   ViT-B
#   772  193   7     8   the eighth chunk is zero on every lane
#   896  224   7     8   the eighth chunk is zero on every lane
CPL_WIDTHS = {132: 2, 192: 2, 256: 2, 400: 4, 512: 4, 516: 6, 640: 6, 768: 6, 772: 8, 896: 8}
# S = 9 and 13: one and two blocks, wave runs of 21 and 22 rows (Lloyd: ceil(81 / 4) and ceil(169 / 8)), so a run of odd
# length, where the wave's second lane group sits out the last trip, and a last wave with a shorter run
CPL_SIZES = (9, 13)
EDGE_BOOST = 6.0
# input seeds per (S, D), the first of 0, 1, ... where, on the float64 reference, the tie margin is >= 1e-5, each cluster gets at
# least a quarter of the rows and leaving out either the first or the last four columns moves at least four labels
CPL_SEEDS = {(9, 132): 2, (9, 192): 0, (9, 256): 0, (9, 400): 0, (9, 512): 4, (9, 516): 1, (9, 640): 1, (9, 768): 0, (9, 772): 1,
             (9, 896): 0, (13, 132): 0, (13, 192): 0, (13, 256): 0, (13, 400): 1, (13, 512): 0, (13, 516): 0, (13, 640): 1,
             (13, 768): 0, (13, 772): 0, (13, 896): 1}


def cpl_inputs(S, D):
    """x, 3 candidates, 2 centres. Every column has its own scale and offset; the first and the last four columns are
    scaled up so that they carry about as much of a distance as all the others: dropping either group moves labels."""
    x = kmeans_matrix(S, D, CPL_SEEDS[S, D])
    x[:, :4] *= EDGE_BOOST
    x[:, -4:] *= EDGE_BOOST
    return x, x[[3, 17, 40]].copy(), x[[5, 11]].copy()


def test_cpl_table():
    for D, cpl in CPL_WIDTHS.items():
        assert cpl_for(D) == cpl
    assert {cpl_for(D) for D in (4, 12, 32, 64, 100, 384, 1024)} == {1, 3, 8}  # the widths of the other k-means tests
    assert [lloyd_split(S * S) for S in CPL_SIZES] == [(1, 21), (2, 22)]


@pytest.mark.parametrize("D", list(CPL_WIDTHS))
@pytest.mark.parametrize("S", CPL_SIZES)
def test_cpl_dist_and_lloyd_against_float64(dev, S, D):
    x, cand, centers = cpl_inputs(S, D)
    ref = lloyd_reference(x, centers)
    assert tie_margin(ref["dd"]) >= MIN_MARGIN
    for cols in (slice(4, None), slice(None, -4)):  # without the first / the last four columns the labels are different ones
        dd = sq_dist64(x[:, cols], centers[:, cols])
        assert np.any((dd[1] < dd[0]) != (ref["labels"] == 1))
    b = cluster.DeviceBackend(torch.from_numpy(x).to(dev))
    check_kmeans_dist(b, cand, sq_dist64(x, cand), k1_closest=True)
    check_kmeans_lloyd(b, x, centers, ref)


# ---- B. capped row splits -------------------------------------------------------------------------------------------------------
#   S     rows     Lloyd blocks x per    kdist blocks x per    z-score chunks x chunk
#   363   131769   1024 x 33             515 x 64              512 x 258
#   384   147456   1024 x 36             576 x 64              512 x 288
#   513   263169   1024 x 65             1024 x 65             512 x 515
# Below the caps (1024 Lloyd blocks and 512 z-score chunks from S = 363, 1024 kdist blocks from S = 513) `per` is at most
# 32 (Lloyd) or 64 (kdist) and a chunk at most 256 rows. At S = 363 the 3993 Lloyd waves of 33 rows end in block 998: blocks
# 999..1023 are empty, and so is z-score chunk 511. At S = 384 every wave and chunk is full.
CAPPED = [(363, 8), (384, 8), (513, 4), (363, 192)]
_CAPPED = {}


def capped_inputs(S, D):
    x = kmeans_matrix(S, D, 2000 + S + D)
    n = S * S
    return x, x[[3, n // 2, n - 2]].copy(), x[[5, n - 7]].copy()


def _capped(S, D):
    """The inputs of a capped case with their float64 references, computed once and shared (read-only)."""
    if (S, D) not in _CAPPED:
        x, cand, centers = capped_inputs(S, D)
        x64 = x.astype(np.float64)
        ref = lloyd_reference(x64, centers)
        _CAPPED[S, D] = dict(x=x, x64=x64, cand=cand, centers=centers, ref=ref, want_d=sq_dist64(x64, cand))
        for a in (x, x64, cand, centers, _CAPPED[S, D]["want_d"], *ref.values()):
            a.setflags(write=False)
    return _CAPPED[S, D]


def fp64_sum_rtol(terms, base):
    """The tolerance for a device fp64 sum (over axis 0) of this many terms, from the reference alone: the relative spread
    of two float64 summation orders of the same terms (numpy's pairwise sum along a contiguous axis and a sequential
    cumsum). Two fixed-order fp64 sums may differ by about that much, so `base` (the tolerance the project uses at 4096
    rows) holds while the spread is below a quarter of it, and 4 x the spread otherwise."""
    a, b = np.ascontiguousarray(terms.T).sum(-1), np.cumsum(terms, axis=0)[-1]
    spread = float(np.max(np.abs(a - b) / np.abs(a)))
    print(f"fp64 summation spread over {terms.shape}: {spread:.3e} (base {base:g})")
    return base if spread < base / 4 else 4 * spread


def test_capped_splits_table():
    assert [lloyd_split(S * S) for S in (362, 363, 384, 513)] == [(1024, 32), (1024, 33), (1024, 36), (1024, 65)]
    assert [kdist_split(S * S) for S in (363, 384, 512, 513)] == [(515, 64), (576, 64), (1024, 64), (1024, 65)]
    assert [zs_split(S * S) for S in (362, 363, 384, 513)] == [(512, 256), (512, 258), (512, 288), (512, 515)]
    assert -(-363 * 363 // 33) == 3993 and -(-3993 // 4) == 999  # Lloyd blocks 999..1023 hold no row
    assert 511 * 258 >= 363 * 363 > 510 * 258  # z-score chunk 511 holds no row


@pytest.mark.parametrize("S,D", CAPPED)
def test_capped_zscore_against_float64(dev, S, D):
    x = _capped(S, D)["x"]
    X = torch.tensor(x, device=dev)
    stats = cluster.DeviceBackend(X).zscore()
    ref = cluster.NumpyBackend(x)
    want = ref.zscore()
    np.testing.assert_allclose(stats[:2], want[:2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(stats[2], want[2], rtol=0, atol=1e-7)  # an fp32 mean of values that sum to ~0
    np.testing.assert_allclose(stats[3], want[3], rtol=1e-5)
    np.testing.assert_allclose(X.cpu().numpy(), ref.X, rtol=0, atol=2e-6)


@pytest.mark.parametrize("S,D", CAPPED)
def test_capped_dist_against_float64(dev, S, D):
    c = _capped(S, D)
    b = cluster.DeviceBackend(torch.tensor(c["x"], device=dev))
    check_kmeans_dist(b, c["cand"], c["want_d"])  # 3 candidates, then 2 with closest


@pytest.mark.parametrize("S,D", CAPPED)
def test_capped_lloyd_against_float64(dev, S, D):
    c = _capped(S, D)
    assert tie_margin(c["ref"]["dd"]) >= MIN_MARGIN
    b = cluster.DeviceBackend(torch.tensor(c["x"], device=dev))
    check_kmeans_lloyd(b, c["x64"], c["centers"], c["ref"], sum_rtol=fp64_sum_rtol)


@pytest.mark.parametrize("name", list(KMEANS_WIDE_FITS))
def test_fit_matches_float64_driver(dev, name):
    """fit_two_means on the device against the same driver on float64 numpy (held against live sklearn on these inputs in
    tests/test_cluster_host.py): CPL 2 on 32 blocks, CPL 6 on 18."""
    seed, g, D, S = KMEANS_WIDE_FITS[name]
    feats = synth.upsample_token_grid(synth.synth_token_grid(seed, g, D, True), S).reshape(S * S, D).contiguous()
    rec_dev, rec_ref = [], []
    want = cluster.fit_two_means(cluster.NumpyBackend(feats.numpy()), n_init=3, record=rec_ref)
    got = cluster.fit_two_means(cluster.DeviceBackend(feats.clone().to(dev)), n_init=3, record=rec_dev)  # z-scores in place
    assert np.array_equal(got["labels"], want["labels"])
    assert [n for _, n in rec_dev] == [n for _, n in rec_ref] and got["n_iter"] == want["n_iter"]
    for (a, _), (r, _) in zip(rec_dev + [(got["inertia"], 0)], rec_ref + [(want["inertia"], 0)]):
        assert abs(a / r - 1) <= 1e-9, (a, r)


# ---- C. feature map ----------------------------------------------------------------------------------------------------------------
# (H, hd, g, S, B, images): ViT-B's width; ViT-S's heads at hd = 64; the smallest hd, where every float4 is another head; and
# 363^2 * 32 = 4 216 608 work items, more than the grid cap of 16384 x 256 threads: a second trip of the grid-stride loop,
# checked on image 1 of 2 so that the looped trip also carries the image offset
@pytest.mark.parametrize("H,hd,g,S,B,images", [(12, 64, 3, 10, 2, (0, 1)), (3, 64, 14, 56, 2, (0, 1)), (8, 4, 5, 12, 2, (0, 1)),
                                                 (2, 64, 24, 363, 2, (1,))])
def test_features_at_model_head_shapes(dev, lib, H, hd, g, S, B, images):
    gen = torch.Generator().manual_seed(7)
    qkv = torch.randn((3, B, H, g * g + 1, hd), generator=gen).to(dev)
    if S == 363:
        assert S * S * (H * hd // 4) > 16384 * 256
    for image in images:
        out = torch.full((S * S, H * hd), float("nan"), device=dev)  # an element left unwritten fails the bound
        check_key_features(qkv, image, S, out=out)


# ---- D. status outputs ---------------------------------------------------------------------------------------------------------------
def _changed(b, centers, labels_old, assign_only):
    labels, _, info = b.lloyd(centers, torch.from_numpy(labels_old).to(b.dev), assign_only=assign_only)
    return labels.cpu().numpy(), info[5]


@pytest.mark.parametrize("S,D", [(13, 64), (363, 8)])
def test_changed_flag_sees_one_row(dev, S, D):
    rows = S * S
    nb, per = lloyd_split(rows)
    last_wave = -(-rows // per) - 1
    if S == 13:
        assert (nb, per, last_wave) == (2, 22, 7)
        x = kmeans_matrix(S, D, 5)
        # lane groups 0 and 1 of the first wave, both groups of the last wave, the first row of wave 3 of block 0 and the
        # first row of the last block
        positions = [0, 1, 2, rows - 1, rows - 2, 3 * per, (last_wave // 4) * 4 * per]
        assert positions[5:] == [66, 88]
    else:
        assert (nb, per, last_wave, last_wave // 4) == (1024, 33, 3992, 998)
        x = _capped(S, D)["x"]
        positions = [rows - 1, last_wave * per + 1]  # the last row (lane group 0) and a row of lane group 1 of that wave
        assert (positions[0] - last_wave * per) % 2 == 0
    centers = x[[5, 11]]
    ref = lloyd_reference(x, centers)
    assert tie_margin(ref["dd"]) >= MIN_MARGIN
    L = ref["labels"]
    b = cluster.DeviceBackend(torch.tensor(x, device=dev))
    for assign_only in (False, True):
        labels, changed = _changed(b, centers, L, assign_only)
        assert np.array_equal(labels, L) and changed == 0.0
        for p in positions:
            old = L.copy()
            old[p] ^= 1
            labels, changed = _changed(b, centers, old, assign_only)
            assert np.array_equal(labels, L) and changed == 1.0, (p, assign_only)


def test_empty_cluster_in_full_mode(dev, lib):
    """Every row goes to cluster 0: the n == 0 branch of lloyd_cols_kernel and info[6], read from the device."""
    S, D = 13, 132
    x = (np.random.RandomState(3).standard_normal((S * S, D)) * 0.5).astype(np.float32)
    centers = np.stack([np.zeros(D, np.float32), np.full(D, 100.0, np.float32)])
    X, c_dev = torch.from_numpy(x).to(dev), torch.from_numpy(centers).to(dev)
    b = cluster.DeviceBackend(X)
    labels = torch.full((S * S,), -1, dtype=torch.int32, device=dev)
    new = torch.full((2, D), float("nan"), device=dev)
    sums = torch.full((2, D), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((7,), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(lib.ocm_op_kmeans_lloyd(_p(X), S, D, _p(c_dev), None, _p(labels), _p(new), _p(sums), _p(info), 0, _p(b.ws),
                                       b.ws.numel(), _s()))
    info, new, sums = info.cpu().numpy(), new.cpu().numpy(), sums.cpu().numpy()
    assert info[6] == 1.0 and info[2] == 0.0 and info[1] == S * S and int(labels.abs().sum()) == 0
    assert np.array_equal(new[1], np.zeros(D, np.float32)) and np.array_equal(sums[1], np.zeros(D))
    np.testing.assert_allclose(info[4], D * 100.0 ** 2, rtol=1e-12)  # ||0 - c1||^2
    x64 = x.astype(np.float64)
    np.testing.assert_allclose(sums[0], x64.sum(0), rtol=1e-11, atol=1e-9)
    np.testing.assert_allclose(new[0], x64.mean(0), rtol=2e-7, atol=1e-6)
    np.testing.assert_allclose(info[0], (x64 ** 2).sum(), rtol=1e-12)
    np.testing.assert_allclose(info[3], (new[0].astype(np.float64) ** 2).sum(), rtol=1e-12)
    with pytest.raises(cluster.EmptyClusterError):
        cluster.lloyd_single(b, centers, 1e-4)


@pytest.mark.parametrize("n_cand", [5, 64])
def test_dist_candidate_counts(dev, n_cand):
    """n_cand candidates go through ceil(n_cand / 2) launches, each writing its own rows of `dist`."""
    S, D = 9, 132
    x, _, _ = cpl_inputs(S, D)
    cand = kmeans_matrix(8, D, 77)[:n_cand]
    b = cluster.DeviceBackend(torch.from_numpy(x).to(dev))
    check_kmeans_dist(b, cand, sq_dist64(x, cand))


def test_dist_rejects_65_candidates(dev, lib):
    S, D = 9, 132
    X = torch.zeros((S * S, D), device=dev)
    cand = torch.zeros((65, D), device=dev)
    d = torch.zeros((65, S * S), dtype=torch.float64, device=dev)
    assert lib.ocm_op_kmeans_dist(_p(X), S, D, _p(cand), 65, None, _p(d), _s()) == _lib.OCM_EINVAL
    assert lib.ocm_op_kmeans_dist(_p(X), S, D, _p(cand), 0, None, _p(d), _s()) == _lib.OCM_EINVAL
    assert lib.ocm_op_kmeans_dist(_p(X), S, D, _p(cand), 64, None, _p(d), _s()) == _lib.OCM_OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("assign_only", [False, True])
def test_lloyd_tie_goes_to_cluster_zero_with_a_zero_chunk(dev, assign_only):
    """test_lloyd_tie_goes_to_cluster_zero's rows at D = 640 (CPL 6, need 5): the zero-filled sixth chunk of x and of both
    centres takes part in an exact tie."""
    x = np.zeros((16, 640), np.float32)
    b = cluster.DeviceBackend(torch.from_numpy(x).to(dev))
    labels, new, info = b.lloyd(np.ones((2, 640), np.float32), assign_only=assign_only)
    assert int(labels.sum()) == 0 and info[0] == 16 * 640 and info[1] == 16 and info[2] == 0 and info[6] == 1
    if not assign_only:
        assert np.array_equal(new, np.zeros((2, 640), np.float32)) and info[3] == 640 and info[4] == 640
