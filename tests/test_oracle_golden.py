"""The oracle (oracle/vit_oracle.py, the CPU restatement) against the golden vectors that
oracle/make_golden.py captured from the REAL reference module. Runs anywhere (CPU only)."""
import numpy as np
import pytest
import torch

from oracle import vit_oracle as O
from tests.golden_cases import SATURATED
from tests.helpers import CASES, case_dims, case_inputs, case_state_dict, load_golden

# fp32 CPU arithmetic re-run on possibly different host cores / thread counts: summation order of
# MKL / oneDNN kernels may differ, so allow a few ulps of the O(1) activations.
TOL = 2e-5


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_matches_reference_golden(name):
    case, gold = CASES[name], load_golden(name)
    assert float(gold["oracle_vs_reference_maxabs"]) <= 1e-6  # pinned when the fixture was made
    sd = case_state_dict(case)
    cfg = O.make_cfg(sd, case["patch"], case_dims(case)[2])
    for idx, x in enumerate(case_inputs(case)):
        pfx = f"in{idx}_"
        n = case["n"]
        feat, attns, qkvs = O.get_intermediate_feat(sd, cfg, x, n)
        a = attns[-1]
        # the saturated set is ill-conditioned: another summation order of the same fp32 arithmetic (other core count /
        # BLAS blocking) moves it by up to ~5e-4 (fp32 vs float64: tools/precision_study.py). That holds for the last block's
        # qkv too, not only for the maps: MKL's AVX2 kernels instead of the AVX-512 ones the fixture was written with move
        # it (|q|, |k|, |v| up to 18) by 4.6e-4 (the block's output by 8e-5, inside the common bound)
        atol = 2e-3 if name in SATURATED else TOL
        atol_qkv = 2e-3 if name in SATURATED else 10 * TOL
        np.testing.assert_allclose(a[:, :, 0, 1:].numpy(), gold[pfx + "cls_rows"], rtol=0, atol=atol)
        np.testing.assert_allclose(a[:, :, a.shape[-1] // 2, :].numpy(), gold[pfx + "mid_rows"], rtol=0, atol=atol)
        assert np.array_equal(a[:, :, 0, 1:].mean(1).argmax(-1).numpy(), gold[pfx + "argmax"])  # indices: exact
        np.testing.assert_allclose(feat[-1][:, :4, :16].numpy(), gold[pfx + "feat_head"], rtol=0, atol=10 * TOL)
        assert abs(float(feat[-1].double().abs().sum()) / float(gold[pfx + "feat_abssum"]) - 1) < 1e-5
        np.testing.assert_allclose(qkvs[-1][:, :, :, :3, :8].numpy(), gold[pfx + "qkv_head"], rtol=0, atol=atol_qkv)
        tokens = O.prepare_tokens(sd, cfg, x)
        np.testing.assert_allclose(tokens[:, :3, :16].numpy(), gold[pfx + "tokens_head"], rtol=0, atol=TOL)
        assert abs(float(tokens.double().abs().sum()) / float(gold[pfx + "tokens_abssum"]) - 1) < 1e-6
        if name in ("tiny_p8", "vits16_init"):  # the cheap cases also pin the other entry points
            assert torch.equal(O.get_last_selfattention(sd, cfg, x), a)
            np.testing.assert_allclose(O.forward_feats(sd, cfg, x)[:, 0, :32].numpy(), gold[pfx + "cls_out"],
                                       rtol=0, atol=10 * TOL)
        if case.get("full"):
            for j in range(n):
                np.testing.assert_allclose(feat[j].numpy(), gold[pfx + f"feat{j}"], rtol=0, atol=10 * TOL)
                np.testing.assert_allclose(attns[j].numpy(), gold[pfx + f"attn{j}"], rtol=0, atol=TOL)
                np.testing.assert_allclose(qkvs[j].numpy(), gold[pfx + f"qkv{j}"], rtol=0, atol=10 * TOL)


def test_compute_attention_contract():
    """utils.py:229-235: batch 0, one query row, CLS column dropped, (w,h) row-major, nearest x p."""
    B, H, wf, hf, p = 2, 3, 4, 5, 8
    N = wf * hf + 1
    attn = torch.arange(B * H * N * N, dtype=torch.float32).reshape(B, H, N, N)
    maps, nh = O.compute_attention([attn], 7, wf, hf, p)
    assert nh == H and maps.shape == (H, wf * p, hf * p)
    for head in range(H):
        for ty in range(wf):
            for tx in range(hf):
                blockv = maps[head, ty * p:(ty + 1) * p, tx * p:(tx + 1) * p]
                assert (blockv == attn[0, head, 7, 1 + ty * hf + tx].item()).all()
    assert O.region_query_index(37, 90, 16, 14) == 37 // 16 * 14 + 90 // 16


def test_sliding_window_origins_restatement():
    """sw_processing.py:151-163 on the sizes the reference / BASELINE use."""
    o = O.sliding_window_origins(1152, 1152, 128)
    assert len(o) == 49 and o[0] == (0, 0) and o[1] == (0, 128) and o[7] == (128, 0) and o[-1] == (768, 768)
    o = O.sliding_window_origins(4096, 4096, 128)
    assert len(o) == 900 and o[-1] == (3712, 3712) and o[-1][0] + 384 == 4096
    assert O.sliding_window_origins(256, 256, 128) == []  # size - 2*stride <= 0: no window
    assert O.sliding_window_origins(384, 384, 128) == [(0, 0)]


def test_helpers_match_reference_golden():
    """compute_attention / sliding_window / concat_crops: the oracle against outputs of the REFERENCE's own
    functions (tests/golden/helpers.npz, written by oracle/make_golden.py::run_helpers)."""
    gold = load_golden("helpers")
    attn = torch.from_numpy(gold["ca_attn"])
    for query in (0, 9):
        maps, nh = O.compute_attention([attn], query, 5, 7, 8)
        assert nh == 3 and np.array_equal(maps, gold[f"ca_maps_q{query}"])
    for size in (640, 1152):
        assert [tuple(o) for o in gold[f"sw_origins_{size}"].tolist()] == O.sliding_window_origins(size, size, 128)
    for n in (3, 2):
        rng = np.random.default_rng(int(gold[f"stitch_{n}_seed"]))
        crops = np.stack([rng.random((384, 384), dtype=np.float32) * 255 for _ in range(n * n)])
        assert np.array_equal(O.concat_crops(crops, 128, 384), gold[f"stitch_{n}"])


def test_oracle_threshold_chain_properties():
    """utils.py:61-115 restatement: PIL grey conversion is the identity on R=G=B planes, a flat attention map
    leaves min_max_normalize inactive, and Otsu separates a clean bimodal image between its two modes."""
    rng = np.random.default_rng(0)
    g = rng.uniform(0, 1, (1, 40, 40)).astype(np.float32)
    u1 = O.to_pil_gray_u8(g)
    assert np.array_equal(u1, O.to_pil_gray_u8(np.repeat(g, 3, 0)))
    assert np.array_equal(u1, (g[0] * np.float32(255)).astype(np.uint8))
    img = np.where(np.arange(1600).reshape(40, 40) % 3 == 0, 200, 40).astype(np.uint8)
    (th, th2, th3), (l1, l2, l3), result = O.threshold_masks(img, np.full((40, 40), 0.5, np.float32))
    assert 40 <= l2 < 200 and np.array_equal(th2, np.where(img > l2, 255, 0))
    assert np.array_equal(result, ((img / 2) * 0.6 + (127 / 2) * 0.4).astype(np.uint8))  # flat map: 0.5*255 -> 127
    assert set(np.unique(th3)) <= {0, 255}


def test_median_filter_restatement_equals_scipy_fixture():
    """oracle.median_filter against outputs of the real scipy.ndimage.median_filter (eval.py:144,158) — fixture written by
    oracle/make_golden_median.py; when scipy is importable where the tests run, against scipy itself too."""
    import numpy as np
    from oracle import vit_oracle as O
    from tests.golden_cases import MEDIAN_SIZES as SIZES, median_inputs as inputs
    from tests.helpers import load_golden
    gold = load_golden("median")
    x = inputs(int(gold["seed"]))
    for k in SIZES:
        assert np.array_equal(O.median_filter(x, k), gold[f"size{k}"]), k
    try:
        from scipy.ndimage import median_filter
    except ImportError:
        return
    for k in (2, 3, 6):
        assert np.array_equal(O.median_filter(x[:1], k)[0], median_filter(x[0], size=k))


def test_median_filter_restatement_equals_scipy_edge_fixture():
    """oracle.median_filter at the filter's edges against scipy's own outputs (tests/golden/median_edges.npz, written by
    oracle/make_golden_median.py): maps of height / width 1, windows that reflect through more than one period of the
    map, size 1 (the identity), eval.py's 13 and the cap 15. The same fixture holds ocm_op_median_filter
    (tests/test_post_shapes_gpu.py), and the oracle stands in for scipy there on a map too large to store."""
    from tests.golden_cases import MEDIAN_EDGE_SHAPES, MEDIAN_EDGE_SIZES, median_edge_inputs
    gold = load_golden("median_edges")
    maps = median_edge_inputs(int(gold["seed"]))
    assert tuple(m.shape for m in maps) == MEDIAN_EDGE_SHAPES
    assert any(k // 2 >= 2 * m.shape[1] for m in maps for k in MEDIAN_EDGE_SIZES)  # more than one period of reflection
    for i, x in enumerate(maps):
        assert len(np.unique(x)) < x.size or x.size == 1  # ties are planted
        assert not np.isnan(x).any() and not np.signbit(x).any()
        for k in MEDIAN_EDGE_SIZES:
            want = gold[f"map{i}_size{k}"]
            assert want.shape == x.shape and want.dtype == np.float32
            assert np.array_equal(O.median_filter(x, k), want), (x.shape, k)
        assert np.array_equal(gold[f"map{i}_size1"], x)
    try:
        from scipy.ndimage import median_filter
    except ImportError:
        return
    for i, x in enumerate(maps):
        for k in (13, 15):
            assert np.array_equal(gold[f"map{i}_size{k}"][0], median_filter(x[0], size=k))


def test_stitcher_restatements_accept_every_window_to_stride_ratio():
    """concat_crops / stitched_gray_image at stride < window <= 3 * stride, not only the reference's 3:1: the geometries
    tests/test_post_shapes_gpu.py holds the device stitchers to. A later edit of the oracle that narrows what it accepts
    fails here, not by silently shrinking the GPU tests."""
    from tests.golden_cases import STITCH_GEOMETRIES, STITCH_U8_GEOMETRIES
    rng = np.random.default_rng(8)
    for n, window, stride in STITCH_GEOMETRIES:
        assert stride < window <= 3 * stride
        crops = rng.random((n * n, window, window), dtype=np.float32) * 255
        out = O.concat_crops(crops, stride, window)
        S = window + (n - 1) * stride
        assert out.shape == (S, S) and out.dtype == np.float32
        # pixels only the first / the last window covers are copies of it
        assert np.array_equal(out[:stride, :stride], crops[0][:stride, :stride])
        assert np.array_equal(out[-stride:, -stride:], crops[-1][-stride:, -stride:])
        # windows cut from ONE smooth map stitch back to it (every blend is a convex combination of equal values)
        field = (np.add.outer(np.arange(S), 2 * np.arange(S)) % 64).astype(np.float32)
        cut = np.stack([field[y:y + window, x:x + window] for y in range(0, n * stride, stride) for x in range(0, n * stride, stride)])
        assert np.abs(O.concat_crops(cut, stride, window) - field).max() <= 64 * 2.0 ** -22
    assert {(3 * s == w, w <= 2 * s, w == s + 1, w % s != 0) for _, w, s in STITCH_GEOMETRIES} >= {
        (True, False, False, False), (False, True, False, False), (False, True, True, True), (False, False, False, True)}
    for H, W, stride, window in STITCH_U8_GEOMETRIES:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        n = len(range(0, H - 2 * stride, stride))
        assert n >= 1 and n == len(range(0, W - 2 * stride, stride))
        S = window + (n - 1) * stride
        out = O.stitched_gray_image(img, stride, window)
        assert out.shape == (S, S) and out.dtype == np.uint8
        k = min(stride, H, W)
        assert np.array_equal(out[:k, :k], O.pil_rgb_to_l(img[:k, :k]))  # the first window's own corner
        if S > H:
            assert not out[H:].any()  # PIL crop's zero fill below the slab
        assert np.array_equal(O.stitched_gray_image(img[:, :, 1], stride, window),
                              O.stitched_gray_image(np.repeat(img[:, :, 1:2], 3, 2), stride, window))
    assert sum(w + (len(range(0, H - 2 * s, s)) - 1) * s > min(H, W) for H, W, s, w in STITCH_U8_GEOMETRIES) >= 2


def test_bilinear_f64_restatement_equals_double_interpolate():
    """oracle.bilinear_upsample_f64 (numpy, taps and weights written out) against torch's double-precision bilinear with
    align_corners=False on every shape the GPU test uses. Both are float64 evaluations of one formula: they may differ by
    a few roundings of the coordinate (<= 4 ulp of the side on either side, times the map's range per pixel) and of the
    two blends (<= 4 ulp of max|src| on either side), so 16 * 2^-53 * (max|src| + (h + w) * (max - min)) bounds it."""
    import torch.nn.functional as F
    from tests.golden_cases import BILINEAR_SHAPES
    for T, h, w, scale in BILINEAR_SHAPES:
        rng = np.random.default_rng(100 * h + w)
        m = (rng.standard_normal((T, h, w)) * 40 + 100).astype(np.float32)
        got = O.bilinear_upsample_f64(m, scale)
        want = F.interpolate(torch.from_numpy(m).double()[:, None], scale_factor=scale, mode="bilinear", align_corners=False)[:, 0]
        assert got.shape == (T, h * scale, w * scale) and got.dtype == np.float64
        bound = 16 * 2.0 ** -53 * (np.abs(m).max() + (h + w) * float(m.max() - m.min()))
        assert np.abs(got - want.numpy()).max() <= bound, (T, h, w, scale)
        if scale == 1:
            assert np.array_equal(got, m.astype(np.float64))
        # and the float32 oracle the older tests use is this map rounded, to float32 round-off
        assert np.abs(O.bilinear_upsample(m, scale) - got).max() <= 2e-6 * np.abs(m).max() * (1 + h + w)


def test_uint8_stitcher_restatement_equals_reference_fixture():
    """oracle.stitched_gray_image / concat_crops on uint8 RGB windows against the reference's own sliding_window +
    concat_crops + PIL convert (helpers.npz: stitch_u8_*)."""
    import numpy as np
    from oracle import vit_oracle as O
    from tests.helpers import load_golden
    gold = load_golden("helpers")
    rng = np.random.default_rng(int(gold["stitch_u8_seed"]))
    img = rng.integers(0, 256, (160, 160), dtype=np.uint8)
    assert np.array_equal(O.stitched_gray_image(img, 32, 96), gold["stitch_u8_gray"])
    rnd = [rng.integers(0, 256, (96, 96, 3), dtype=np.uint8) for _ in range(9)]
    assert np.array_equal(O.pil_rgb_to_l(O.concat_crops(rnd, 32, 96)), gold["stitch_u8_random"])


def test_post_chain_restatements_are_self_consistent():
    """cv2 / skimage steps are restated (parity unpinned): properties that must hold whatever the library version."""
    import numpy as np
    from oracle import vit_oracle as O
    rng = np.random.default_rng(2)
    small = rng.random((3, 6, 5), dtype=np.float32)
    for p in (8, 16):
        up = np.repeat(np.repeat(small, p, 1), p, 2)
        assert np.array_equal(O.cv2_downscale(up, p), small)      # block-constant map: the centre average is the value
        assert np.array_equal(O.cv2_downscale(np.repeat(np.repeat(small, 16, 1), 16, 2), 8), np.repeat(np.repeat(small, 2, 1), 2, 2))
    img = np.concatenate([rng.integers(40, 90, 5000), rng.integers(150, 220, 5000)]).astype(np.uint8).reshape(100, 100)
    lvl = O.skimage_otsu_level(img)
    assert 89 <= lvl < 150 and abs(lvl - O.otsu_level(img)) <= 1  # both maximise the same between-class variance
    assert O.skimage_otsu_level(np.full((4, 4), 7, np.uint8)) == 7
    tiles = [np.full((2, 3), i, np.float32) for i in range(4)]
    assert np.array_equal(O.plain_concat_crops(tiles), np.array([[0, 0, 0, 1, 1, 1]] * 2 + [[2, 2, 2, 3, 3, 3]] * 2, np.float32))
