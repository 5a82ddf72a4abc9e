"""The device operators of the region-query chain (kernels_morph.hip) bit for bit against tests/morph_ref.py (itself pinned
against live scipy.ndimage by tests/test_morph_host.py): labelling, remove_small_objects, dilation / erosion / closing,
region sums, the get_ROIs / morphology_cleaning chains, the Yen mask and the query mean. Every case runs as a batch of
three DIFFERENT images, so that labels or parents of one image leaking into another show. One 1024 x 1024 case is checked
by construction. Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import morph_ref as R
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import analyse_attention, utils

pytestmark = pytest.mark.gpu

T = 32  # ocm_label8_tile(), asserted in test_tile_side


def _groups(names):
    """The family names in batches of three different images (the last batch wraps around)."""
    names = list(names)
    padded = names + names[:(-len(names)) % 3]
    return [padded[i:i + 3] for i in range(0, len(padded), 3)]


def _eq(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert_same_bits(got.cpu(), want, what, ("image", "row", "col"))


def test_tile_side(lib):
    assert lib.ocm_label8_tile() == T


@pytest.mark.parametrize("h,w", R.sizes(T))
def test_operators_match_reference(dev, h, w):
    fam, ref = R.families(h, w, T), R.reference(h, w, T)
    for group in _groups(fam):
        what = f"{h}x{w} {group}"
        m = torch.from_numpy(np.stack([fam[n] for n in group])).to(dev)
        want = {k: np.stack([ref[n][k] for n in group]) for k in ("labels", "removed", "dilated", "eroded0", "eroded1",
                                                                   "closed", "rois")}
        labels, counts = utils.label_regions(m)
        assert labels.dtype == torch.int32 and counts.dtype == torch.int32
        _eq(labels, want["labels"], f"labels {what}")
        assert counts.cpu().tolist() == [ref[n]["n"] for n in group], what
        again, counts2 = utils.label_regions(m)
        assert_same_bits(labels, again, f"labels, second run {what}")
        assert_same_bits(counts, counts2, f"counts, second run {what}")
        as_u8, _ = utils.label_regions(m.to(torch.uint8) * 255)  # any nonzero byte is foreground
        assert_same_bits(labels, as_u8, f"labels of the 0/255 mask {what}")
        _eq(utils.remove_small_objects(m, 20), want["removed"], f"remove_small_objects {what}")
        _eq(utils.binary_morph(m, R.DISK2, 0, 0), want["dilated"], f"dilation {what}")
        _eq(utils.binary_morph(m, R.DISK2, 1, 0), want["eroded0"], f"erosion, border 0 {what}")
        _eq(utils.binary_morph(m, R.DISK2, 1, 1), want["eroded1"], f"erosion, border 1 {what}")
        _eq(utils.binary_closing(m), want["closed"], f"closing {what}")
        _eq(utils.get_ROIs(m), want["rois"], f"get_ROIs {what}")
        nmax = max(max(ref[n]["n"] for n in group), 1)
        st = utils.region_stats(labels, nmax)
        for b, n in enumerate(group):
            k = max(ref[n]["n"], 1)
            area, sr, sc, bbox = ref[n]["stats"]
            for key, w_ in (("area", area), ("sum_row", sr), ("sum_col", sc), ("bbox", bbox)):
                got = st[key][b].cpu().numpy()
                assert np.array_equal(got[:k], w_), (key, what, n)
                if key != "bbox":
                    assert not got[k:].any(), (key, what, n)  # labels the image does not hold: zero sums
            assert utils.morphology_cleaning(m[b]) == ref[n]["points"], (what, n)
        single = utils.label_regions(m[1])
        assert_same_bits(single[0], labels[1], f"(H,W) mask {what}")
        assert single[1].dim() == 0 and int(single[1]) == ref[group[1]]["n"]


def test_asymmetric_footprint(dev):
    fp = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 0]], np.uint8)
    big = np.zeros((7, 7), np.uint8)
    big[0, 6] = big[3, 3] = big[6, 1] = 1
    ms = np.stack([R.gaussian_noise(29, 41, s) for s in (1, 2, 3)])
    m = torch.from_numpy(ms).to(dev)
    for f in (fp, big, np.ones((1, 1), np.uint8)):
        for border in (0, 1):
            _eq(utils.binary_morph(m, f, 0, border), np.stack([R.dilate(x, f, border) for x in ms]), f"dilate {f.shape} {border}")
            _eq(utils.binary_morph(m, f, 1, border), np.stack([R.erode(x, f, border) for x in ms]), f"erode {f.shape} {border}")


def test_get_rois_of_a_uint8_mask_reads_it_as_a_label_image(dev):
    """data.py:222-224 passes a uint8 {0, 255} array: skimage's remove_small_objects then counts the white CLASS, not its
    components — two 12-pixel blobs (24 white pixels) stay, although each is smaller than 20."""
    m = np.zeros((40, 40), bool)
    m[3:6, 3:7] = m[20:23, 30:34] = True
    white = torch.from_numpy(m.astype(np.uint8) * 255).to(dev)
    _eq(utils.get_ROIs(white), R.label8(R.closing(m))[0], "uint8 mask with 24 white pixels")
    assert int(utils.get_ROIs(torch.from_numpy(m).to(dev)).max()) == 0  # the bool mask loses both blobs
    m[20:23, 30:34] = False
    m[30, 30:37] = True  # 12 + 7 = 19 white pixels
    assert int(utils.get_ROIs(torch.from_numpy(m.astype(np.uint8) * 255).to(dev)).max()) == 0
    with pytest.raises(ValueError):
        utils.get_ROIs(torch.full((8, 8), 7, dtype=torch.uint8, device=dev))


def test_yen_threshold(dev):
    rs = np.random.RandomState(5)
    img = rs.normal(50, 10, (61, 83))
    img[10:30, 20:50] += 120
    u8 = img.clip(0, 255).astype(np.uint8)
    level = R.yen_from_hist(np.bincount(u8.ravel(), minlength=256))
    assert 60 < level < 170
    mask, got_level = utils.yen_threshold(torch.from_numpy(u8).to(dev), return_level=True)
    assert got_level == level and mask.dtype == torch.bool
    _eq(mask, level <= u8, "Yen mask of a uint8 image")
    rgb = np.stack([u8 / 255.0, (u8 // 2) / 255.0, (255 - u8) / 255.0]).astype(np.float32)
    g = R.gray_u8(rgb)
    _eq(utils.yen_threshold(torch.from_numpy(rgb).to(dev)), R.yen_from_hist(np.bincount(g.ravel(), minlength=256)) <= g,
        "Yen mask of a float RGB image")
    flat = torch.full((9, 9), 41, dtype=torch.uint8, device=dev)
    mask, lv = utils.yen_threshold(flat, return_level=True)
    assert lv == 41 and bool(mask.all())


def test_large_image_by_construction(dev):
    """1024 x 1024: a serpentine over the upper half (one component through every tile it covers) and a grid of 3 x 3
    blobs below it; the second image of the batch is the first upside down, so that the blobs come first."""
    S = 1024
    top = R.serpentine(512, S)
    img = np.zeros((S, S), bool)
    img[:512] = top
    ys, xs = np.arange(516, S - 3, 8), np.arange(2, S - 3, 8)
    for y in ys:
        for x in xs:
            img[y:y + 3, x:x + 3] = True
    nblobs = len(ys) * len(xs)
    batch = np.stack([img, img[::-1].copy()])
    m = torch.from_numpy(batch).to(dev)
    labels, counts = utils.label_regions(m)
    assert counts.cpu().tolist() == [nblobs + 1, nblobs + 1]
    again, _ = utils.label_regions(m)
    assert_same_bits(labels, again, "labels, second run")
    area = utils.region_stats(labels, nblobs + 1)["area"].cpu().numpy()
    assert area[0, 0] == top.sum() and (area[0, 1:] == 9).all()          # the serpentine starts at pixel 0
    assert area[1, -1] == top.sum() and (area[1, :-1] == 9).all()        # upside down its first pixel comes last
    assert bool(((labels > 0) == m).all())
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):                      # every 8-neighbour pair of foreground pixels
        a = labels[:, :S - dy, max(-dx, 0):S - max(dx, 0)]
        b = labels[:, dy:, max(dx, 0):S + min(dx, 0)]
        both = (a > 0) & (b > 0)
        assert bool((a[both] == b[both]).all()), (dy, dx)
    for b in range(2):
        lab = labels[b].cpu().numpy().ravel()
        fg = np.nonzero(lab)[0]
        ids, first = np.unique(lab[fg], return_index=True)
        assert np.array_equal(ids, np.arange(1, nblobs + 2))
        assert (np.diff(fg[first]) > 0).all()                            # first pixels in increasing label order
    kept = utils.remove_small_objects(m, 10)
    _eq(kept[0, :512], top, "remove_small_objects keeps the serpentine")
    assert not bool(kept[0, 512:].any()) and not bool(kept[1, :512 - 4].any())


@pytest.mark.parametrize("H", [3, 6])
@pytest.mark.parametrize("P", [1, 49, 2304])
def test_query_mean(dev, H, P):
    """ocm_op_query_mean against numpy bit for bit: np.mean over the heads of each selected row, then
    np.mean(list_of_maps, axis=0). numpy adds the maps one after the other, except that for a single pixel (P = 1) it
    switches to pairwise summation from eight maps on; the operator always adds sequentially, so at P = 1 numpy itself is
    the reference for the selections of fewer than eight maps and its sequential restatement (morph_ref.query_mean) for
    the longer one."""
    rs = np.random.RandomState(100 * H + P)
    rows = (rs.standard_normal((4, H, 5, P)) * rs.uniform(0.1, 3, (4, H, 5, 1))).astype(np.float32)
    sel = [[3, 0, 3, 4, 1, 1, 2, 0, 4, 3, 2], [], [2], [4, 4, 0, 1, 4, 2, 3]]
    got = analyse_attention.query_mean(torch.from_numpy(rows).to(dev), sel).cpu().numpy()
    want = R.query_mean(rows, sel)
    assert np.isnan(got[1]).all() and np.isnan(want[1]).all()
    for t in (0, 2, 3):
        assert np.array_equal(got[t], want[t]), t
        if P > 1 or len(sel[t]) < 8:
            maps = [np.mean(rows[t, :, q], axis=0) for q in sel[t]]
            assert np.array_equal(got[t], np.mean(maps, axis=0)), t
    again = analyse_attention.query_mean(torch.from_numpy(rows).to(dev), sel)
    assert_same_bits(torch.from_numpy(got)[[0, 2, 3]], again.cpu()[[0, 2, 3]], "query_mean, second run")
    with pytest.raises(ValueError):
        analyse_attention.query_mean(torch.from_numpy(rows).to(dev), [[5], [], [], []])
