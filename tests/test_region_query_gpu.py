"""analyse_attention.region_query_points / region_queried_attention (the reference's analyse_attention.py --region_query,
:183-223) on a small synthetic encoder: the query points against the numpy chain of tests/morph_ref.py, the region-queried
map against the numpy query mean of the rows get_last_attention_rows returns for the same tokens, the masks against
threshold() on that map. Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import morph_ref as R
from tests.helpers import build_module
from tests.memcheck import assert_same_bits
from vit_ocm_wmsegmentation_amd import analyse_attention as A
from vit_ocm_wmsegmentation_amd import eval as E
from vit_ocm_wmsegmentation_amd import utils

pytestmark = pytest.mark.gpu

PATCH = 8
CASE = dict(dim=128, depth=2, heads=2, patch=PATCH, img_size=64, variant="sharp", seed=3)


@pytest.fixture(scope="module")
def model(dev):
    return build_module(CASE, dev)


def _images(S):
    """(3,3,S,S) float32: dark noise with a few bright blobs (two large ones, one of 3 x 3 pixels that the 20-pixel
    clean-up removes, one L-shaped); the last image is blank (the same dark noise) but for a grid of 2 x 2 bright specks, all cleaned away: no region."""
    rs = np.random.RandomState(S)
    img = (rs.uniform(0.02, 0.12, (3, 1, S, S))).astype(np.float32)
    for b, blobs in enumerate([[(5, 7, 9, 11), (30, 40, 8, 6), (50, 12, 3, 3)], [(20, 3, 12, 5), (S - 13, S - 17, 10, 14)]]):
        for y, x, hh, ww in blobs:
            img[b, 0, y:y + hh, x:x + ww] = rs.uniform(0.7, 0.95, (hh, ww))
    img[1, 0, 40:52, 30:33] = img[1, 0, 49:52, 30:44] = 0.8
    for y in range(4, S - 2, 12):
        for x in range(6, S - 2, 12):
            img[2, 0, y:y + 2, x:x + 2] = rs.uniform(0.7, 0.95, (2, 2))
    return np.ascontiguousarray(np.repeat(img, 3, axis=1))


@pytest.mark.parametrize("S", [64, 96])
def test_region_query_chain(dev, model, S):
    imgs = _images(S)
    x = torch.from_numpy(imgs).to(dev)
    want = [R.query_points(im, PATCH) for im in imgs]
    points, tokens = A.region_query_points(x, PATCH)
    assert points == [w[0] for w in want] and tokens == [w[1] for w in want]
    assert [len(t) for t in tokens][2] == 0 and len(tokens[0]) == 2 and len(tokens[1]) >= 2  # the 3 x 3 blob is cleaned away

    masks, maps, n_points = A.region_queried_attention(model, x)
    assert n_points == [len(t) for t in tokens] and n_points[2] == 0
    assert masks.shape == (3, 3, S, S) and masks.dtype == torch.uint8 and maps.shape == (3, S, S) and maps.dtype == torch.float32
    union = sorted({q for t in tokens for q in t})
    rows = model.get_last_attention_rows(x, query_rows=torch.tensor(union, dtype=torch.int32, device=dev))
    sel = [[union.index(q) for q in t] for t in tokens]
    small = R.query_mean(rows.cpu().numpy(), sel)  # numpy up to the resize stage
    g = S // PATCH
    got_small = A.query_mean(rows, sel).cpu().numpy()
    assert np.array_equal(got_small, small, equal_nan=True) and np.isnan(small[2]).all()
    big = E._upsample(torch.from_numpy(small).to(dev).reshape(3, g, g), PATCH)
    for b in (0, 1):
        assert_same_bits(maps[b], big[b], f"region-queried map of image {b}")
        assert bool(torch.isfinite(maps[b]).all())
        th = utils.threshold(x[b], maps[b], as_numpy=False)
        assert_same_bits(masks[b], torch.stack(th), f"masks of image {b}")
        assert 0 < int((masks[b, 0] > 0).sum()) < S * S
    assert bool(torch.isnan(maps[2]).all()) and not bool(masks[2].any())

    masks3, maps3, n3 = A.region_queried_attention(model, x, median_filter=3)
    assert n3 == n_points and bool(torch.isfinite(maps3[:2]).all()) and bool(torch.isnan(maps3[2]).all())
    assert not bool(masks3[2].any())


def test_no_points_in_the_whole_batch(dev, model):
    x = torch.from_numpy(_images(64)[2:]).to(dev)
    masks, maps, n_points = A.region_queried_attention(model, x)
    assert n_points == [0] and bool(torch.isnan(maps).all()) and not bool(masks.any())
