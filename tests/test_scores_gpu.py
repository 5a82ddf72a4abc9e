"""The mask scores on the device (kernels_score.hip through utils.mask_scores / calculate_metrics and eval.score_images /
validate) against the float64 restatement tests/scores_ref.py. Every operator case scores B = 3 different images, one of them
degenerate, at counts that put images 1 and 2 on unaligned addresses, end spans in every tail length and reach the cap on the
workgroups per image:
  * counts equal to the restatement's, the six scores that are quotients of them equal bit for bit;
  * dice_loss within DICE_BOUND of the float64 restatement. The bound: every fp32 sigmoid carries a few units of 2^-24 = 6e-8
    relative error, the float64 sums keep that, and the loss is one minus a ratio of two such sums and lies in [0, 1]. Measured
    maximum over this file: see MEASURED_DICE (a value above 3e-7 would mean a bug, not a bound to loosen);
  * two runs give the same bits, and an image scored alone gives the bits it has within the batch.
Needs an MI355X."""
import numpy as np
import pytest
import torch

from tests import scores_ref as R
from vit_ocm_wmsegmentation_amd import utils

pytestmark = pytest.mark.gpu

B = R.B
DICE_BOUND = R.DICE_BOUND
MEASURED_DICE = 1.264e-8  # the largest |dice_loss - restatement| over this file on an MI355X
CAP = (R.MAX_GROUPS - 1) * R.SPAN + 1  # the smallest count with the full MAX_GROUPS workgroups per image
COUNTS = [1, 3, 15, 16, 17, 255, 37 * 53, 4095, 4096, 4097, CAP, CAP + R.SPAN + 1]
KINDS = R.KINDS


def bits(t):
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def check(got_scores, got_counts, want_scores, want_counts, what):
    """-> the largest Dice difference. Counts exact, six scores bit-equal, dice_loss within DICE_BOUND (NaN where it is NaN)."""
    s, c = got_scores.cpu().numpy(), got_counts.cpu().numpy()
    assert s.dtype == np.float64 and c.dtype == np.int64 and s.shape == want_scores.shape and c.shape == want_counts.shape
    assert np.array_equal(c, want_counts), (what, c, want_counts)
    assert R.same_bits(s[:, :6], want_scores[:, :6]), (what, s[:, :6], want_scores[:, :6])
    nan = np.isnan(want_scores[:, 6])
    assert np.array_equal(np.isnan(s[:, 6]), nan), (what, s[:, 6], want_scores[:, 6])
    err = float(np.abs(s[~nan, 6] - want_scores[~nan, 6]).max()) if (~nan).any() else 0.0
    print(f"{what}: max |dice_loss - restatement| = {err:.3e}")
    assert err <= DICE_BOUND, (what, err)
    return err


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_scores_match_the_restatement(dev, kind, n):
    pred, target, want_scores, want_counts = R.case(kind, n)
    x, t = torch.tensor(pred, device=dev), torch.tensor(target, device=dev)
    scores, counts = utils.mask_scores(x, t)
    assert scores.is_cuda and counts.is_cuda and scores.shape == (B, 7) and counts.shape == (B, 4)
    check(scores, counts, want_scores, want_counts, f"{kind} n={n}")
    assert int(counts.sum()) == B * n
    if kind == "f32_nan":
        assert np.isnan(want_scores[1, 6]) and not np.isnan(want_scores[0, 6])
    # a second run gives the same bits
    again_s, again_c = utils.mask_scores(x, t)
    assert torch.equal(bits(again_s), bits(scores)) and torch.equal(again_c, counts)
    # image b alone (an aligned start) against image b within the batch (for odd n an unaligned one)
    for b in range(B):
        one_s, one_c = utils.mask_scores(x[b:b + 1].clone(), t[b:b + 1].clone())
        assert torch.equal(bits(one_s[0]), bits(scores[b])) and torch.equal(one_c[0], counts[b]), (kind, n, b)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_smooth_shapes_and_target_dtypes(dev, kind):
    n = 37 * 53
    pred, target, want_scores, want_counts = R.case(kind, n)
    x = torch.tensor(pred, device=dev).reshape(B, 1, 37, 53)
    t = torch.tensor(target, device=dev)
    for smooth in (0.0, 2.5):
        scores, counts = utils.mask_scores(x, t.reshape(B, 37, 53), smooth=smooth)
        check(scores, counts, R.score_batch(pred, target, smooth)[0], want_counts, f"{kind} smooth={smooth}")
    # the target in other dtypes: made float32 first. 0/1 targets, so that uint8 and bool hold them exactly
    t01 = (target > 0.5)
    want = R.score_batch(pred, t01.astype(np.float32))
    for dtype in (torch.float64, torch.float16, torch.uint8, torch.bool):
        scores, counts = utils.mask_scores(x, torch.from_numpy(t01).to(dev).to(dtype))
        check(scores, counts, want[0], want[1], f"{kind} target {dtype}")
    # a non-contiguous prediction is made contiguous
    wide = torch.zeros((B, 2 * n), dtype=x.dtype, device=dev)
    wide[:, ::2] = x.reshape(B, n)
    scores, counts = utils.mask_scores(wide[:, ::2], t)
    check(scores, counts, want_scores, want_counts, f"{kind} strided")
    with pytest.raises(ValueError):
        utils.mask_scores(x.to(torch.float64), t)
    with pytest.raises(ValueError):
        utils.mask_scores(x, t.to(torch.int32))


def test_calculate_metrics(dev):
    pred, target, _, _ = R.case("f32", 37 * 53)
    y_pred, y_true = torch.tensor(pred[0], device=dev).reshape(1, 1, 37, 53), torch.tensor(target[0], device=dev).reshape(1, 37, 53)
    y_score = torch.tensor(pred[1], device=dev).reshape(1, 1, 37, 53)
    five = utils.calculate_metrics(y_true, y_pred)
    six = utils.calculate_metrics(y_true, y_pred, y_score)
    assert len(five) == 5 and len(six) == 6 and all(type(v) is np.float64 for v in six)
    assert [v.item() for v in six[:5]] == [v.item() for v in five]  # .item() as eval.py calls it
    want = R.count_scores(*R.counts(pred[0], target[0]))
    want_auc = R.count_scores(*R.counts(pred[1], target[0]))[5]
    assert R.same_bits(np.array(five), want[:5]) and R.same_bits(np.array(six), np.append(want[:5], want_auc))
    # a uint8 / bool tensor holds classes here (not a mask of 0 / 255), as in the reference
    classes = y_pred > 0.5
    assert R.same_bits(np.array(utils.calculate_metrics(y_true > 0.5, classes.to(torch.uint8), classes)), np.append(want, []))
    try:
        import sklearn.metrics as M
    except ImportError:
        return
    yt, yp, ys = ((a > 0.5).astype(np.uint8).reshape(-1) for a in (target[0], pred[0], pred[1]))
    sk = [M.jaccard_score(yt, yp), M.f1_score(yt, yp), M.recall_score(yt, yp), M.precision_score(yt, yp), M.accuracy_score(yt, yp)]
    assert R.same_bits(np.array(five), np.array(sk, np.float64))
    auc = M.roc_auc_score(yt, ys)
    assert abs(six[5] - auc) <= 2 * np.spacing(auc)


# ---- eval.score_images / validate on the tiny ViT the other eval tests build ---------------------------------------------
METHODS = ["ours", "otsu", "heatmap_threshold", "k-means_feature_clustering", "chan-vese", "chan-vese_ours"]
S = 48


def _images(n, seed):
    from tests import chan_vese_ref as CV
    g = np.stack([CV.blobs(S, S, seed + b) for b in range(n)])
    return np.ascontiguousarray(np.repeat((g.astype(np.float32) / np.float32(255))[:, None], 3, axis=1)), g


@pytest.fixture(scope="module")
def model(dev):
    from tests.helpers import CASES, build_module
    return build_module(CASES["tiny_p8"], dev)


def _check_scored(scores, masks, maps, targets, what):
    assert masks.dtype == torch.uint8 and masks.is_cuda and maps.dtype == torch.float32 and scores.is_cuda
    assert set(np.unique(masks.cpu().numpy())) <= {0, 255}
    want_scores, want_counts = R.score_batch(masks.cpu().numpy(), targets.reshape(masks.shape))
    s = scores.cpu().numpy()
    assert R.same_bits(s[:, :6], want_scores[:, :6]), (what, s, want_scores)
    err = float(np.abs(s[:, 6] - want_scores[:, 6]).max())
    print(f"score_images {what}: max |dice_loss - restatement| = {err:.3e}")
    assert err <= DICE_BOUND
    return s


@pytest.mark.parametrize("method", METHODS)
def test_score_images(dev, model, method):
    from vit_ocm_wmsegmentation_amd import eval as E
    x, gray = _images(2, 20)
    targets = (gray > 128).astype(np.float32)[:, None]  # (B,1,S,S), as eval.py's dataset yields it
    scores, masks, maps = E.score_images(model, torch.from_numpy(x).to(dev), torch.from_numpy(targets).to(dev), method=method)
    assert scores.shape == (2, 7) and masks.shape == (2, S, S) and maps.shape == (2, S, S)
    _check_scored(scores, masks, maps, targets, method)
    segment = E.chan_vese_segment if method in E.CHAN_VESE else E.segment_images
    assert torch.equal(segment(model, torch.from_numpy(x).to(dev), method=method)[0], masks)
    with pytest.raises(ValueError):
        E.score_images(model, torch.from_numpy(x).to(dev), torch.from_numpy(targets[:, 0, :-1]).to(dev), method=method)


def test_score_images_crops(dev, model):
    from vit_ocm_wmsegmentation_amd import eval as E
    x, _ = _images(8, 30)
    x = torch.from_numpy(x).reshape(2, 4, 3, S, S).to(dev)
    targets = (E.tile_crops_image(x)[:, 0] > 0.5).to(torch.uint8)  # (B, 2S, 2S) uint8 classes
    scores, masks, maps = E.score_images(model, x, targets, method="ours", median_filter=3)
    assert masks.shape == (2, 2 * S, 2 * S)
    _check_scored(scores, masks, maps, targets.cpu().numpy().astype(np.float32), "crops")


def test_validate(dev, model):
    from vit_ocm_wmsegmentation_amd import eval as E
    xa, ga = _images(2, 20)
    xb, gb = _images(3, 40)
    ta, tb = (ga > 128).astype(np.float32), (gb > 128).astype(np.float32)[:, None]
    tb[1] = 0  # a target with one class only: no ROC-AUC for this image
    batches = [(torch.from_numpy(xa).to(dev), torch.from_numpy(ta).to(dev)), (torch.from_numpy(xb).to(dev), torch.from_numpy(tb).to(dev))]
    per_image = np.concatenate([E.score_images(model, x, t)[0].cpu().numpy() for x, t in batches])
    assert np.isnan(per_image[:, 5]).tolist() == [False, False, False, True, False]
    acc, f1, loss, means = E.validate(model, iter(batches))
    assert means["images"] == 5 and means["auc_nan_images"] == 1
    assert (acc, f1, loss) == (means["accuracy"], means["f1"], means["dice_loss"])
    for k, name in enumerate(R.SCORE_NAMES):  # float64 sums of five values in [0, 1] in another order: a few 2^-53
        want = np.nanmean(per_image[:, k])
        assert abs(means[name] - want) <= 8 * 2.0 ** -53, (name, means[name], want)
    # every image without a ROC-AUC: its mean is NaN and nothing else changes
    one = (batches[1][0][1:2], batches[1][1][1:2])
    acc1, _, _, only = E.validate(model, [one])
    assert np.isnan(only["auc"]) and only["auc_nan_images"] == only["images"] == 1
    assert acc1 == float(E.score_images(model, *one)[0][0, 4])
