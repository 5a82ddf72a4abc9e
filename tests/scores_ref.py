"""float64 numpy restatement of ocm_op_mask_scores (kernels_score.hip): the counts tp, fp, fn, tn of the classes value > 0.5 and
target > 0.5, the six scores that are functions of them (sklearn's jaccard_score, f1_score, recall_score, precision_score,
accuracy_score and the roc_auc_score of a 0/1 score, with sklearn 1.7's conventions: a zero denominator gives 0.0, the AUC of a
one-class target is NaN), and the reference's DiceLoss (utils.py:410-424) with the sigmoid and the sums in float64. The arbiter
of the GPU tests; tests/test_scores_host.py holds it against live sklearn."""
import functools

import numpy as np

SCORE_NAMES = ("jaccard", "f1", "recall", "precision", "accuracy", "auc", "dice_loss")
SPAN, MAX_GROUPS = 4096, 256  # the kernels' span per workgroup and workgroups per image (asserted in test_scores_host.py)
PART_BYTES = 48               # one workgroup's partial in the workspace
DICE_BOUND = 1e-6             # |dice_loss - restatement| on the device: fp32 sigmoids (a few 2^-24 relative each) in float64 sums


def values(pred):
    """What the operator scores: a uint8 mask stands for v / 255 in float32 (eval.py's output / 255), float32 is used as is."""
    pred = np.asarray(pred)
    if pred.dtype == np.uint8:
        return pred.astype(np.float32) / np.float32(255)
    assert pred.dtype == np.float32, pred.dtype
    return pred


def counts(pred, target):
    """(tp, fp, fn, tn) as Python ints. NaN compares false: class 0."""
    with np.errstate(invalid="ignore"):
        pc = values(pred).reshape(-1) > np.float32(0.5)
        tc = np.asarray(target, np.float32).reshape(-1) > np.float32(0.5)
    return int((pc & tc).sum()), int((pc & ~tc).sum()), int((~pc & tc).sum()), int((~pc & ~tc).sum())


def ratio(num, den):
    return np.float64(num) / np.float64(den) if den else np.float64(0.0)


def count_scores(tp, fp, fn, tn):
    """[jaccard, f1, recall, precision, accuracy, auc]: one IEEE float64 division of integers each."""
    if (tp + fn) and (tn + fp):
        auc = np.float64(0.5) * (np.float64(tp) / np.float64(tp + fn) + np.float64(tn) / np.float64(tn + fp))
    else:
        auc = np.float64("nan")
    return np.array([ratio(tp, tp + fp + fn), ratio(2 * tp, 2 * tp + fp + fn), ratio(tp, tp + fn), ratio(tp, tp + fp),
                     np.float64(tp + tn) / np.float64(tp + fp + fn + tn), auc], np.float64)


def sigmoid(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def dice_loss(pred, target, smooth=1.0):
    p = sigmoid(values(pred).reshape(-1))
    t = np.asarray(target, np.float32).reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.float64(1.0) - (2.0 * np.sum(p * t) + smooth) / (np.sum(p) + np.sum(t) + smooth)


def score(pred, target, smooth=1.0):
    """One image -> (scores (7,) float64 in SCORE_NAMES order, counts (4,) int64)."""
    c = counts(pred, target)
    return np.append(count_scores(*c), dice_loss(pred, target, smooth)), np.array(c, np.int64)


def score_batch(pred, target, smooth=1.0):
    """(B, ...) -> (scores (B,7), counts (B,4)), every image on its own."""
    res = [score(p, t, smooth) for p, t in zip(pred, target)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def same_bits(a, b):
    """float64 arrays equal bit for bit, every NaN standing for every other."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def random_pair(n, share, seed):
    """A 0/1 float32 prediction and target of n elements with about `share` foreground, agreeing on about 80 % of it."""
    rng = np.random.default_rng(seed)
    t = rng.random(n) < share
    flip = rng.random(n) < 0.2
    return (t ^ flip).astype(np.float32), t.astype(np.float32)


# ---- the inputs the GPU tests share -------------------------------------------------------------------------------------
B = 3
KINDS = ["u8", "f32", "f32_nan"]  # a uint8 mask, float32 values, float32 values with NaN in image 1
HALF_UP = np.nextafter(np.float32(0.5), np.float32(1))
U8_SPECIAL = np.array([0, 127, 128, 255, 1, 254, 126, 129], np.uint8)  # 127 is class 0, 128 is class 1
F32_SPECIAL = np.array([0.5, HALF_UP, np.inf, -np.inf, -3.0, 0.0, 1.0, 40.0, -40.0, 100.0, -100.0, 88.8, -88.8, 0.49999997,
                        1e-30, -0.0], np.float32)  # the threshold, infinities, negatives, logits that saturate the sigmoid
T_SPECIAL = np.array([0.5, HALF_UP, 0.25, 0.75, 0.0, 1.0], np.float32)


@functools.lru_cache(maxsize=None)
def case(kind, n):
    """The inputs of the GPU tests: B different images of n elements, image 2 degenerate, the special values scattered over
    images 0 and 1. -> (pred (B,n), target (B,n), restatement scores (B,7), restatement counts (B,4)), computed once and read-only."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n % 997)
    target = (rng.random((B, n)) < np.array([[0.3], [0.7], [0.5]])).astype(np.float32)
    spots = rng.permutation(n)[:min(n, 3 * len(T_SPECIAL))]
    target[0, spots] = T_SPECIAL[np.arange(len(spots)) % len(T_SPECIAL)]
    if kind == "u8":
        pred = np.where(rng.random((B, n)) < 0.8, (target > 0.5) * np.uint8(255), rng.integers(0, 256, (B, n))).astype(np.uint8)
        special = U8_SPECIAL
    else:
        pred = np.where(rng.random((B, n)) < 0.6, (target > 0.5).astype(np.float32), 3 * rng.standard_normal((B, n)))
        pred = pred.astype(np.float32)
        special = F32_SPECIAL
    for b in (0, 1):  # the special values at scattered places of two images
        spots = rng.permutation(n)[:min(n, 2 * len(special))]
        pred[b, spots] = special[(np.arange(len(spots)) + b) % len(special)]
    if kind == "f32_nan":  # NaN is class 0 on either side, and makes this image's Dice loss NaN
        pred[1, rng.permutation(n)[:min(n, 3)]] = np.nan
        target[1, rng.permutation(n)[:1]] = np.nan
    deg = {"u8": (0, 0), "f32": (1, 1), "f32_nan": (0, 1)}[kind]  # image 2 is degenerate: constant prediction and target
    pred[2], target[2] = deg[0] * (255 if kind == "u8" else 1), deg[1]
    scores, counts = score_batch(pred, target)
    for a in (pred, target, scores, counts):
        a.setflags(write=False)
    return pred, target, scores, counts
