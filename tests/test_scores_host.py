"""Host side of the mask scores (kernels_score.hip, utils.mask_scores / calculate_metrics, eval.score_images / validate): the
numpy restatement tests/scores_ref.py against live sklearn, the C ABI's declarations, workspace sizes and argument refusals, and
the refusals of the Python surface. No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

from tests import scores_ref as R
from vit_ocm_wmsegmentation_amd import _lib, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ocm_mask_scores_workspace_bytes", "ocm_op_mask_scores"]
MAX_COUNT = 1 << 36

DEGENERATE = {"zeros_zeros": (0, 0), "zeros_ones": (0, 1), "ones_zeros": (1, 0), "ones_ones": (1, 1)}  # (pred, target)


def _sklearn_scores(pred, target):
    """The reference's calculate_metrics (utils.py:388-408) plus PGT.py's roc_auc_score of the 0/1 prediction."""
    M = pytest.importorskip("sklearn.metrics")
    y_true = (target > 0.5).astype(np.uint8).reshape(-1)
    y_pred = (pred > 0.5).astype(np.uint8).reshape(-1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        five = [M.jaccard_score(y_true, y_pred), M.f1_score(y_true, y_pred), M.recall_score(y_true, y_pred),
                M.precision_score(y_true, y_pred), M.accuracy_score(y_true, y_pred)]
        auc = M.roc_auc_score(y_true, y_pred)
    return np.array(five, np.float64), np.float64(auc)


def _check_against_sklearn(pred, target):
    five, auc = _sklearn_scores(pred, target)
    got = R.count_scores(*R.counts(pred, target))
    assert R.same_bits(got[:5], five), (got[:5], five)
    if np.isnan(auc):
        assert np.isnan(got[5])
    else:
        assert abs(got[5] - auc) <= 2 * np.spacing(auc), (got[5], auc)


@pytest.mark.parametrize("share", [0.02, 0.3, 0.5, 0.9])
@pytest.mark.parametrize("n", [1, 17, 37 * 53, 96 * 96])
def test_restatement_matches_sklearn_on_random_pairs(n, share):
    _check_against_sklearn(*R.random_pair(n, share, seed=n + int(100 * share)))


@pytest.mark.parametrize("kind", sorted(DEGENERATE))
def test_restatement_matches_sklearn_on_degenerate_pairs(kind):
    p, t = DEGENERATE[kind]
    pred, target = np.full(1000, p, np.float32), np.full(1000, t, np.float32)
    _check_against_sklearn(pred, target)
    got = R.count_scores(*R.counts(pred, target))
    assert np.isnan(got[5])  # one class only in the target
    if kind == "zeros_zeros":
        assert list(got[:5]) == [0, 0, 0, 0, 1]


def test_restatement_pieces():
    # the uint8 mask stands for v / 255: 127 is class 0, 128 is class 1; NaN is class 0 on either side
    pred = np.array([0, 127, 128, 255], np.uint8)
    assert R.counts(pred, np.ones(4, np.float32)) == (2, 0, 2, 0)
    half_up = np.nextafter(np.float32(0.5), np.float32(1))
    vals = np.array([0.5, half_up, np.nan, np.inf, -np.inf, -3.0], np.float32)
    assert R.counts(vals, vals) == (2, 0, 0, 4)
    assert R.counts(np.ones(2, np.float32), np.array([np.nan, 1], np.float32)) == (1, 1, 0, 0)
    # the Dice loss puts the 0/1 mask through the sigmoid, as the reference's DiceLoss does
    want = 1 - (2 * (0.5 * 0 + 1 / (1 + np.exp(-1.0)) * 1) + 1) / (0.5 + 1 / (1 + np.exp(-1.0)) + 1 + 1)
    assert abs(R.dice_loss(np.array([0, 255], np.uint8), np.array([0, 1], np.float32)) - want) < 1e-15
    x = np.array([-200.0, -1.0, 0.0, 1.0, 200.0, np.inf, -np.inf])
    assert np.allclose(R.sigmoid(x), [0, 1 / (1 + np.e), 0.5, np.e / (1 + np.e), 1, 1, 0], rtol=1e-15, atol=1e-80)
    torch_loss = 1 - (2 * (torch.sigmoid(torch.tensor(x[:5])) * torch.tensor([0, 1, 1, 0, 1.0])).sum() + 1) / (
        torch.sigmoid(torch.tensor(x[:5])).sum() + 3 + 1)
    assert abs(R.dice_loss(x[:5].astype(np.float32), np.array([0, 1, 1, 0, 1], np.float32)) - float(torch_loss)) < 1e-15


def test_entry_points_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "ocm_vit.h")).read()
    assert re.search(r"#define OCM_ABI_VERSION 20\b", text)
    assert "NaN compares false" in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ocm_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert lib.ocm_abi_version() == _lib.OCM_ABI_VERSION == 20
    assert "kernels_score.hip" in open(os.path.join(ROOT, "vit-ocm-wmsegmentation_amd", "csrc", "Makefile")).read()


def test_workspace_sizes(lib):
    ws = lib.ocm_mask_scores_workspace_bytes
    assert ws(1, 1) == ws(1, R.SPAN) == R.PART_BYTES and ws(1, R.SPAN + 1) == 2 * R.PART_BYTES
    assert ws(3, 37 * 53) == 3 * R.PART_BYTES and ws(64, 384 * 384) == 64 * 36 * R.PART_BYTES
    cap = (R.MAX_GROUPS - 1) * R.SPAN + 1  # the smallest count with MAX_GROUPS workgroups per image
    assert ws(1, cap - 1) == (R.MAX_GROUPS - 1) * R.PART_BYTES and ws(1, cap) == R.MAX_GROUPS * R.PART_BYTES
    probes = [1, 2, 15, 16, 17, R.SPAN - 1, R.SPAN, R.SPAN + 1, 3 * R.SPAN + 5, 384 * 384, cap - 1, cap, cap + 1, cap + R.SPAN + 1,
              1 << 24, 1 << 31, (1 << 32) + 1, MAX_COUNT - 1, MAX_COUNT]
    sizes = [ws(1, n) for n in probes]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s > 0 for s in sizes)  # monotone in count ...
    assert all(s == R.MAX_GROUPS * R.PART_BYTES for n, s in zip(probes, sizes) if n >= cap)  # ... and flat beyond the cap
    for n in probes:  # proportional to the batch, a function of the arguments alone
        assert ws(7, n) == 7 * ws(1, n)
    for bad in [(0, 4), (-1, 4), (65536, 4), (1, 0), (1, MAX_COUNT + 1), (1, 1 << 40)]:
        assert ws(*bad) == 0


def test_argument_refusals(lib):
    """Every refusal is decided before any launch: it needs no device, and the pointers are never dereferenced."""
    p = C.c_void_p(4096)  # non-null, never touched
    big = 1 << 40
    nan, inf = float("nan"), float("inf")

    def call(pred=p, u8=1, target=p, batch=1, count=16, smooth=1.0, counts=p, scores=p, ws=p, nbytes=big):
        return lib.ocm_op_mask_scores(pred, u8, target, batch, count, smooth, counts, scores, ws, nbytes, None)

    def refused(rc, word):
        assert rc == _lib.OCM_EINVAL, rc
        assert word in lib.ocm_last_error().decode(), lib.ocm_last_error()

    for u8 in (0, 1):
        for name in ("pred", "target", "counts", "scores"):
            refused(call(u8=u8, **{name: None}), "null")
        for batch in (0, -1, 65536):
            refused(call(u8=u8, batch=batch), "batch")
        for count in (0, MAX_COUNT + 1, 1 << 63):
            refused(call(u8=u8, count=count), "count")
        for bad in (nan, inf, -inf, -1e-9):
            refused(call(u8=u8, smooth=bad), "smooth")
        for kw in (dict(nbytes=16), dict(ws=None), dict(nbytes=0),
                   dict(batch=3, count=5000, nbytes=lib.ocm_mask_scores_workspace_bytes(3, 5000) - 1)):
            assert call(u8=u8, **kw) == _lib.OCM_ENOMEM
            assert "workspace" in lib.ocm_last_error().decode()


def test_python_surface_refusals():
    from vit_ocm_wmsegmentation_amd import eval as E
    assert utils.SCORE_NAMES == R.SCORE_NAMES and utils.COUNT_NAMES == ("tp", "fp", "fn", "tn")
    mask, target = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError):  # no host fall-back
        utils.mask_scores(mask, target)
    with pytest.raises(RuntimeError):
        utils.mask_scores(mask.float(), target)
    with pytest.raises(RuntimeError):
        utils.calculate_metrics(target, mask.float())
    with pytest.raises(RuntimeError):
        utils.calculate_metrics(target, mask.float(), mask.float())
    with pytest.raises(ValueError):  # element counts differ
        utils.mask_scores(mask, torch.zeros(2, 8, 7))
    with pytest.raises(ValueError):
        utils.mask_scores(mask, torch.zeros(1, 8, 8))
    with pytest.raises(ValueError):
        utils.mask_scores(torch.zeros(0, 8, dtype=torch.uint8), torch.zeros(0, 8))
    for method in ("k-means", "k-means_ours"):  # cv2.kmeans: refused as segment_images refuses them
        with pytest.raises(ValueError):
            E.score_images(None, torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16), method=method)
        with pytest.raises(ValueError):
            E.validate(None, [(torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16))], method=method)
    with pytest.raises(ValueError):
        E.score_images(None, torch.zeros(1, 3, 16, 16), torch.zeros(1, 16, 16), median_filter=0)
    with pytest.raises(ValueError):
        E.validate(None, [])
