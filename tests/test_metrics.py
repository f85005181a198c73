"""tdnet_amd.metrics.runningScore against what the reference's runningScore recorded for the same label maps (tests/golden/running_score.npz,
tools/make_golden_score.py): matrices equal, the four scores and the class IoUs within 1e-12 relative -- both sides are float64 evaluations of
the same few operations on exact integers -- with NaN in the same places; reset() and add_counts()."""
import os
import warnings

import numpy as np
import pytest

from tdnet_amd.metrics import SCORE_KEYS, confusion_counts, runningScore

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "running_score.npz"))
NAMES = [str(n) for n in GOLDEN["names"]]


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all(), (got, want)


def scores_of(rs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                 # nanmean of an all-NaN slice does not occur; 0 / 0 does
        return rs.get_scores()


def test_the_golden_holds_the_cases_it_should():
    assert NAMES == ["c19_ignore", "c19_two_updates", "c256", "c40_absent"]
    assert (GOLDEN["c19_ignore/gt"] == 255).mean() > 0.05 and GOLDEN["c19_two_updates/gt"].shape[0] == 2
    assert np.isnan(GOLDEN["c40_absent/class_iou"]).sum() >= 30 and not np.isnan(GOLDEN["c40_absent/scores"]).any()
    assert GOLDEN["c256/matrix"].shape == (256, 256)


@pytest.mark.parametrize("name", NAMES)
def test_running_score_equals_the_reference(name):
    n = int(GOLDEN[name + "/n_classes"])
    rs = runningScore(n)
    assert rs.n_classes == n and rs.confusion_matrix.shape == (n, n) and not rs.confusion_matrix.any()
    for gt, pred in zip(GOLDEN[name + "/gt"], GOLDEN[name + "/pred"]):
        rs.update([gt], [pred])
    assert rs.confusion_matrix.dtype == np.int64 and np.array_equal(rs.confusion_matrix, GOLDEN[name + "/matrix"])
    assert rs.confusion_matrix.sum() == (GOLDEN[name + "/gt"] < n).sum()
    score, cls_iu = scores_of(rs)
    assert tuple(score) == SCORE_KEYS == ("Overall Acc: \t", "Mean Acc : \t", "FreqW Acc : \t", "Mean IoU : \t")
    assert list(cls_iu) == list(range(n))
    close([score[k] for k in SCORE_KEYS], GOLDEN[name + "/scores"])
    close([cls_iu[i] for i in range(n)], GOLDEN[name + "/class_iou"])
    # a batch in one update() is the same sum; int32 predictions and int64 ground truth (what validate.py hands over) count the same
    rs2 = runningScore(n)
    rs2.update(GOLDEN[name + "/gt"].astype(np.int64), GOLDEN[name + "/pred"].astype(np.int32))
    assert np.array_equal(rs2.confusion_matrix, GOLDEN[name + "/matrix"])
    rs.reset()
    assert rs.confusion_matrix.shape == (n, n) and not rs.confusion_matrix.any()


@pytest.mark.parametrize("name", NAMES)
def test_add_counts_takes_a_device_matrix(name):
    n = int(GOLDEN[name + "/n_classes"])
    rs = runningScore(n)
    for gt, pred in zip(GOLDEN[name + "/gt"], GOLDEN[name + "/pred"]):
        rs.add_counts(confusion_counts(gt, pred, n).astype(np.uint64))  # uint64 is what tdnet_score_read fills
    assert np.array_equal(rs.confusion_matrix, GOLDEN[name + "/matrix"])
    score, cls_iu = scores_of(rs)
    close([score[k] for k in SCORE_KEYS], GOLDEN[name + "/scores"])
    close([cls_iu[i] for i in range(n)], GOLDEN[name + "/class_iou"])
    with pytest.raises(ValueError):
        rs.add_counts(np.zeros((n + 1, n + 1), np.int64))
    with pytest.raises(ValueError):
        rs.add_counts(np.zeros((n, n), np.float64))


def test_negative_ground_truth_is_ignored_like_255():
    gt = np.array([[0, 1, -1], [2, 255, 1]], np.int64)
    pred = np.array([[0, 2, 1], [2, 0, 1]], np.int64)
    want = np.zeros((3, 3), np.int64)
    want[0, 0] = want[1, 2] = want[2, 2] = want[1, 1] = 1
    assert np.array_equal(confusion_counts(gt, pred, 3), want)
