#!/usr/bin/env python3
"""Generate tests/golden/running_score.npz by running the REAL reference's runningScore (Training/ptsemseg/metrics.py, imported read-only; it
needs only numpy) on a handful of small (ground truth, prediction) pairs.  Data only: per pair the two label maps, the confusion matrix, the
four scores and the per-class IoUs; tests/test_metrics.py compares tdnet_amd.metrics.runningScore against them.

    python tools/make_golden_score.py --reference /path/to/TDNet"""
import argparse
import importlib.util
import os
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("Overall Acc: \t", "Mean Acc : \t", "FreqW Acc : \t", "Mean IoU : \t")


def pairs():
    """name -> (n_classes, [(gt, pred), ...]): one update() per listed pair."""
    rng = np.random.default_rng(2026)
    out = {}
    gt = rng.integers(0, 19, (33, 65)).astype(np.uint8)                # 19 classes, about 10 % of the ground truth ignored (255)
    gt[rng.random((33, 65)) < 0.1] = 255
    out["c19_ignore"] = (19, [(gt, rng.integers(0, 19, (33, 65)).astype(np.uint8))])
    out["c256"] = (256, [(rng.integers(0, 256, (8, 12)).astype(np.uint8), rng.integers(0, 256, (8, 12)).astype(np.uint8))])
    present = np.array([0, 3, 4, 9, 17, 22, 38])                       # 40 classes, most of them absent from both maps: NaN IoUs
    gt = present[rng.integers(0, len(present), (33, 65))].astype(np.uint8)
    pred = np.where(rng.random((33, 65)) < 0.7, gt, present[rng.integers(0, len(present) - 1, (33, 65))]).astype(np.uint8)
    out["c40_absent"] = (40, [(gt, pred)])
    seq = []
    for _ in range(2):                                                 # a sequence of two updates
        gt = rng.integers(0, 19, (33, 65)).astype(np.uint8)
        gt[rng.random((33, 65)) < 0.1] = 255
        seq.append((gt, np.where(rng.random((33, 65)) < 0.6, np.minimum(gt, 18), rng.integers(0, 19, (33, 65))).astype(np.uint8)))
    out["c19_two_updates"] = (19, seq)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TDNET_REFERENCE"), required="TDNET_REFERENCE" not in os.environ,
                    help="checkout of the reference project (its Training/ptsemseg/metrics.py is imported)")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(a.reference, "Training", "ptsemseg", "metrics.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cases = pairs()
    data = {"names": np.array(sorted(cases))}
    for name, (n, seq) in cases.items():
        rs = ref.runningScore(n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for gt, pred in seq:
                rs.update([gt], [pred])
            score, cls_iu = rs.get_scores()
        assert tuple(score) == KEYS
        data[name + "/n_classes"] = np.int64(n)
        data[name + "/gt"] = np.stack([g for g, _ in seq])
        data[name + "/pred"] = np.stack([p for _, p in seq])
        data[name + "/matrix"] = rs.confusion_matrix.astype(np.int64)
        assert np.array_equal(data[name + "/matrix"], rs.confusion_matrix)
        data[name + "/scores"] = np.array([score[k] for k in KEYS], np.float64)
        data[name + "/class_iou"] = np.array([cls_iu[i] for i in range(n)], np.float64)
    path = os.path.join(ROOT, "tests", "golden", "running_score.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
