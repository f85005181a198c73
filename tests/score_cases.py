"""Cases and expected values shared by tests/test_emu_score.py (CPU, through the emulator) and tests/test_gpu_score.py (device memory).

The expected confusion matrix comes from code that predates the score entries: np.bincount with the reference's mask (Training/ptsemseg/metrics.py
_fast_hist) on the labels of tdnet_op_upsample_argmax.  Every comparison the two test files make is exact: the counts are integers."""
import numpy as np

from ingest_u8_cases import ARGMAX_CASES as _ARGMAX_CASES, lowres_logits  # noqa: F401  (re-exported: the logits of the operator cases)

LDS_CLASSES = 64                                                       # td_score.h TD_SCORE_LDS_CLASSES: private LDS histograms up to here, global atomics above
# (name, C, (h, w), (H, W)): the label cases + a class count on each side of that threshold
ARGMAX_CASES = list(_ARGMAX_CASES) + [("c64_lds", LDS_CLASSES, (5, 9), (33, 65)), ("c65_global", LDS_CLASSES + 1, (5, 9), (33, 65))]
# rows wider than one workgroup's strip (256 lanes x 4 pixels) and the real geometry: GPU only
WIDE_CASES = [("wide", 19, (2, 300), (6, 2051)), ("native_769x1537", 19, (97, 193), (769, 1537))]
GT_KINDS = ("noise", "blocky", "one_id", "all_ignored", "labels")
# (gt byte offset, labels byte offset) inside their holders: every offset 0..3 on either side
OFFSETS = ((0, 0), (1, 2), (2, 3), (3, 1))


def ground_truth(kind, C, labels):
    """uint8 [H, W].  noise: uniform in [0, C) with about 10 % 255; blocky: 8 x 16 tiles of one id (about one tile in eight 255); one_id: C // 2
    everywhere; all_ignored: 255 everywhere (at C = 256 that is class 255: nothing is ignored there without a map); labels: the labels themselves."""
    H, W = labels.shape
    rng = np.random.default_rng(C * 7919 + H * 131 + W + GT_KINDS.index(kind))
    if kind == "noise":
        gt = rng.integers(0, C, (H, W)).astype(np.uint8)
        gt[rng.random((H, W)) < 0.1] = 255
    elif kind == "blocky":
        tiles = rng.integers(0, C, ((H + 7) // 8, (W + 15) // 16)).astype(np.uint8)
        tiles[rng.random(tiles.shape) < 0.125] = 255
        gt = np.repeat(np.repeat(tiles, 8, axis=0), 16, axis=1)[:H, :W]
    elif kind == "one_id":
        gt = np.full((H, W), C // 2, np.uint8)
    elif kind == "all_ignored":
        gt = np.full((H, W), 255, np.uint8)
    else:
        gt = labels.astype(np.uint8)
    return np.ascontiguousarray(gt)


def expected_matrix(gt, labels, C, gt_map=None):
    """int64 [C, C]: bincount(C * g + label) over the pixels with g = gt_map[gt] < C (the reference's mask on bytes)."""
    g = np.asarray(gt).astype(np.int64) if gt_map is None else np.asarray(gt_map, np.int64)[np.asarray(gt)]
    keep = g < C
    return np.bincount(C * g[keep] + np.asarray(labels).astype(np.int64)[keep], minlength=C * C).reshape(C, C)


def permuting_map(C, seed=5):
    """256 bytes: a permutation of the class ids on [0, C), every fourth id folded to 255 instead, bytes >= C folded to 255 too.  255 means
    "ignore" for C < 256; at C = 256 no byte is >= nclass, so there the map only permutes (255 is then class 255 like any other)."""
    rng = np.random.default_rng(seed)
    m = np.full(256, 255, np.uint8)
    m[:C] = rng.permutation(C).astype(np.uint8)
    m[:C:4] = 255
    return m
