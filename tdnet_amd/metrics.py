"""Segmentation scores from a confusion matrix, with the interface of the reference's Training/ptsemseg/metrics.py runningScore: update() on host
label arrays, get_scores(), reset(), confusion_matrix -- plus add_counts() for the matrix a device handle counted (include/tdnet.h "score out").

The matrix is kept as exact int64 counts; get_scores() evaluates the reference's formulas on it in float64, nanmean semantics included: a class
absent from both ground truth and prediction has IoU 0 / 0 = NaN and is left out of the mean, a class absent from the ground truth has NaN accuracy."""
import numpy as np

SCORE_KEYS = ("Overall Acc: \t", "Mean Acc : \t", "FreqW Acc : \t", "Mean IoU : \t")


def confusion_counts(label_true, label_pred, n_classes):
    """int64 [n_classes, n_classes]: rows ground truth, columns prediction, over the pixels with 0 <= ground truth < n_classes."""
    t = np.asarray(label_true).reshape(-1).astype(np.int64)
    p = np.asarray(label_pred).reshape(-1).astype(np.int64)
    keep = (t >= 0) & (t < n_classes)
    return np.bincount(n_classes * t[keep] + p[keep], minlength=n_classes * n_classes).reshape(n_classes, n_classes)


class runningScore(object):
    def __init__(self, n_classes):
        self.n_classes = int(n_classes)
        self.reset()

    def reset(self):
        self.confusion_matrix = np.zeros((self.n_classes, self.n_classes), np.int64)

    def update(self, label_trues, label_preds):
        for lt, lp in zip(label_trues, label_preds):
            self.confusion_matrix += confusion_counts(lt, lp, self.n_classes)

    def add_counts(self, matrix):
        """Add a matrix of counts [n_classes, n_classes] (any integer dtype), e.g. what a device handle read out."""
        m = np.asarray(matrix)
        if m.shape != self.confusion_matrix.shape or m.dtype.kind not in "iu":
            raise ValueError("add_counts: an integer matrix %r expected, got %s %r" % (self.confusion_matrix.shape, m.dtype, m.shape))
        self.confusion_matrix += m.astype(np.int64)

    def get_scores(self):
        """({overall accuracy, mean accuracy, frequency-weighted accuracy, mean IoU} under the reference's keys, {class: IoU})."""
        hist = self.confusion_matrix.astype(np.float64)
        diag, rows, cols, total = np.diag(hist), hist.sum(axis=1), hist.sum(axis=0), hist.sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = diag.sum() / total
            acc_cls = np.nanmean(diag / rows)
            iu = diag / (rows + cols - diag)
            mean_iu = np.nanmean(iu)
            freq = rows / total
            fwavacc = (freq[freq > 0] * iu[freq > 0]).sum()
        return dict(zip(SCORE_KEYS, (acc, acc_cls, fwavacc, mean_iu))), dict(zip(range(self.n_classes), iu))
