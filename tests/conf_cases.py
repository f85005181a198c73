"""Cases and expected values shared by tests/test_emu_conf.py (CPU, through the emulator) and tests/test_gpu_conf.py (device memory).

The expected values come from code that predates the confidence entries.  Expected LABELS: tdnet_op_upsample_argmax's.  Expected CONFIDENCE: the
fp32 full-resolution logits of tdnet_op_upsample (tdnet_forward for whole frames), softmax in numpy float64 with the maximum subtracted,
t = 255 p, want = floor(t + 0.5).

The gate.  A pixel is NEAR A BOUNDARY when |t - floor(t) - 0.5| < 2^-8.  The device byte must equal `want` at every other pixel and be within 1
of it at those.  Where 2^-8 comes from: the fp32 evaluation's relative error is about |d| 2^-24 from the exponent's argument (for the terms with
d > -30, which are the ones that contribute at all), an ulp or two of the hardware exp2 and of the reciprocal, C 2^-24 from the sum and 255 2^-24
from the scaling: about 3e-6 relative, 8e-4 of a byte step.  2^-8 = 3.9e-3 is five times that.  The share of near-boundary pixels is capped at
2 % per case -- a condition on the INPUTS, asserted here on the fp64 reference alone for every case handed out (0.2 - 1.1 % on the cases below;
the `ties` case, whose exact two-way ties are p = 0.5 = 127.5 exactly, is used at scale 1 only: scaled up, a tenth of its pixels sit on that
boundary)."""
import numpy as np

from score_cases import ARGMAX_CASES, WIDE_CASES, lowres_logits  # noqa: F401  (re-exported: the geometry sets)

NEAR = 2.0 ** -8
NEAR_CAP = 0.02
# x1: bytes of about 17..210; x6: the whole byte range up to 255; x40: |logit| up to about 360 -- a kernel that forgets the maximum overflows
SCALES = (1, 6, 40)
# (name, C, (h, w), (H, W), scale)
CASES = [c + (s,) for c in ARGMAX_CASES for s in SCALES if c[0] != "ties" or s == 1]
ALL_OFFSETS = tuple((lo, co) for lo in range(4) for co in range(4))     # (labels byte offset, confidence byte offset) inside their holders
FEW_OFFSETS = ((0, 0), (1, 2), (2, 3), (3, 1))
ALL_OFFSET_CASES = ("odd_w", "w_mult_of_4")
REJECT_LABELS = (255, 0, 19)


def case_id(c):
    return "%s-x%d" % (c[0], c[4])


def offsets_of(name):
    return ALL_OFFSETS if name in ALL_OFFSET_CASES else FEW_OFFSETS


def logits(name, C, h, w, scale):
    """the case's low-resolution logits [C, h, w] at `scale`, fp32"""
    x = np.ascontiguousarray(lowres_logits(name, C, h, w) * np.float32(scale), dtype=np.float32)
    x.setflags(write=False)
    return x


def expected(full, who=""):
    """(want uint8 [H, W], near bool [H, W]) of fp32 full-resolution logits [C, H, W]: float64 softmax with the maximum subtracted.  Asserts the
    2 % cap on the near-boundary share: a case that breaks it is a bad case, not a reason for a wider gate."""
    v = np.asarray(full, dtype=np.float64)
    assert np.isfinite(v).all(), who
    p = 1.0 / np.exp(v - v.max(axis=0, keepdims=True)).sum(axis=0)
    t = 255.0 * p
    want = np.floor(t + 0.5)
    assert want.min() >= 0 and want.max() <= 255, who
    near = np.abs(t - np.floor(t) - 0.5) < NEAR
    assert near.mean() <= NEAR_CAP, (who, near.mean())
    return want.astype(np.uint8), near


def gate(got, want, near, who=""):
    """the device bytes `got` against (want, near) of expected()"""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (who, got.shape, want.shape)
    bad = (got != want) & ~near
    assert not bad.any(), (who, int(bad.sum()), got[bad][:8], want[bad][:8])
    assert (np.abs(got - want)[near] <= 1).all(), (who, got[near][:8], want[near][:8])


def rejected(labels, conf, min_conf, reject_label):
    """the label map the contract defines from the confidence BYTES the kernel itself wrote"""
    return np.where(np.asarray(conf) < min_conf, reject_label, np.asarray(labels)).astype(np.uint8)


def thresholds(conf):
    """min_conf values of the rejection tests: fixed ones and one between the case's own minimum and maximum byte"""
    lo, hi = int(np.min(conf)), int(np.max(conf))
    return (1, 64, 128, 255, max(1, (lo + hi + 1) // 2))
