"""An evaluation of the output stage that shares no text with csrc/td_out.h: the bilinear upsample (align_corners=True) and the first maximum
over classes, in numpy.  tests/label_ref_cases.py holds tdnet_op_upsample and tdnet_op_upsample_argmax to it; every other output form is held
bit for bit to those two by its own tests, so this is where the whole stage is anchored.

The COEFFICIENTS follow the reference's fp32 rule and are written in numpy float32:
    s = f32(n_in - 1) / f32(n_out - 1)   (0 for n_out == 1),   f = s * f32(d),   i0 = int(f),   i1 = i0 + (i0 < n_in - 1),   l = f - f32(i0)
Each is one IEEE operation and the library is built with -ffp-contract=off, so these are the device's values exactly: which source pixels a
result reads is not a matter of tolerance.  The four-tap INTERPOLATION is float64.

The band.  The fp32 expression (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11) has four products, three sums and the two 1 - l
(half an ulp of a value <= 1).  Every intermediate is a convex combination of the taps, so at most max|x| in size, and each operation is
within half an ulp (2^-24 relative) of it.  Inside a row: 1 - lx, two products, one sum -- four roundings, and the two rows enter the result
with the weights 1 - ly and ly, which add up to 1: 4 in all.  Outside: 1 - ly, two products, one sum: 4 more.  So
    band = 8 * 2^-24 * max|x|
A numpy-float32 restatement of the expression stays below 0.24 band on every case of tests/label_ref_cases.py, at scales 1 and 40."""
import numpy as np

EPS = 2.0 ** -24


def coef(n_in, n_out):
    """(i0, i1, l) of every output index 0 .. n_out - 1: int64, int64, float32"""
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)
    f = (s * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = f.astype(np.int64)                                            # f >= 0: truncation
    i1 = i0 + (i0 < n_in - 1)
    l = (f - i0.astype(np.float32)).astype(np.float32)
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and l.min() >= 0 and l.max() < 1
    return i0, i1, l


def up_ref(x, H, W):
    """float64 [C, H, W] of fp32 low-resolution logits [C, h, w].  Non-finite logits take part as IEEE has it (0 * inf is a NaN, here and in
    the kernels)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    C, h, w = x.shape
    y0, y1, ly = coef(h, H)
    x0, x1, lx = coef(w, W)
    v = x.astype(np.float64)
    ly = ly.astype(np.float64)[None, :, None]
    lx = lx.astype(np.float64)[None, None, :]
    with np.errstate(invalid="ignore"):
        top = (1.0 - lx) * v[:, y0][:, :, x0] + lx * v[:, y0][:, :, x1]
        bot = (1.0 - lx) * v[:, y1][:, :, x0] + lx * v[:, y1][:, :, x1]
        return (1.0 - ly) * top + ly * bot


def band_of(x):
    return 8.0 * EPS * float(np.abs(np.asarray(x, np.float64)).max())


def labels_ref(x, H, W):
    """(labels int64 [H, W], gap float64 [H, W], band): the first maximum of up_ref, the reference's top-2 gap (inf for one class), the band"""
    up = up_ref(x, H, W)
    labels = np.argmax(up, axis=0)                                     # numpy's argmax names the first of equal maxima
    if up.shape[0] == 1:
        gap = np.full((H, W), np.inf)
    else:
        top2 = np.partition(up, up.shape[0] - 2, axis=0)[-2:]
        gap = top2[1] - top2[0]
    return labels, gap, band_of(x)


NEAR_TIE_CAP = 0.01


def gate_labels(got, up, labels, gap, band, who=""):
    """Device labels `got` [H, W] against labels_ref's: equal where the reference's top two are further apart than both evaluations can move
    (2 band); equal where they tie exactly (the first maximum is a rule, not a rounding); in between, the class named must be within 2 band
    of the reference's maximum.  The share of in-between pixels is capped at 1 %: a condition on the INPUTS, asserted on the reference
    alone.  Returns that share."""
    got = np.asarray(got).astype(np.int64)
    assert got.shape == labels.shape, (who, got.shape, labels.shape)
    C = up.shape[0]
    assert got.min() >= 0 and got.max() < C, (who, int(got.min()), int(got.max()))
    near = (gap > 0) & (gap <= 2 * band)
    share = float(near.mean())
    assert share <= NEAR_TIE_CAP, (who, "near-tie share", share)
    firm = ~near
    bad = firm & (got != labels)
    assert not bad.any(), (who, "labels differ from the fp64 reference at %d of %d pixels outside the tie band" % (int(bad.sum()), bad.size),
                           [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]], got[bad][:4], labels[bad][:4], gap[bad][:4], band)
    if near.any():
        named = np.take_along_axis(up, got[None], axis=0)[0]
        off = (up.max(axis=0) - named)[near]
        assert (off <= 2 * band).all(), (who, "a near-tie pixel names a class further than 2 band below the maximum", float(off.max()), band)
    return share


def gate_upsample(got, up, band, who=""):
    """fp32 full-resolution logits `got` against up_ref elementwise at band; returns max(err / band) (0 when the logits are all zero)"""
    err = np.abs(np.asarray(got, np.float64) - up)
    worst = float(err.max())
    assert worst <= band, (who, "upsample error %.3e over the band %.3e" % (worst, band), tuple(int(i) for i in np.unravel_index(int(np.argmax(err)), err.shape)))
    return worst / band if band > 0 else 0.0


def first_max_rule(v):
    """The label rule as the sources state it (td_out.h td_first_max), in numpy on values [C, ...]: class 0 starts the running maximum, class
    c replaces it where v[c] > best.  A NaN compares false on either side: it never replaces the maximum, and a NaN in class 0 is never
    replaced.  Equal to np.argmax wherever no value of the pixel is a NaN."""
    v = np.asarray(v)
    best, bi = v[0].copy(), np.zeros(v.shape[1:], np.int64)
    with np.errstate(invalid="ignore"):
        for c in range(1, v.shape[0]):
            up = v[c] > best
            best = np.where(up, v[c], best)
            bi = np.where(up, c, bi)
    return bi
