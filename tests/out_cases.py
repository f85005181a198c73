"""One cross-form check of the output stage (csrc/td_out.h), shared by tests/test_emu_out.py (CPU, through the emulator) and
tests/test_gpu_out.py (device memory): the SAME low-resolution logits leave through every output form the operator entries reach -- int32
labels, uint8 labels, the score entry's labels and matrix, the confidence entry's labels in both pass forms, the colour map read back as
labels -- and every form must name the same label under every pixel.  All comparisons are exact: the forms share one bilinear expression,
one first-maximum rule and one class loop, there is nothing to tolerate.

The logits sit between guard bands (opcheck._Guarded) and the whole check runs once per band fill of opcheck._Guarded.POISONS -- the quiet NaN, which
td_first_max's comparison swallows, and 2^127, which it cannot: an out-of-range read of logits names another class under one of the two, and
the labels of the two runs must be the same bytes.

The byte maps start at byte offsets 0..3 inside their holders.  The int32 map is moved by 0..3 ELEMENTS instead: an int32_t* that is not
4-byte aligned is outside the C ABI of the entry."""
import numpy as np

import opcheck

# (C, (h, w), (H, W)): 3 and 19 classes; 5x9 -> 33x65, and 4x7 -> 25x49 (W odd: the rows of a map start at every alignment)
CASES = [(C, lo, hi) for C in (3, 19) for lo, hi in (((5, 9), (33, 65)), ((4, 7), (25, 49)))]
FIELDS = ("noise", "ties")
OFFSETS = (0, 1, 2, 3)
GUARD = 16


def case_id(c):
    return "c%d-%dx%d" % (c[0], c[2][0], c[2][1])


def logits(field, C, h, w):
    """fp32 [C, h, w].  noise: standard normal.  ties: small integers (every interpolated value is exact, equal values meet often), the
    last class plane a copy of the first and (C > 3) class 1 a copy of class 2, a constant left half and a constant top row: the first
    maximum and the c == 0 start decide most pixels."""
    rng = np.random.default_rng(1000 * C + 10 * h + w + FIELDS.index(field))
    if field == "noise":
        x = rng.standard_normal((C, h, w))
    else:
        x = rng.integers(-2, 3, (C, h, w)).astype(np.float64)
        x[:, :, : w // 2] = 1.0
        x[:, 0, :] = -1.0
        x[C - 1] = x[0]
        if C > 3:
            x[1] = x[2]
    x = np.ascontiguousarray(x, dtype=np.float32)
    x.setflags(write=False)
    return x


def grey_palette():
    """colour l = (l, l, l): the picture's bytes are the labels"""
    return np.ascontiguousarray(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1))


def ground_truth(C, H, W):
    rng = np.random.default_rng(C + H + W)
    gt = rng.integers(0, C, (H, W)).astype(np.uint8)
    gt[rng.random((H, W)) < 0.1] = 255
    return np.ascontiguousarray(gt)


def check(lib, mem, setenv, case, field):
    """mem: the memory the entries work on -- mem.put(array) -> (keepalive, pointer), mem.put_logits(array, poison) -> the same between guard bands
    of that fill, mem.holder(nbytes, off) -> (pointer, read) with read() the nbytes written behind `off` (it asserts the 0xEE guard bytes around
    them), mem.stream.  setenv: monkeypatch.setenv."""
    ref = None
    for poison in opcheck._Guarded.POISONS:
        ref = _check(lib, mem, setenv, case, field, poison, ref)


def _check(lib, mem, setenv, case, field, poison, ref):
    C, (h, w), (H, W) = case
    n = H * W
    x_keep, x = mem.put_logits(logits(field, C, h, w), poison)
    gt_keep, gt = mem.put(ground_truth(C, H, W))
    pal = grey_palette()
    s = mem.stream
    for off in OFFSETS:
        who = (case_id(case), field, off, hex(poison))
        # int32 and uint8 labels, one call
        p32, read32 = mem.holder(4 * n, 4 * off)
        p8, read8 = mem.holder(n, off)
        lib.check(lib.tdnet_op_upsample_argmax(x, C, h, w, H, W, p32, p8, s))
        l32 = read32().view(np.int32).reshape(H, W)
        l8 = read8().reshape(H, W)
        assert l32.min() >= 0 and l32.max() < C, who
        assert np.array_equal(l32, l8), who
        ref = l8 if ref is None else ref
        assert np.array_equal(l8, ref), who                             # a pixel's label does not depend on which lane computed it
        # the score entry: its labels, and its matrix against the one k_labels_score counts from the uint8 map
        cms = []
        for labels_in in (False, True):
            cm_keep, cm = mem.put(np.zeros((C, C), np.uint64))
            ps, reads = mem.holder(n, (off + 1) & 3)
            if labels_in:
                lab_keep, lab = mem.put(l8)
                lib.check(lib.tdnet_op_upsample_argmax_score(None, C, 0, 0, H, W, gt, None, None, cm, lab, s))
            else:
                lib.check(lib.tdnet_op_upsample_argmax_score(x, C, h, w, H, W, gt, None, ps, cm, None, s))
                assert np.array_equal(reads().reshape(H, W), l8), who
            cms.append(mem.get(cm_keep))
        assert cms[0].sum() > 0 and np.array_equal(cms[0], cms[1]), who
        # the confidence entry with min_conf = 0, one pass and two passes
        for passes in ("1", "2"):
            setenv("TDNET_CONF_PASSES", passes)
            pl, readl = mem.holder(n, off)
            pc, readc = mem.holder(n, (off + 2) & 3)
            lib.check(lib.tdnet_op_upsample_argmax_conf(x, C, h, w, H, W, pl, pc, 0, 255, None, s))
            assert np.array_equal(readl().reshape(H, W), l8), who + (passes,)
            readc()
        # the colour map at the labels' own size through a grey palette
        pr, readr = mem.holder(3 * n, off)
        lib.check(lib.tdnet_op_upsample_argmax_rgb(x, C, h, w, H, W, H, W, pal.ctypes.data, 256, pr, None, s))
        pic = readr().reshape(H, W, 3)
        assert np.array_equal(pic, np.repeat(l8[:, :, None], 3, axis=2)), who
    if field == "ties":
        assert (ref == 0).any() and (ref == C - 1).sum() == 0, case_id(case)   # the first of two equal planes wins everywhere
    x_keep.verify()                                                    # the bands around the logits are intact
    del x_keep, gt_keep
    return ref
