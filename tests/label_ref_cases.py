"""tdnet_op_upsample and tdnet_op_upsample_argmax against tests/out_ref.py, an evaluation that shares no text with the kernels: shared by
tests/test_emu_label_ref.py (CPU, through the emulator) and tests/test_gpu_label_ref.py (device memory).

Every other output form -- colour map, overlay, score, confidence, matte, composite, destination views, surfaces -- is held bit for bit to the
labels of tdnet_op_upsample_argmax, and the confidence and matte expectations to the logits of tdnet_op_upsample, by their own tests
(conf_cases.py, score_cases.py, out_cases.py, matte_cases.py, view_cases.py, overlay_cases.py, test_*_rgb_out.py).  Those tests share
td_up_coef / td_bilerp / td_up_classes / td_first_max with the kernels they take their expectation from, so "every form names the same
label" cannot see an error in that shared text.  This is where the two are held to something else.

The gates are out_ref's: the logits elementwise at band = 8 * 2^-24 * max|x|; the labels equal to the fp64 reference's first maximum wherever
its top two are more than 2 band apart or tie exactly, within 2 band of the maximum in between, such pixels capped at 1 % per case (asserted
on the reference alone).

The logits sit in a guarded mem (opcheck._Guarded) and every case runs once per input fill of opcheck._Guarded.POISONS: the quiet NaN, which a
comparison swallows, and 2^127, which it cannot.  Both runs must give the same bytes.

Measured with the unmodified kernels (the tests print every figure, pytest -s): max(err / band) of tdnet_op_upsample between 0.155 and 0.223 on
the cases of 5x9 / 4x8 / 13x25 source maps and at most 0.145 on the edge geometries, the same to the digit under the emulator and on the MI355X
(an expression of IEEE operations without contraction); on the device's own cases 0.209 / 0.245 (6 x 2051 at scales 1 / 40) and 0.189 / 0.206
(769 x 1537).  The near-tie share is 0 on every case."""
import numpy as np

import opcheck
import out_ref
from conf_cases import SCALES
from score_cases import ARGMAX_CASES, WIDE_CASES, lowres_logits

# the smallest geometries at which a coefficient rule can go wrong: one source pixel, one output row (scale 0 by definition), one source
# column, and 2 x 2 -> 7 x 7 (scale 1 / 6: not representable)
EDGE_CASES = [("edge_1x1", 5, (1, 1), (5, 8)), ("edge_one_row_out", 3, (4, 7), (1, 9)), ("edge_one_col_in", 4, (6, 1), (11, 5)), ("edge_2x2", 2, (2, 2), (7, 7))]
WIDE_SCALES = (1, 40)
# (name, C, (h, w), (H, W), scale)
CASES = [c + (s,) for c in list(ARGMAX_CASES) + EDGE_CASES for s in SCALES]
GPU_ONLY_CASES = [c + (s,) for c in WIDE_CASES for s in WIDE_SCALES]    # rows wider than one workgroup's strip, the real geometry
OFFSETS = (0, 1, 2, 3)
GUARD = 16


def case_id(c):
    return "%s-x%d" % (c[0], c[4])


def logits(name, C, h, w, scale):
    x = np.ascontiguousarray(lowres_logits(name, C, h, w) * np.float32(scale), dtype=np.float32)
    x.setflags(write=False)
    return x


_ref = {}


def reference(case):
    """(x, up_ref, labels, gap, band) of a case: computed once, read-only"""
    key = case_id(case)
    if key not in _ref:
        name, C, (h, w), (H, W), scale = case
        x = logits(name, C, h, w, scale)
        up = out_ref.up_ref(x, H, W)
        labels, gap, band = out_ref.labels_ref(x, H, W)
        for a in (up, labels, gap):
            a.setflags(write=False)
        _ref[key] = (x, up, labels, gap, band)
    return _ref[key]


def check(lib, mem, case):
    """mem: a guarded mem of opcheck with holder(nbytes, off) -> (address, read): room for nbytes at byte offset `off` inside a 0xEE holder
    whose GUARD bytes on either side read() asserts.  Returns (max err / band of the logits, near-tie share)."""
    name, C, (h, w), (H, W), scale = case
    x, up, ref_labels, gap, band = reference(case)
    who = case_id(case)
    n = H * W
    first_full = first_labels = None
    ratio = share = 0.0
    for poison in mem.POISONS:
        dx = mem.put(x, poison=poison)
        out = mem.empty((C, H, W))
        lib.check(lib.tdnet_op_upsample(mem.ptr(dx), C, h, w, H, W, mem.ptr(out), mem.stream))
        full = np.array(mem.get(out))
        ratio = out_ref.gate_upsample(full, up, band, (who, hex(poison)))
        for off in OFFSETS:
            p32, read32 = mem.holder(4 * n, 4 * off)
            p8, read8 = mem.holder(n, off)
            lib.check(lib.tdnet_op_upsample_argmax(mem.ptr(dx), C, h, w, H, W, p32, p8, mem.stream))
            l32 = read32().view(np.int32).reshape(H, W)
            l8 = read8().reshape(H, W)
            assert np.array_equal(l32, l8), (who, hex(poison), off)
            if first_labels is None:
                first_labels = l8
                share = out_ref.gate_labels(l8, up, ref_labels, gap, band, (who, hex(poison), off))
            assert np.array_equal(l8, first_labels), (who, hex(poison), off, "the labels depend on the band's fill or on the byte offset")
        mem.verify()
        first_full = full if first_full is None else first_full
        assert np.array_equal(full.view(np.int32), first_full.view(np.int32)), (who, "the logits depend on the band's fill")
    if name == "ties":                                                 # the case is what it is there for: exact ties, decided by the rule
        assert (gap == 0).mean() > 0.05, who                           # the tied source columns and the tied source row
    print("label_ref %-22s C %3d %dx%d -> %dx%d: upsample max err / band %.3f, near-tie share %.4f" % (who, C, h, w, H, W, ratio, share))
    return ratio, share


def check_up_ref_definition():
    """up_ref against F.interpolate(float64, bilinear, align_corners=True).  The two differ by the fp32 coordinate alone: f = s d carries two
    roundings of a value < max(h, w) (2^-23 max(h, w) in all, generously 2^-22), a coordinate error e moves a bilinear value by at most
    e * (the largest difference of neighbouring taps) <= 2 e max|x|: 2^-22 max(h, w) 2 max|x|.  On a geometry whose scale is representable
    and whose products are exact the two agree to the last float64 rounding.  CPU only.  Returns {case: (err, bound)}."""
    import torch
    import torch.nn.functional as F
    seen = {}
    for case in CASES + GPU_ONLY_CASES[:1]:
        name, C, (h, w), (H, W), scale = case
        x, up, _, _, _ = reference(case)
        ref = F.interpolate(torch.from_numpy(x.astype(np.float64))[None], (H, W), mode="bilinear", align_corners=True)[0].numpy()
        bound = 2.0 ** -22 * max(h, w) * 2.0 * float(np.abs(x).max())
        err = float(np.abs(up - ref).max())
        assert err <= bound, (case_id(case), err, bound)
        seen[case_id(case)] = (err, bound)
    return seen


class HolderMixin:
    """holder() for a guarded numpy mem; tests/test_gpu_label_ref.py has the device's"""
    def holder(self, nbytes, off):
        hold = np.full(nbytes + 2 * GUARD, 0xEE, np.uint8)

        def read():
            assert (hold[:GUARD + off] == 0xEE).all() and (hold[GUARD + off + nbytes:] == 0xEE).all(), off
            return hold[GUARD + off:GUARD + off + nbytes].copy()
        return hold.ctypes.data + GUARD + off, read


class HostMem(HolderMixin, opcheck.GuardedNumpyMem):
    pass
