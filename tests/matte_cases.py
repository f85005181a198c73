"""Cases and expected values shared by tests/test_emu_matte.py (CPU, through the emulator), tests/test_gpu_matte.py (device memory) and
tests/test_matte_host.py.

The expected values come from code that predates the matte entries.  Expected LABELS: tdnet_op_upsample_argmax's.  Expected MATTE: the fp32
full-resolution logits of tdnet_op_upsample (tdnet_forward* for whole frames), softmax in numpy float64 with the maximum subtracted, summed over
the members of the set, t = 255 num / den, want = floor(t + 0.5).

The gate is tests/conf_cases.py's, with the same derivation: a pixel is NEAR A BOUNDARY when |t - floor(t) - 0.5| < 2^-8; the device byte must
equal `want` at every other pixel and be within 1 of it at those.  The error budget is the confidence kernel's -- every term of num and den is
positive (no cancellation), the same exponent arguments, an ulp or two of exp2 and of the ONE division, C 2^-24 from either sum, 255 2^-24 from
the scaling, and t <= 255: about 8e-4 of a byte step against 2^-8 = 3.9e-3.  The share of near-boundary pixels is capped at 2 % per case AND
SET, asserted here on the float64 reference alone for every pair handed out (`ties` at scale 1 only, as there).

What is exact is compared exactly, by the tests themselves: every class -> 255, the empty set -> 0, the labels, one byte per pixel."""
import ctypes

import numpy as np

import opcheck

from conf_cases import ALL_OFFSETS, ALL_OFFSET_CASES, FEW_OFFSETS, NEAR, NEAR_CAP, SCALES, gate, logits, offsets_of  # noqa: F401  (re-exported)
from ingest_u8_cases import ARGMAX_CASES
from score_cases import WIDE_CASES  # noqa: F401  (re-exported: rows wider than one workgroup's strip, and the real geometry)

# (name, C, (h, w), (H, W), scale): odd_w, w_mult_of_4, native 97x193, c256, c1 at x1 / x6 / x40, ties at x1
CASES = [c + (s,) for c in ARGMAX_CASES for s in SCALES if c[0] != "ties" or s == 1]
MOVING = tuple(range(11, 19))                                          # Cityscapes train ids 11..18: person .. bicycle


def case_id(c):
    return "%s-x%d" % (c[0], c[4])


def class_sets(C):
    """{name: ids} of the sets a case with C classes is run with; ids below C only.  `high` (C = 256): classes >= 224 only, and `last` holds
    class C - 1 -- at C = 256 both live in the last membership word alone."""
    sets = {"every": tuple(range(C)), "empty": (), "first": (0,), "last": (C - 1,), "odd": tuple(range(1, C, 2))}
    if C > MOVING[-1]:
        sets["moving"] = MOVING
    if C == 256:
        sets["high"] = tuple(range(224, 256, 3))
        sets["with_255"] = (3, 40, 100, 255, 255)                      # a duplicate is legal
    return {k: v for k, v in sets.items() if k in ("every", "empty") or 0 < len(set(v)) < C}


def complement(C, ids):
    return tuple(c for c in range(C) if c not in set(ids))


def ids_array(ids):
    """the ids as the uint8 host array the C entries take (at least one element, so that there is an address)"""
    a = np.zeros(max(1, len(ids)), np.uint8)
    a[:len(ids)] = ids
    return a


def expected(full, ids, who=""):
    """(want uint8 [H, W], near bool [H, W]) of fp32 full-resolution logits [C, H, W] and a class set: float64 softmax with the maximum
    subtracted.  Asserts the 2 % cap on the near-boundary share: a pair that breaks it is a bad pair, not a reason for a wider gate."""
    v = np.asarray(full, dtype=np.float64)
    assert np.isfinite(v).all(), who
    member = np.zeros(v.shape[0], bool)
    member[list(ids)] = True
    e = np.exp(v - v.max(axis=0, keepdims=True))
    t = 255.0 * (e[member].sum(axis=0) / e.sum(axis=0))
    want = np.floor(t + 0.5)
    assert want.min() >= 0 and want.max() <= 255, who
    near = np.abs(t - np.floor(t) - 0.5) < NEAR
    assert near.mean() <= NEAR_CAP, (who, near.mean())
    return want.astype(np.uint8), near


# ---- the operator on any memory ----------------------------------------------------------------------------------------------------------
# `mem` stands for the memory a scenario runs in, as in view_cases.py: mem.up(array, off=0) -> (holder, address); mem.get(buffer) -> numpy
# (synchronises); mem.stream.
def _is_array(a):
    return a is not None and not isinstance(a, int)


def matte_op(lib, mem, C, H, W, ids, x=None, h=0, w=0, full=None, lab_off=0, mat_off=0, want_labels=True):
    """One call of tdnet_op_upsample_argmax_matte: (labels written or None, matte written) as numpy.  x / full: the low-resolution / full-resolution
    logits -- an ADDRESS in `mem`, or the ARRAY itself: it then goes in between guard bands, once per band fill, and both runs must give the same
    bytes (opcheck.each_poison).  Either map sits at its byte offset inside a 0xEE holder whose 16 guard bytes must survive."""
    dev = mem.stream is not None
    if _is_array(x):
        return opcheck.each_poison(x, dev, lambda px: matte_op(lib, mem, C, H, W, ids, px, h, w, full, lab_off, mat_off, want_labels))
    if _is_array(full):
        return opcheck.each_poison(full, dev, lambda pf: matte_op(lib, mem, C, H, W, ids, x, h, w, pf, lab_off, mat_off, want_labels))
    n = H * W
    mh, mp = mem.up(np.full(n + 16, 0xEE, np.uint8))
    lh, lp = mem.up(np.full(n + 16, 0xEE, np.uint8)) if want_labels else (None, None)
    cls = ids_array(ids)
    lib.check(lib.tdnet_op_upsample_argmax_matte(x, C, h, w, H, W, None if lp is None else lp + lab_off, mp + mat_off, cls.ctypes.data if len(ids) else None, len(ids),
                                                 full, mem.stream))
    mhost = mem.get(mh)[:n + 16]
    assert (mhost[:mat_off] == 0xEE).all() and (mhost[mat_off + n:] == 0xEE).all(), (lab_off, mat_off)
    lab = None
    if lh is not None:
        lhost = mem.get(lh)[:n + 16]
        assert (lhost[:lab_off] == 0xEE).all() and (lhost[lab_off + n:] == 0xEE).all(), (lab_off, mat_off)
        lab = lhost[lab_off:lab_off + n].reshape(H, W).copy()
    return lab, mhost[mat_off:mat_off + n].reshape(H, W).copy()


# ---- the composite -------------------------------------------------------------------------------------------------------------------------
# Every comparison is EXACT against dataloader.composite_u8 applied to the matte bytes the matte operator itself wrote for the same logits.
import surface_cases as sc  # noqa: E402
import view_cases as vc  # noqa: E402
from tdnet_amd.dataloader import (PIX_BGR24, PIX_BGRA32, PIX_NV12, PIX_RGB24, PIX_RGBA32, SURF_I420, SURF_P010, SourceView, composite_u8,  # noqa: E402
                                  surface_extent, surface_to_rgb_u8, view_extent, view_to_rgb_u8, write_view)

NET, LOW = (33, 65), (5, 9)
SIZES = {"up_41x83": (41, 83), "down_17x29": (17, 29), "same_33x65": (33, 65)}
BG = (200, 30, 90)                                                     # three distinct bytes: an r / b mix-up shows
GUARD, GUARD_BYTE = 64, 0xEE
FILLS = (0xA5, 0x00)
SOURCE_KINDS = ("rgb24", "bgr24", "rgba32", "bgra32", "nv12", "i420", "p010")
PACKED = {"rgb24": PIX_RGB24, "bgr24": PIX_BGR24, "rgba32": PIX_RGBA32, "bgra32": PIX_BGRA32}


def comp_source(kind, size, seed=1):
    """(description, bytes, true r g b [h, w, 3], the source's bytes are b g r) of a source whose rectangle is `size`: a crop at an odd origin and a
    pitch with padding, or a padded surface."""
    h, w = size
    if kind in PACKED:
        view = vc.packed_view(PACKED[kind], (3, 7, h, w), frame=(h + 9, w + 7))
        b = vc.packed_bytes(view, 0x77, seed)
        return view, b, view_to_rgb_u8(b, view), kind.startswith("bgr")
    if kind == "nv12":
        view = vc.nv12_view((3, 7, h, w), 1, frame=(h + 10, w + 8), standard=1)
        b = vc.nv12_bytes(view, 0x77, seed)
        return view, b, view_to_rgb_u8(b, view), False
    surf = sc.surface({"i420": SURF_I420, "p010": SURF_P010}[kind], (3, 5, h, w), "padded", frame=(h + 10, w + 8), standard=2)
    b = sc.surface_bytes(surf, 0x77, seed)
    return surf, b, surface_to_rgb_u8(b, surf), False


def comp_dest(fmt, size):
    h, w = size
    return SourceView(fmt, h + 9, w + 13, pitch=(w + 13) * vc.BPP[fmt] + 5, crop=(3, 5, h, w))


def expected_dest(prefill, dview, picture_rgb, alpha=None):
    """write_view of the true r g b picture; alpha: the matte bytes [h, w] that are the rectangle's x bytes (the alpha mode)."""
    out = write_view(prefill, dview, picture_rgb)
    if alpha is not None:
        y0, x0, h, w = dview.rect
        idx = (y0 + np.arange(h))[:, None] * dview.row_pitch + (x0 + np.arange(w))[None, :] * 4 + 3
        out[idx] = alpha
    return out


def op_composite(lib, mem, src, src_off, dview, prefill, dst_off, bg, x=None, ids=(), matte=None):
    """tdnet_op_composite into a guarded copy of `prefill` (dview None: the contiguous block of prefill.size bytes): the whole buffer back, and the
    offset of the destination's base in it.  x: logits [19, 5, 9] -- an ADDRESS in `mem`, or the ARRAY: between guard bands, once per band fill, the
    same bytes both times (opcheck.each_poison); or matte: a map [H, W] (uploaded at an odd address)."""
    if _is_array(x):
        return opcheck.each_poison(x, mem.stream is not None, lambda px: op_composite(lib, mem, src, src_off, dview, prefill, dst_off, bg, px, ids, matte))
    H, W = NET
    desc, sbytes = src[0], src[1]
    host = np.full(GUARD + dst_off + prefill.size + GUARD, GUARD_BYTE, np.uint8)
    base = GUARD + dst_off
    host[base:base + prefill.size] = prefill
    kd, pd = mem.up(host)
    ks, ps = mem.up(sbytes, src_off)
    is_surf = not isinstance(desc, SourceView)
    keep_s, pts = sc.csurf(desc) if is_surf else vc.cview(desc)
    keep_d, ptd = vc.cview(dview) if dview is not None else (None, None)
    cls = ids_array(ids)
    km, pm = mem.up(matte, 1) if matte is not None else (None, None)
    bgb = None if bg is None else (ctypes.c_uint8 * 3)(*bg)
    lib.check(lib.tdnet_op_composite(None if matte is not None else x, 19, LOW[0], LOW[1], H, W, cls.ctypes.data if len(ids) else None, len(ids), pm, ps,
                                     None if is_surf else pts, pts if is_surf else None, pd + base, ptd, 0 if bg is not None else 1, bgb, mem.stream))
    return mem.get(kd)[:host.size].copy(), host, base


def check_composite(lib, mem, src, dview, matte, bg, x, ids, offsets=range(4), fills=FILLS, what=""):
    """The fused kernel and the kernel on the matte map `matte` (the matte operator's bytes for x and ids), at every base offset and prefill: the
    WHOLE guarded buffer equals the oracle's picture in the rectangle's pixel bytes and the prefill / the guards everywhere else."""
    desc, sbytes, rgb, bgr = src
    H, W = NET
    size = rgb.shape[:2]
    if bg is not None:
        pic = composite_u8(rgb, matte, H, W, bg)
        alpha = None
    else:
        rgba = composite_u8(rgb, matte, H, W, None)
        pic, alpha = np.ascontiguousarray(rgba[..., :3]), rgba[..., 3]
    n = 3 * size[0] * size[1] if dview is None else view_extent(dview)
    for off in offsets:
        for fill in fills:
            prefill = np.full(n, fill, np.uint8)
            if dview is None:                                          # the contiguous block takes the SOURCE's byte order
                inner = np.ascontiguousarray(pic[..., ::-1] if bgr else pic).reshape(-1)
            else:
                inner = expected_dest(prefill, dview, pic, alpha)
            for how in (dict(x=x, ids=ids), dict(matte=matte)):
                out, host, base = op_composite(lib, mem, src, (off + 1) & 3, dview, prefill, off, bg, **how)
                want = host.copy()
                want[base:base + n] = inner
                assert np.array_equal(out, want), (what, "map" if "matte" in how else "fused", off, fill, int((out != want).sum()), np.flatnonzero(out != want)[:8] - base)
