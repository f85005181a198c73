"""Cases, expected values and scenarios shared by tests/test_emu_dst_view.py (CPU, through the emulator) and tests/test_gpu_dst_view.py (device
memory): destination views -- the colour map or the overlay written by a frame's last launch into a rectangle of a pitched RGB / BGR / RGBA / BGRA
frame or of an NV12 surface (include/tdnet.h "destination views").

The oracle is dataloader.write_view -- and under it dataloader.nv12_from_rgb_u8, pinned by hand in tests/test_dst_view_host.py -- applied to the
picture the entries that predate the feature define (the labels of tdnet_op_upsample_argmax through the palette; dataloader.overlay_u8 over
dataloader.view_to_rgb_u8 of the source).  Every comparison is exact, and over the WHOLE destination buffer with 64 guard bytes on each side.

`mem` stands for the memory a scenario runs in, as in view_cases.py: mem.up(array, off=0) -> (holder, address); mem.out(shape, dtype, fill);
mem.addr(buffer); mem.get(buffer) -> numpy (synchronises); mem.stream."""
import ctypes

import numpy as np

import opcheck

import ingest_u8_cases as u8cases
import view_cases as vc
from tdnet_amd import _capi
from tdnet_amd.dataloader import (PIX_BGR, PIX_BGR24, PIX_BGRA32, PIX_NV12, PIX_RGB24, PIX_RGBA32, SourceView, nearest_index, overlay_u8, view_extent,
                                  view_to_rgb_u8, write_view)
from tdnet_amd.engine import view_struct

NET, LOW = (33, 65), (5, 9)
FRAME, RECT = (50, 96), (2, 6, 41, 83)                                 # even origin, odd h and w
GUARD, GUARD_BYTE = 64, 0x3C
FILLS = (0xA5, 0x00)
BPP = vc.BPP
# (tag, format, NV12 layout, standard)
DESTS = [(vc.NAMES[f], f, None, 0) for f in vc.PACKED] + [("nv12_%s_std%d" % (lay, std), PIX_NV12, li, std) for li, lay in enumerate(("tight", "padded"))
                                                           for std in range(4)]
DEST_IDS = [d[0] for d in DESTS]
# the overlay's sources: RGB24 whole and tight, a BGRA32 view, an NV12 view at an odd origin -- b g r and r g b pictures behind every destination order
SOURCES = ("rgb24_whole", "bgra32_view", "nv12_view")
# (frame, rectangle): widths 1, 2, 3, 5, heights 1 and 2, a rectangle ending at the frame's odd last row / column and one ending inside, and one wider
# than a workgroup's strip of 256 lanes x 4 pixels
EDGES = [((51, 97), r) for r in ((0, 0, 1, 1), (2, 4, 1, 2), (2, 4, 2, 3), (4, 8, 5, 5), (48, 94, 2, 3), (46, 92, 5, 5), (50, 96, 1, 1), (0, 2, 2, 1))] + \
        [((4, 2060), (0, 2, 3, 2051))]
EDGE_IDS = ["%dx%d_at_%d_%d" % (r[2], r[3], r[0], r[1]) for _, r in EDGES]
EDGE_FORMATS = (PIX_RGB24, PIX_BGRA32, PIX_NV12)


def dest_view(fmt, layout=None, standard=0, frame=FRAME, rect=RECT):
    """Packed: pitch = the row's bytes + 5 (odd: the rows start at every alignment).  NV12: vc.nv12_layouts -- tight, or padded pitch + a plane gap."""
    Hf, Wf = frame
    if fmt == PIX_NV12:
        _, pitch, uv = vc.nv12_layouts(Hf, Wf)[layout or 0]
        return SourceView(PIX_NV12, Hf, Wf, pitch=pitch, crop=rect, standard=standard, uv_offset=uv)
    return SourceView(fmt, Hf, Wf, pitch=Wf * BPP[fmt] + 5, crop=rect)


def palette(n=19):
    """n rows r, g, b, a of vc.overlay_palette: alphas 0, 255 and mid among the first 12 already."""
    return np.ascontiguousarray(vc.overlay_palette()[:n])


def source(kind, size, seed=1):
    """(view, the frame's bytes) of one of SOURCES with a rectangle of `size`."""
    h, w = size
    if kind == "rgb24_whole":
        view = SourceView(PIX_RGB24, h, w)
        return view, vc.packed_bytes(view, 0, seed)
    if kind == "bgra32_view":
        view = vc.packed_view(PIX_BGRA32, (3, 7, h, w), frame=(h + 9, w + 7))
        return view, vc.packed_bytes(view, 0x77, seed)
    view = vc.nv12_view((3, 7, h, w), 1, frame=(h + 10, w + 8))
    return view, vc.nv12_bytes(view, 0x77, seed)


def sampled(labels, size):
    return np.asarray(labels)[nearest_index(NET[0], size[0])][:, nearest_index(NET[1], size[1])]


def colour_map(labels, pal3, size):
    """decode_segmap of the sampled labels: true r, g, b [h, w, 3]; a label >= n_colours is grey (l, l, l)."""
    l = sampled(labels, size).astype(np.int64)
    table = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    table[:len(pal3)] = pal3
    return table[l]


def overlay(labels, pal4, src_view, src_bytes):
    """The overlay as true r, g, b whatever the source's order."""
    return overlay_u8(view_to_rgb_u8(src_bytes, src_view), labels, pal4)


def guarded(prefill, off):
    """The destination frame's bytes `off` bytes behind GUARD guard bytes, GUARD more behind them: (host array, offset of the base)."""
    g = np.full(GUARD + off + prefill.size + GUARD, GUARD_BYTE, np.uint8)
    g[GUARD + off:GUARD + off + prefill.size] = prefill
    return g, GUARD + off


def op_picture(lib, mem, dview, prefill, off, pal, x=None, labels_u8=None, src=None, size=None):
    """tdnet_op_picture_view into a guarded copy of `prefill`; the whole buffer back.  src: (view, bytes) of the overlay's source, or None: the colour
    map of `size`.  x: logits [C, h, w] (the fused kernel) or labels_u8 [H, W] (the label-map kernel).
    The logits go in between guard bands, once per band fill (opcheck.each_poison): the same bytes both times."""
    if x is None:
        return _op_picture(lib, mem, dview, prefill, off, pal, x, labels_u8, src, size, None)
    return opcheck.each_poison(x, mem.stream is not None, lambda px: _op_picture(lib, mem, dview, prefill, off, pal, x, labels_u8, src, size, px))


def _op_picture(lib, mem, dview, prefill, off, pal, x, labels_u8, src, size, px):
    H, W = NET
    host, base = guarded(prefill, off)
    kd, pd = mem.up(host)
    td, ptd = vc.cview(dview)
    pal = np.ascontiguousarray(pal)
    if x is not None:
        C, lh, lw = x.shape
        pl = None
    else:
        C = lh = lw = 0
        px = None
        kl, pl = mem.up(labels_u8, 3)
    if src is not None:
        ks, ps = mem.up(src[1], 1)
        ts, pts = vc.cview(src[0])
        oh = ow = 0
    else:
        ps, pts = None, None
        oh, ow = size
    lib.check(lib.tdnet_op_picture_view(px, C, lh, lw, H, W, pl, pal.ctypes.data, len(pal), ps, pts, oh, ow, pd + base, ptd, mem.stream))
    return mem.get(kd)[:host.size], host, base


def check_picture(lib, mem, dview, picture, pal, x=None, labels_u8=None, src=None, size=None, offsets=range(4), what=""):
    """Both prefills at every base offset: the whole buffer (guards included) is write_view of the prefill, and the two fills agree inside the rectangle."""
    n = view_extent(dview)
    inside = write_view(np.zeros(n, np.uint8), dview, picture) == write_view(np.full(n, 255, np.uint8), dview, picture)   # the bytes the picture decides
    for off in offsets:
        got = {}
        for fill in FILLS:
            prefill = np.full(n, fill, np.uint8)
            out, host, base = op_picture(lib, mem, dview, prefill, off, pal, x, labels_u8, src, size)
            want = host.copy()
            want[base:base + n] = write_view(prefill, dview, picture)
            assert np.array_equal(out, want), (what, dview, off, fill, int((out != want).sum()), np.flatnonzero(out != want)[:8] - base)
            got[fill] = out[base:base + n]
        assert np.array_equal(got[FILLS[0]][inside], got[FILLS[1]][inside]), (what, dview, off)


_LABELS = {}


def fused_labels(lib, mem, C):
    """(logits, their labels through the label kernel that predates the feature), computed once per memory kind."""
    key = (type(mem).__name__, C)
    if key not in _LABELS:
        x = u8cases.lowres_logits("odd_w", C, *LOW)
        lab = vc.fused_labels(lib, mem, x) if C > 1 else np.zeros(NET, np.int32)
        if C == 1:
            assert not vc.fused_labels(lib, mem, x).any()
        lab.setflags(write=False)
        _LABELS[key] = (x, lab)
    return _LABELS[key]


def run_dest_case(lib, mem, fmt, layout, standard):
    """One destination form: colour map and the overlay over every source, the fused kernel with C = 1 and 19 and the label-map kernel, base offsets
    0..3, two prefills.  The palette has 12 rows: labels 12..18 of the fused kernel and 23 of the label map are >= n_colours."""
    dview = dest_view(fmt, layout, standard)
    size = dview.size
    pal4 = palette(12)
    pal3 = np.ascontiguousarray(pal4[:, :3])
    l8 = vc.overlay_labels()
    runs = [("labels", dict(labels_u8=l8), l8)]
    for C in (1, 19):
        x, lab = fused_labels(lib, mem, C)
        runs.append(("fused C=%d" % C, dict(x=x), lab))
    assert (sampled(runs[2][2], size) >= 12).any() and (sampled(l8, size) == 23).any()
    for name, how, lab in runs:
        check_picture(lib, mem, dview, colour_map(lab, pal3, size), pal3, size=size, what=name + " colour map", **how)
        for kind in SOURCES:
            sview, sbytes = source(kind, size)
            check_picture(lib, mem, dview, overlay(lab, pal4, sview, sbytes), pal4, src=(sview, sbytes), what=name + " overlay over " + kind, **how)


def run_edge_case(lib, mem, frame, rect):
    """An edge rectangle in a 3-byte, a 4-byte and both NV12 destinations: the colour map and the overlay over a tight RGB source, both kernels."""
    size = rect[2:]
    pal4 = palette(12)
    pal3 = np.ascontiguousarray(pal4[:, :3])
    l8 = vc.overlay_labels()
    x, lab = fused_labels(lib, mem, 19)
    sview, sbytes = source("rgb24_whole", size)
    for fmt in EDGE_FORMATS:
        for layout in ((0, 1) if fmt == PIX_NV12 else (None,)):
            dview = dest_view(fmt, layout, 1, frame, rect)
            for name, how, labels in (("labels", dict(labels_u8=l8), l8), ("fused", dict(x=x), lab)):
                check_picture(lib, mem, dview, colour_map(labels, pal3, size), pal3, size=size, offsets=(0, 1), what=name + " colour map", **how)
                check_picture(lib, mem, dview, overlay(labels, pal4, sview, sbytes), pal4, src=(sview, sbytes), offsets=(0, 3), what=name + " overlay", **how)


# ---- whole frames: one scenario for the emulator (numpy memory) and the device (torch memory) -------------------------------------------
SRC_VIEW = vc.packed_view(PIX_BGRA32, (3, 7, 41, 83))                  # the frames' byte input: a b g r source, picture 41 x 83
FRAME_DESTS = [dest_view(PIX_RGBA32), dest_view(PIX_BGR24), dest_view(PIX_NV12, 1, 1)]
PAL3 = np.arange(19 * 3, dtype=np.uint8).reshape(19, 3) * 4 + 3


def true_rgb(block, bgr):
    return np.ascontiguousarray(block[..., ::-1]) if bgr else block


def run_frame_scenario(a, mem, dests=None):
    """`a`: a finalized td2-psp18 Engine at NET.  Twin handles fed the same frames: A writes the contiguous picture, B (a destination view in force)
    into a prefilled destination frame that must equal write_view of A's picture -- for every picture entry, with equal launch counts and FIFO lengths;
    set_output_view(None) restores A's bytes."""
    (H, W), nc = NET, 19
    h, w = SRC_VIEW.size
    frames = [vc.view_bytes(SRC_VIEW, 0x5A, 30 + t) for t in range(4)]
    img32 = [vc.expected_image(SRC_VIEW, H, W, 30 + t) for t in range(2)]
    pal4 = vc.overlay_palette()
    l8 = vc.overlay_labels()
    kl, plab = mem.up(l8, 1)
    for dview in dests or FRAME_DESTS:
        n = view_extent(dview)
        prefill = np.full(n, 0xA5, np.uint8)
        a.reset()
        b = a.share()
        for e in (a, b):
            e.set_input_view(SRC_VIEW)
            e.set_output_overlay(pal4)
            e.set_output_rgb(h, w, PAL3)
        before = b.memory_bytes()[1]
        b.set_output_view(dview)
        b.set_output_view(SourceView(dview.format, dview.height, dview.width, dview.pitch, dview.crop, dview.standard, dview.uv_offset))   # idempotent
        assert b.memory_bytes()[1] == before                           # nothing is allocated: the view travels as kernel arguments
        pa = mem.out((h, w, 3), np.uint8, 0xEE)
        srcs = [mem.up(f, t % 4) for t, f in enumerate(frames)]
        imgs = [mem.up(i) for i in img32]

        def both(t, call_a, call_b, bgr, what):
            host, base = guarded(prefill, t % 4)
            kd, pd = mem.up(host)
            call_a(mem.addr(pa))
            call_b(pd + base)
            want = host.copy()
            want[base:base + n] = write_view(prefill, dview, true_rgb(mem.get(pa).copy(), bgr))
            got = mem.get(kd)[:host.size]
            assert np.array_equal(got, want), (what, dview, int((got != want).sum()))
            assert a.fifo_len() == b.fifo_len(), what
            return got

        s = mem.stream
        both(0, lambda p: a.forward_u8_rgb(srcs[0][1], 0, p, s), lambda p: b.forward_u8_rgb(srcs[0][1], 0, p, s), False, "forward_u8_rgb")
        assert a.last_launch_count() == b.last_launch_count() > 0
        both(1, lambda p: a.forward_u8_overlay(srcs[1][1], 1, p, s), lambda p: b.forward_u8_overlay(srcs[1][1], 1, p, s), True, "forward_u8_overlay")
        assert a.last_launch_count() == b.last_launch_count() > 0
        both(2, lambda p: a.forward_rgb(imgs[0][1], 0, p, s), lambda p: b.forward_rgb(imgs[0][1], 0, p, s), False, "forward_rgb")
        assert a.last_launch_count() == b.last_launch_count() > 0
        for e in (a, b):
            e.encode_u8(srcs[2][1], 1, s)
        both(3, lambda p: a.propagate_rgb(p, s), lambda p: b.propagate_rgb(p, s), False, "propagate_rgb")
        assert a.last_launch_count() == b.last_launch_count() > 0
        for e in (a, b):
            e.encode_u8(srcs[3][1], 0, s)
        both(0, lambda p: a.propagate_overlay(srcs[3][1], p, s), lambda p: b.propagate_overlay(srcs[3][1], p, s), True, "propagate_overlay")
        assert a.last_launch_count() == b.last_launch_count() > 0
        both(1, lambda p: a.labels_rgb(plab, p, s), lambda p: b.labels_rgb(plab, p, s), False, "labels_rgb")
        got = both(2, lambda p: a.labels_overlay(plab, srcs[0][1], p, s), lambda p: b.labels_overlay(plab, srcs[0][1], p, s), True, "labels_overlay")
        want_rgb = overlay_u8(view_to_rgb_u8(frames[0], SRC_VIEW), l8, pal4)
        host, base = guarded(prefill, 2)
        assert np.array_equal(got[base:base + n], write_view(prefill, dview, want_rgb))   # against the host oracle too, not only the twin
        # the label, logit, score and confidence entries are unaffected
        la, lb = mem.out((H, W), np.uint8, 0xEE), mem.out((H, W), np.uint8, 0xEE)
        a.forward_u8_labels(srcs[1][1], 0, mem.addr(la), s); b.forward_u8_labels(srcs[1][1], 0, mem.addr(lb), s)
        assert np.array_equal(mem.get(la), mem.get(lb))
        # back to the contiguous form: today's bytes exactly
        b.set_output_view(None)
        a.reset(); b.reset()
        pb = mem.out((h, w, 3), np.uint8, 0x11)
        a.forward_u8_overlay(srcs[0][1], 0, mem.addr(pa), s); b.forward_u8_overlay(srcs[0][1], 0, mem.addr(pb), s)
        assert np.array_equal(mem.get(pa), mem.get(pb))
        a.forward_u8_rgb(srcs[1][1], 1, mem.addr(pa), s); b.forward_u8_rgb(srcs[1][1], 1, mem.addr(pb), s)
        assert np.array_equal(mem.get(pa), mem.get(pb))
        b.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def bad_dst_views():
    """[(match, TdnetView)]: one case per failure include/tdnet.h lists for tdnet_set_output_view."""
    Hf, Wf = FRAME
    ok = dict(height=Hf, width=Wf, pitch=Wf * 4 + 5, crop=RECT)
    out = []

    def sv(match, fmt=PIX_BGRA32, **kw):
        args = dict(ok)
        args.update(kw)
        out.append((match, view_struct(SourceView(fmt, **args))))

    def raw(match, **fields):
        t = view_struct(SourceView(PIX_BGRA32, **ok))
        for k, v in fields.items():
            if k == "reserved":
                t.reserved[v[0]] = v[1]
            else:
                setattr(t, k, v)
        out.append((match, t))

    raw("format", format=5)
    raw("format", format=-1)
    sv("height", height=0, crop=None, pitch=0)
    sv("width", width=0, crop=None, pitch=0)
    raw("crop_height", crop_height=0)
    raw("crop_width", crop_width=-3)
    sv("crop_y", crop=(10, 6, 41, 83))                                 # 10 + 41 > 50
    sv("crop_x", crop=(2, 14, 41, 83))                                 # 14 + 83 > 96
    sv("crop_x", crop=(2, 2 ** 31 - 1, 41, 83))
    sv("negative", crop=(-2, 6, 41, 83))
    sv("negative", crop=(2, -6, 41, 83))
    sv("pitch", pitch=Wf * 4 - 1)
    sv("pitch", fmt=PIX_RGB24, pitch=Wf * 3 - 1)
    sv("pitch", pitch=-8)
    raw("reserved", reserved=(0, 1))
    raw("reserved", reserved=(4, -1))
    raw("standard", standard=1)
    raw("uv_offset", uv_offset=4096)
    sv("pitch", fmt=PIX_NV12, pitch=95)                                # the NV12 conditions of tdnet_set_input_nv12
    sv("uv_offset", fmt=PIX_NV12, pitch=96, uv_offset=50 * 96 - 1)
    sv("standard", fmt=PIX_NV12, pitch=96, standard=4)
    sv("extent", fmt=PIX_NV12, pitch=96, uv_offset=2 ** 31)
    sv("extent", height=40000, pitch=60000)
    sv("crop_y", fmt=PIX_NV12, pitch=96, crop=(3, 6, 41, 83))          # an odd NV12 origin
    sv("crop_x", fmt=PIX_NV12, pitch=96, crop=(2, 7, 41, 83))
    return out


def run_error_cases(e, mem, frame_ptr, H, W):
    """`e`: an Engine with SRC_VIEW, the overlay, the colour map 41 x 83 and the destination view FRAME_DESTS[0] in force.  Every bad view fails naming
    tdnet_set_output_view and the field and leaves the configuration, the FIFO and a pending encoded frame alone: the same logit bits and the same
    destination bytes afterwards.  Size mismatch and overlap are the frame entries' to report, with nothing enqueued."""
    dview = FRAME_DESTS[0]
    n = view_extent(dview)
    s = mem.stream
    out = mem.out((1, 19, H, W), np.float32, 3e7)
    e.reset()
    e.forward_u8(frame_ptr, 0, mem.addr(out), s)
    ref_bits = mem.get(out).view(np.uint32).copy()
    kd, pd = mem.up(np.full(n, 0xA5, np.uint8))
    e.reset()
    e.forward_u8_overlay(frame_ptr, 0, pd, s)
    ref_dst = mem.get(kd).copy()
    e.reset()
    e.encode_u8(frame_ptr, 0, s)                                       # a pending encoded frame
    for match, t in bad_dst_views():
        rc = e.lib.tdnet_set_output_view(e.h, ctypes.byref(t))
        msg = e.lib.tdnet_last_error().decode()
        assert rc < 0 and "tdnet_set_output_view" in msg and match in msg, (match, msg)
        assert e.fifo_len() == 0, match
    e.propagate(mem.addr(out), s)                                      # ... is still pending, and is this frame
    assert np.array_equal(mem.get(out).view(np.uint32), ref_bits) and e.fifo_len() == 1
    kd2, pd2 = mem.up(np.full(n, 0xA5, np.uint8))
    e.reset()
    e.forward_u8_overlay(frame_ptr, 0, pd2, s)                         # the view in force is still FRAME_DESTS[0]
    assert np.array_equal(mem.get(kd2), ref_dst)
    # size mismatch: the frame entries', both sizes named, nothing enqueued, a pending frame stays pending
    e.reset()
    e.set_output_view(dest_view(PIX_RGBA32, rect=(2, 6, 40, 83)))
    e.encode_u8(frame_ptr, 0, s)
    launches = e.last_launch_count()
    calls = [lambda: e.forward_u8_overlay(frame_ptr, 1, pd, s), lambda: e.forward_u8_rgb(frame_ptr, 1, pd, s), lambda: e.propagate_rgb(pd, s),
             lambda: e.propagate_overlay(frame_ptr, pd, s), lambda: e.labels_rgb(frame_ptr, pd, s), lambda: e.labels_overlay(frame_ptr, frame_ptr, pd, s)]
    for call in calls:
        try:
            call()
            raise AssertionError("a picture of another size than the rectangle was accepted")
        except _capi.TdnetError as err:
            assert "41 x 83" in str(err) and "40 x 83" in str(err), str(err)
        assert e.fifo_len() == 0 and e.last_launch_count() == launches
    e.propagate(mem.addr(out), s)
    assert np.array_equal(mem.get(out).view(np.uint32), ref_bits)
    # overlap: the destination FRAME's extent against the source frame's, although the rectangles' bytes do not meet
    e.set_output_view(dview)
    e.reset()
    e.encode_u8(frame_ptr, 0, s)
    launches = e.last_launch_count()
    for call in (lambda: e.forward_u8_overlay(frame_ptr, 1, frame_ptr + view_extent(SRC_VIEW) - 1, s), lambda: e.forward_u8_overlay(frame_ptr, 1, frame_ptr - n + 1, s),
                 lambda: e.propagate_overlay(frame_ptr, frame_ptr - n + 1, s), lambda: e.labels_overlay(frame_ptr, frame_ptr, frame_ptr + 8, s)):
        try:
            call()
            raise AssertionError("an overlapping destination was accepted")
        except _capi.TdnetError as err:
            assert "overlaps" in str(err), str(err)
        assert e.fifo_len() == 0 and e.last_launch_count() == launches
    e.propagate(mem.addr(out), s)
    assert np.array_equal(mem.get(out).view(np.uint32), ref_bits)
    rc = e.lib.tdnet_set_output_view(None, None)
    assert rc < 0 and "tdnet_set_output_view" in e.lib.tdnet_last_error().decode()
