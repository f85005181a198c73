"""Cases, expected values and scenarios shared by tests/test_surface_host.py (CPU, no library), tests/test_emu_surface.py (CPU, through the emulator)
and tests/test_gpu_surface.py (device memory): surfaces -- a rectangle of an NV12 / NV21 / I420 / P010 / YUY2 / UYVY frame read in the frame's first
launch and, for the overlay, in its last, and the picture written into a rectangle of a 4:2:0 one (include/tdnet.h "surfaces").

The oracles are dataloader.surface_to_rgb_u8 and dataloader.write_surface (pinned by hand in test_surface_host.py), followed by what the uint8 entries
already define on contiguous RGB bytes (ingest_u8_cases.expected_image; dataloader.overlay_u8 for the overlay).  Every comparison is exact.

`mem` stands for the memory a scenario runs in, as in view_cases.py."""
import ctypes
import functools

import numpy as np

import opcheck

import dst_view_cases as dvc
import ingest_u8_cases as u8cases
import view_cases as vc
from tdnet_amd import _capi
from tdnet_amd.dataloader import (SURF_DST, SURF_I420, SURF_NV12, SURF_NV21, SURF_P010, SURF_UYVY, SURF_YUY2, SourceView, Surface, nearest_index, overlay_u8,
                                  surface_extent, surface_from_samples, surface_sample_index, surface_to_rgb_u8, view_to_rgb_u8, write_surface)
from tdnet_amd.engine import surface_struct

LAYOUTS = (SURF_NV12, SURF_NV21, SURF_I420, SURF_P010, SURF_YUY2, SURF_UYVY)
NAMES = {SURF_NV12: "nv12", SURF_NV21: "nv21", SURF_I420: "i420", SURF_P010: "p010", SURF_YUY2: "yuy2", SURF_UYVY: "uyvy"}
FRAME, NET = (51, 91), (33, 65)                                        # the frame is odd
# (name, rectangle (y, x, h, w), network size): every chroma phase, the no-resize branch, the frame's corner, the last pixel
RECTS = [("phase_2_4", (2, 4, 41, 83), NET), ("phase_2_5", (2, 5, 41, 83), NET), ("phase_3_4", (3, 4, 41, 83), NET), ("phase_3_7", (3, 7, 41, 83), NET),
         ("same", (3, 7, 33, 65), NET), ("corner", (10, 8, 41, 83), NET), ("last_pixel", (50, 90, 1, 1), (1, 1))]
# wider than one workgroup's strip (256 lanes x 4 columns), one per sample width: device only
WIDE_FRAME, WIDE_RECT, WIDE_NET = (9, 2200), (1, 3, 8, 2100), (8, 2051)
WIDE_LAYOUTS = (SURF_I420, SURF_P010)
WIDE_DST = (SURF_P010, (8, 2100))
double3 = u8cases.double3


def variants(layout):
    """The memory forms a layout is tested in: tight; padded (luma pitch != chroma pitch != row bytes, a gap between the planes); I420 also with the V
    plane in front of the U plane (YV12)."""
    return ("tight", "padded") + (("v_first",) if layout == SURF_I420 else ())


def surface(layout, rect=None, variant="tight", frame=FRAME, standard=0):
    Hf, Wf = frame
    t = Surface(layout, Hf, Wf, crop=rect, standard=standard)
    if variant == "tight":                                             # interleaved chroma at an odd width: the one pitch both planes share is the chroma row's
        one = max(t.luma_row_bytes, t.chroma_row_bytes) if layout in (SURF_NV12, SURF_NV21, SURF_P010) else 0
        return Surface(layout, Hf, Wf, pitch=0 if one == t.luma_row_bytes else one, crop=rect, standard=standard)
    pitch = t.luma_row_bytes + 13
    if t.packed422:
        return Surface(layout, Hf, Wf, pitch=pitch, crop=rect, standard=standard)
    cpitch = t.chroma_row_bytes + 7
    u = (Hf + 3) * pitch + 5                                           # three rows and five bytes of gap: the chroma planes start at an odd address
    plane = ((Hf + 1) // 2) * cpitch
    if layout != SURF_I420:
        return Surface(layout, Hf, Wf, pitch=pitch, chroma_pitch=cpitch, crop=rect, standard=standard, u_offset=u)
    if variant == "v_first":
        return Surface(layout, Hf, Wf, pitch=pitch, chroma_pitch=cpitch, crop=rect, standard=standard, u_offset=u + plane + 11, v_offset=u)
    return Surface(layout, Hf, Wf, pitch=pitch, chroma_pitch=cpitch, crop=rect, standard=standard, u_offset=u, v_offset=u + plane + 11)


@functools.lru_cache(maxsize=None)
def samples(layout, Hf, Wf, seed=0):
    """Random samples (Y, U, V) of a whole frame: bytes, or 10-bit values for P010."""
    t = Surface(layout, Hf, Wf)
    rng = np.random.default_rng(Hf * 30011 + Wf * 7 + layout * 101 + seed)
    top = 1024 if t.wide else 256
    out = rng.integers(0, top, (Hf, Wf)), rng.integers(0, top, t.chroma_size), rng.integers(0, top, t.chroma_size)
    for a in out:
        a.setflags(write=False)
    return out


def covering(surf):
    """bool [extent]: the bytes of the samples that cover the rectangle (both bytes of a P010 word)."""
    y, x, h, w = surf.rect
    li, ui, vi = surface_sample_index(surf)
    cs = 0 if surf.packed422 else 1
    rows, cols = slice(y >> cs, ((y + h - 1) >> cs) + 1), slice(x >> 1, ((x + w - 1) >> 1) + 1)
    m = np.zeros(surface_extent(surf), bool)
    for idx in (li[y:y + h, x:x + w], ui[rows, cols], vi[rows, cols]):
        m[idx] = True
        if surf.wide:
            m[idx + 1] = True
    return m


def surface_bytes(surf, fill=0, seed=0, poison=False):
    """The surface's bytes [0, extent) of samples(seed); padding and plane gaps hold `fill`.  poison: EVERY byte that is not a sample covering the
    rectangle holds `fill`, and the low 6 bits of the covering P010 words are random (another draw per fill)."""
    Y, U, V = samples(surf.layout, surf.height, surf.width, seed)
    lows = None
    if surf.wide and poison:
        rng = np.random.default_rng(fill + 1)
        lows = [rng.integers(0, 64, a.shape) for a in (Y, U, V)]
    b = surface_from_samples(Y, U, V, surf, fill, lows)
    if poison:
        b[~covering(surf)] = fill
    return b


def expected_image(surf, H, W, seed=0, mean=None, std=None):
    """The fp32 NCHW tensor the frame must be: the host loader's image of the oracle's RGB bytes of the rectangle."""
    return u8cases.expected_image(surface_to_rgb_u8(surface_bytes(surf, 0, seed), surf), H, W, mean, std)


def csurf(surf):
    """(keepalive, pointer) for the test library's entries."""
    t = surface_struct(surf)
    return t, ctypes.byref(t)


def stem_image_surface(lib, mem, addr, surf, H, W, rows, mean=None, std=None):
    n = vc.stem_buffer_size(lib, H, W, rows)
    out = mem.out((n,), np.float32, 1234.5)
    t, pt = csurf(surf)
    assert lib.check(lib.tdnet_op_stem_image_surface(addr, pt, H, W, double3(mean), double3(std), rows, mem.addr(out), n, mem.stream)) == n
    return mem.get(out).view(np.uint32)


def run_stem_case(lib, mem, surf, net, offsets=(0, 1, 3), fills=(0x00, 0xFF)):
    """One surface against the fp32 route fed the oracle's image: both layouts of the stem image, the base at `offsets` into a holder of 0xA5 that must
    come back unchanged, and every byte that is not a covering sample filled with each of `fills` (P010: the low bits random) -- the same output."""
    H, W = net
    want = {rows: vc.stem_image_ref(lib, mem, H, W, rows, expected_image(surf, H, W)) for rows in (1, 0)}
    for fill in fills:
        s = surface_bytes(surf, fill, 0, poison=True)
        assert s.size == surface_extent(surf)
        for off in offsets:
            holder, addr = mem.up(s, off)
            for rows in (1, 0):
                got = stem_image_surface(lib, mem, addr, surf, H, W, rows)
                assert np.array_equal(got, want[rows]), (surf, (H, W), rows, off, fill, int((got != want[rows]).sum()))
            h = mem.get(holder)
            assert (h[:off] == 0xA5).all() and (h[off + s.size:] == 0xA5).all() and np.array_equal(h[off:off + s.size], s), (surf, off)


# ---- overlay over a surface ---------------------------------------------------------------------------------------------------------------
OVERLAY_RECTS = ((2, 5, 41, 83), (3, 4, 41, 83))


def op_overlay_surface(lib, mem, surf, src_bytes, src_off, out_off, pal, x=None, labels_u8=None):
    """tdnet_op_overlay_surface: the picture `out_off` bytes into a holder of 0xEE whose other bytes must survive; the frame `src_off` bytes into a
    holder of 0xA5.
    The logits go in between guard bands, once per band fill (opcheck.each_poison): the same bytes both times."""
    if x is None:
        return _op_overlay_surface(lib, mem, surf, src_bytes, src_off, out_off, pal, x, labels_u8, None)
    return opcheck.each_poison(x, mem.stream is not None, lambda px: _op_overlay_surface(lib, mem, surf, src_bytes, src_off, out_off, pal, x, labels_u8, px))


def _op_overlay_surface(lib, mem, surf, src_bytes, src_off, out_off, pal, x, labels_u8, px):
    H, W = vc.OVERLAY_NET
    h, w = surf.size
    n = h * w * 3
    ks, ps = mem.up(src_bytes, src_off)
    holder = mem.out((n + 16,), np.uint8, 0xEE)
    pal = np.ascontiguousarray(pal)
    t, pt = csurf(surf)
    if x is not None:
        C, lh, lw = x.shape
        pl = None
    else:
        C = lh = lw = 0
        px = None
        kl, pl = mem.up(labels_u8, 3)
    lib.check(lib.tdnet_op_overlay_surface(px, C, lh, lw, H, W, pl, ps, pt, pal.ctypes.data, len(pal), mem.addr(holder) + out_off, mem.stream))
    host = mem.get(holder)
    assert (host[:out_off] == 0xEE).all() and (host[out_off + n:] == 0xEE).all(), (surf, out_off)
    return host[out_off:out_off + n].reshape(h, w, 3)


def run_overlay_case(lib, mem, surf, offsets=range(4)):
    """Fused and label-map forms over one surface at output offsets 0..3; the non-covering bytes poisoned two ways give the same picture."""
    pal = vc.overlay_palette()
    x, lab = dvc.fused_labels(lib, mem, vc.OVERLAY_C)
    l8 = vc.overlay_labels()
    for fill in (0x00, 0xFF):
        s = surface_bytes(surf, fill, 1, poison=True)
        rgb = surface_to_rgb_u8(s, surf)
        want_f, want_l = overlay_u8(rgb, lab, pal), overlay_u8(rgb, l8, pal)
        for off in offsets:
            got = op_overlay_surface(lib, mem, surf, s, (0, 1, 5, 15)[off], off, pal, x=x)
            assert np.array_equal(got, want_f), (surf, "fused", off, fill)
            got = op_overlay_surface(lib, mem, surf, s, (15, 5, 1, 0)[off], off, pal, labels_u8=l8)
            assert np.array_equal(got, want_l), (surf, "labels", off, fill)
    sampled = l8[nearest_index(NET[0], surf.size[0])][:, nearest_index(NET[1], surf.size[1])]
    assert np.array_equal(want_l[sampled == 23], rgb[sampled == 23]) and (sampled == 23).any()   # a label >= n_colours shows the source


# ---- picture out into a surface -----------------------------------------------------------------------------------------------------------
DST_FRAME = (60, 100)

def dst_rect(name, frame=DST_FRAME):
    """even_41x83: (2, 6, 41, 83).  corner_odd: an odd-sized rectangle whose last row and column are the frame's -- of a frame one smaller than DST_FRAME
    each way, so that the origin stays even."""
    if name == "even_41x83":
        return frame, (2, 6, 41, 83)
    Hf, Wf = frame[0] - 1, frame[1] - 1                                # 59 x 99
    return (Hf, Wf), (Hf - 41, Wf - 83, 41, 83)                        # (18, 16, 41, 83): ends at row 58, column 98


DST_CASES = ("even_41x83", "corner_odd")


def op_picture(lib, mem, dsurf, prefill, off, pal, x=None, labels_u8=None, src=None, size=None):
    """tdnet_op_picture_surface into a guarded copy of `prefill`; the whole buffer back.  src: (Surface or SourceView, bytes) of the overlay's source, or
    None: the colour map of `size`.  dsurf: a Surface, or a SourceView (a destination view behind a surface source).
    The logits go in between guard bands, once per band fill (opcheck.each_poison): the same bytes both times."""
    if x is None:
        return _op_picture(lib, mem, dsurf, prefill, off, pal, x, labels_u8, src, size, None)
    return opcheck.each_poison(x, mem.stream is not None, lambda px: _op_picture(lib, mem, dsurf, prefill, off, pal, x, labels_u8, src, size, px))


def _op_picture(lib, mem, dsurf, prefill, off, pal, x, labels_u8, src, size, px):
    H, W = NET
    host, base = dvc.guarded(prefill, off)
    kd, pd = mem.up(host)
    if isinstance(dsurf, Surface):
        (td, ptd), ptv = csurf(dsurf), None
    else:
        (td, ptv), ptd = vc.cview(dsurf), None
    pal = np.ascontiguousarray(pal)
    if x is not None:
        C, lh, lw = x.shape
        pl = None
    else:
        C = lh = lw = 0
        px = None
        kl, pl = mem.up(labels_u8, 3)
    ps = pss = psv = None
    oh, ow = size if src is None else (0, 0)
    if src is not None:
        ks, ps = mem.up(src[1], 1)
        if isinstance(src[0], Surface):
            ts, pss = csurf(src[0])
        else:
            ts, psv = vc.cview(src[0])
    lib.check(lib.tdnet_op_picture_surface(px, C, lh, lw, H, W, pl, pal.ctypes.data, len(pal), ps, pss, psv, oh, ow, pd + base, ptd, ptv, mem.stream))
    return mem.get(kd)[:host.size], host, base


def write_dst(prefill, dst, picture):
    return write_surface(prefill, dst, picture) if isinstance(dst, Surface) else dvc.write_view(prefill, dst, picture)


def check_picture(lib, mem, dsurf, picture, pal, x=None, labels_u8=None, src=None, size=None, offsets=(0, 1, 2, 3), what=""):
    """Both prefills at every base offset: the whole buffer (guards included) is the oracle's copy of the prefill: only the sample bytes of the rectangle
    change, the 0xEE / 0x00 around and between them stays."""
    n = surface_extent(dsurf) if isinstance(dsurf, Surface) else dvc.view_extent(dsurf)
    for off in offsets:
        for fill in (0xEE, 0x00):
            prefill = np.full(n, fill, np.uint8)
            out, host, base = op_picture(lib, mem, dsurf, prefill, off, pal, x, labels_u8, src, size)
            want = host.copy()
            want[base:base + n] = write_dst(prefill, dsurf, picture)
            assert np.array_equal(out, want), (what, dsurf, off, fill, int((out != want).sum()), np.flatnonzero(out != want)[:8] - base)


def overlay_source(kind, size):
    """(description, bytes, true r g b of the rectangle) of an overlay source with a rectangle of `size`: a surface at an odd origin, or one of
    dst_view_cases' views."""
    h, w = size
    if kind in NAMES.values():
        layout = [k for k, v in NAMES.items() if v == kind][0]
        surf = surface(layout, (3, 7, h, w), "padded", frame=(h + 10, w + 8), standard=1)
        b = surface_bytes(surf, 0x77, 2)
        return surf, b, surface_to_rgb_u8(b, surf)
    view, b = dvc.source(kind, size)
    return view, b, view_to_rgb_u8(b, view)


def run_dest_case(lib, mem, layout, variant, case, standard=0, sources=("p010", "i420", "bgra32_view"), offsets=(0, 1, 2, 3)):
    """One destination surface: the colour map and the overlay over `sources`, the fused kernel (C = 19) and the label-map kernel.  The palette has 12
    rows: labels >= 12 of the fused kernel and 23 of the label map are >= n_colours."""
    frame, rect = dst_rect(case)
    dsurf = surface(layout, rect, variant, frame=frame, standard=standard)
    size = dsurf.size
    pal4 = dvc.palette(12)
    pal3 = np.ascontiguousarray(pal4[:, :3])
    l8 = vc.overlay_labels()
    x, lab = dvc.fused_labels(lib, mem, 19)
    for name, how, labels in (("labels", dict(labels_u8=l8), l8), ("fused", dict(x=x), lab)):
        check_picture(lib, mem, dsurf, dvc.colour_map(labels, pal3, size), pal3, size=size, offsets=offsets, what=name + " colour map", **how)
        for kind in sources:
            desc, sbytes, rgb = overlay_source(kind, size)
            check_picture(lib, mem, dsurf, overlay_u8(rgb, labels, pal4), pal4, src=(desc, sbytes), offsets=offsets, what=name + " overlay over " + kind, **how)


def run_view_dest_behind_surface_source(lib, mem, offsets=(0, 3)):
    """The destination VIEWS of "destination views" behind a surface source: RGBA32, BGR24 and NV12 views, the overlay over a P010 and a YUY2 surface."""
    pal4 = dvc.palette(12)
    l8 = vc.overlay_labels()
    x, lab = dvc.fused_labels(lib, mem, 19)
    for dview in dvc.FRAME_DESTS:
        for kind in ("p010", "yuy2"):
            desc, sbytes, rgb = overlay_source(kind, dview.size)
            for name, how, labels in (("labels", dict(labels_u8=l8), l8), ("fused", dict(x=x), lab)):
                check_picture(lib, mem, dview, overlay_u8(rgb, labels, pal4), pal4, src=(desc, sbytes), offsets=offsets, what=name + " view behind " + kind, **how)


# ---- whole frames: one scenario for the emulator (numpy memory) and the device (torch memory) -------------------------------------------
SCENARIO_RECT = (3, 7, 41, 83)


def _equal_frames(mem, a, b, pa, pb, t, nc, H, W):
    return vc._equal_frames(mem, a, b, pa, pb, t, nc, H, W)


def run_surface_scenario(a, mem, layouts=LAYOUTS, frames_n=3):
    """`a`: a finalized td2-psp18 Engine at NET.  Per layout: handle A takes the oracle's RGB bytes after set_input_u8(41, 83), a shared handle B the
    WHOLE surface after set_input_surface; three frames with equal logit bits, cache entries, fifo_len and last_launch_count, B switched to
    set_input_view and back in the middle; then labels, rgb, score, conf, encode + propagate and the overlay once each."""
    (H, W), nc = NET, 19
    for layout in layouts:
        surf = surface(layout, SCENARIO_RECT, "padded", standard=1)
        h, w = surf.size
        a.reset()
        b = a.share()
        a.set_input_u8(h, w)
        before = b.memory_bytes()[1]
        b.set_input_surface(surf)
        assert b.memory_bytes()[1] > before                            # tdnet_memory_bytes grows with the tables
        grown = b.memory_bytes()[1]
        b.set_input_surface(surface(layout, SCENARIO_RECT, "padded", standard=1))   # idempotent
        assert b.memory_bytes()[1] == grown
        frames = [surface_bytes(surf, 0x5A, 10 + t) for t in range(frames_n)]
        rgbs = [surface_to_rgb_u8(s, surf) for s in frames]
        logits = []
        for t in range(frames_n):
            ka, pa = mem.up(rgbs[t])
            if t == 1:                                                 # B through set_input_view (the tight RGB24 view), then back to the surface
                b.set_input_view(SourceView(0, h, w))
                logits.append(_equal_frames(mem, a, b, pa, pa, t, nc, H, W))
                b.set_input_surface(surf)
                continue
            kb, pb = mem.up(frames[t], (1, 0, 3)[t % 3])               # odd base addresses too
            logits.append(_equal_frames(mem, a, b, pa, pb, t, nc, H, W))
        assert not np.array_equal(logits[0], logits[2])
        c, d = a.share(), a.share()
        c.set_input_u8(h, w)
        d.set_input_surface(surf)
        (k1, pr), (k2, ps) = mem.up(rgbs[0]), mem.up(frames[0], 1)
        la, lb = mem.out((H, W), np.uint8, 0xEE), mem.out((H, W), np.uint8, 0xEE)
        c.forward_u8_labels(pr, 0, mem.addr(la), mem.stream); d.forward_u8_labels(ps, 0, mem.addr(lb), mem.stream)
        assert np.array_equal(mem.get(la), mem.get(lb)) and c.last_launch_count() == d.last_launch_count()
        lab = mem.get(lb).copy()
        pal3 = np.arange(19 * 3, dtype=np.uint8).reshape(19, 3)
        oh, ow = H // 4, W // 4
        ra, rb = mem.out((oh, ow, 3), np.uint8, 0xEE), mem.out((oh, ow, 3), np.uint8, 0xEE)
        for e in (c, d):
            e.set_output_rgb(oh, ow, pal3)
        c.forward_u8_rgb(pr, 1, mem.addr(ra), mem.stream); d.forward_u8_rgb(ps, 1, mem.addr(rb), mem.stream)
        assert np.array_equal(mem.get(ra), mem.get(rb))
        gt = np.random.default_rng(3).integers(0, 19, (H, W), dtype=np.uint8)
        kg, pg = mem.up(gt)
        for e in (c, d):
            e.set_score(None)
        c.forward_u8_score(pr, 0, pg, mem.addr(la), mem.stream); d.forward_u8_score(ps, 0, pg, mem.addr(lb), mem.stream)
        assert np.array_equal(mem.get(la), mem.get(lb))
        cm_c, cm_d = c.score_read(mem.stream), d.score_read(mem.stream)
        assert np.array_equal(cm_c, cm_d) and int(cm_c.sum()) == H * W
        ca, cb = mem.out((H, W), np.uint8, 0xEE), mem.out((H, W), np.uint8, 0xEE)
        c.forward_u8_labels_conf(pr, 1, mem.addr(la), mem.addr(ca), mem.stream); d.forward_u8_labels_conf(ps, 1, mem.addr(lb), mem.addr(cb), mem.stream)
        assert np.array_equal(mem.get(la), mem.get(lb)) and np.array_equal(mem.get(ca), mem.get(cb))
        c.encode_u8(pr, 0, mem.stream); d.encode_u8(ps, 0, mem.stream)
        c.propagate_labels_u8(mem.addr(la), mem.stream); d.propagate_labels_u8(mem.addr(lb), mem.stream)
        assert np.array_equal(mem.get(la), mem.get(lb)) and c.fifo_len() == d.fifo_len()
        pal = vc.overlay_palette()
        for e in (c, d):
            e.set_output_overlay(pal)
        va, vb = mem.out((h, w, 3), np.uint8, 0xEE), mem.out((h, w, 3), np.uint8, 0xEE)
        c.forward_u8_overlay(pr, 1, mem.addr(va), mem.stream); d.forward_u8_overlay(ps, 1, mem.addr(vb), mem.stream)
        assert np.array_equal(mem.get(va), mem.get(vb)) and c.last_launch_count() == d.last_launch_count()
        c.encode_u8(pr, 0, mem.stream); d.encode_u8(ps, 0, mem.stream)
        c.propagate_overlay(pr, mem.addr(va), mem.stream); d.propagate_overlay(ps, mem.addr(vb), mem.stream)
        assert np.array_equal(mem.get(va), mem.get(vb)) and c.fifo_len() == d.fifo_len()
        kl, pl = mem.up(lab)
        d.labels_overlay(pl, ps, mem.addr(vb), mem.stream)
        assert np.array_equal(mem.get(vb), overlay_u8(rgbs[0], lab, pal))
        # an overlay whose out overlaps the SURFACE's extent but none of the rectangle's samples fails without enqueueing
        n_before, fifo = d.last_launch_count(), d.fifo_len()
        try:
            d.forward_u8_overlay(ps, 0, ps + 1, mem.stream)
            raise AssertionError("an overlapping out was accepted")
        except _capi.TdnetError as err:
            assert "overlaps" in str(err)
        assert d.fifo_len() == fifo and d.last_launch_count() == n_before
        for e in (b, c, d):
            e.close()


def run_output_scenario(a, mem, dst_layouts=SURF_DST, src_layout=SURF_P010):
    """Twin handles fed the same surface frames: A writes the contiguous picture, B (a destination surface in force) into a prefilled surface that must
    equal write_surface of A's picture -- for the picture entries, with equal launch counts and FIFO lengths; set_output_view and set_output_surface
    replace each other, and NULL to either restores A's bytes."""
    (H, W), nc = NET, 19
    src = surface(src_layout, SCENARIO_RECT, "padded", standard=1)
    h, w = src.size
    frames = [surface_bytes(src, 0x5A, 30 + t) for t in range(2)]
    pal4 = vc.overlay_palette()
    s = mem.stream
    for layout in dst_layouts:
        dsurf = surface(layout, (2, 6, h, w), "padded", frame=DST_FRAME, standard=1)
        n = surface_extent(dsurf)
        prefill = np.full(n, 0xA5, np.uint8)
        a.reset()
        b = a.share()
        for e in (a, b):
            e.set_input_surface(src)
            e.set_output_overlay(pal4)
            e.set_output_rgb(h, w, dvc.PAL3)
        before = b.memory_bytes()[1]
        b.set_output_view(dvc.dest_view(0, rect=(2, 6, h, w)))          # a view first: the surface replaces it
        b.set_output_surface(dsurf)
        b.set_output_surface(surface(layout, (2, 6, h, w), "padded", frame=DST_FRAME, standard=1))   # idempotent
        assert b.memory_bytes()[1] == before                           # nothing is allocated
        pa = mem.out((h, w, 3), np.uint8, 0xEE)
        srcs = [mem.up(f, t + 1) for t, f in enumerate(frames)]

        def both(t, call_a, call_b, what):
            host, base = dvc.guarded(prefill, t % 4)
            kd, pd = mem.up(host)
            call_a(mem.addr(pa))
            call_b(pd + base)
            want = host.copy()
            want[base:base + n] = write_surface(prefill, dsurf, mem.get(pa).copy())
            got = mem.get(kd)[:host.size]
            assert np.array_equal(got, want), (what, dsurf, int((got != want).sum()))
            assert a.fifo_len() == b.fifo_len() and a.last_launch_count() == b.last_launch_count() > 0, what

        both(0, lambda p: a.forward_u8_rgb(srcs[0][1], 0, p, s), lambda p: b.forward_u8_rgb(srcs[0][1], 0, p, s), "forward_u8_rgb")
        both(1, lambda p: a.forward_u8_overlay(srcs[1][1], 1, p, s), lambda p: b.forward_u8_overlay(srcs[1][1], 1, p, s), "forward_u8_overlay")
        for e in (a, b):
            e.encode_u8(srcs[0][1], 0, s)
        both(3, lambda p: a.propagate_overlay(srcs[0][1], p, s), lambda p: b.propagate_overlay(srcs[0][1], p, s), "propagate_overlay")
        # a size mismatch is the frame entry's to report, nothing enqueued
        b.set_output_surface(surface(layout, (2, 6, h - 1, w), "padded", frame=DST_FRAME))
        fifo, launches = b.fifo_len(), b.last_launch_count()
        kd, pd = mem.up(prefill)
        try:
            b.forward_u8_overlay(srcs[0][1], 1, pd, s)
            raise AssertionError("a picture of another size than the rectangle was accepted")
        except _capi.TdnetError as err:
            assert "41 x 83" in str(err) and "40 x 83" in str(err), str(err)
        assert b.fifo_len() == fifo and b.last_launch_count() == launches
        # the view replaces the surface; NULL to the OTHER call restores the contiguous block
        b.set_output_surface(dsurf)
        b.set_output_view(None)
        a.reset(); b.reset()
        pb = mem.out((h, w, 3), np.uint8, 0x11)
        a.forward_u8_overlay(srcs[0][1], 0, mem.addr(pa), s); b.forward_u8_overlay(srcs[0][1], 0, mem.addr(pb), s)
        assert np.array_equal(mem.get(pa), mem.get(pb))
        b.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def bad_surfaces(output=False):
    """[(match, TdnetSurface, mean, std)]: one case per failure include/tdnet.h lists for tdnet_set_input_surface (output: tdnet_set_output_surface)."""
    Hf, Wf = FRAME if not output else DST_FRAME
    rect = SCENARIO_RECT if not output else (2, 6, 41, 83)
    out = []

    def sf(match, layout=SURF_I420, mean=None, std=None, **kw):
        args = dict(height=Hf, width=Wf, crop=rect)
        args.update(kw)
        out.append((match, surface_struct(Surface(layout, **args)), mean, std))

    def raw(match, base=SURF_I420, **fields):
        t = surface_struct(Surface(base, Hf, Wf, crop=rect))
        for k, v in fields.items():
            if k == "reserved":
                t.reserved[v[0]] = v[1]
            else:
                setattr(t, k, v)
        out.append((match, t, None, None))

    raw("layout", layout=6)
    raw("layout", layout=-1)
    sf("height", height=0, crop=None)
    sf("width", width=0, crop=None)
    raw("crop_height", crop_height=0)
    raw("crop_width", crop_width=-3)
    sf("crop_y", crop=(Hf - 40, rect[1], 41, 83))
    sf("crop_x", crop=(rect[0], Wf - 82, 41, 83))
    sf("crop_x", crop=(rect[0], 2 ** 31 - 1, 41, 83))
    sf("negative", crop=(-2, rect[1], 41, 83))
    sf("negative", crop=(rect[0], -6, 41, 83))
    sf("pitch", pitch=Wf - 1)
    sf("pitch", layout=SURF_P010, pitch=2 * Wf - 1)
    sf("pitch", pitch=-8)
    sf("chroma_pitch", chroma_pitch=(Wf + 1) // 2 - 1)
    sf("chroma_pitch", layout=SURF_NV21, chroma_pitch=2 * ((Wf + 1) // 2) - 1)
    sf("chroma_pitch", layout=SURF_P010, pitch=2 * Wf, chroma_pitch=4 * ((Wf + 1) // 2) - 1)
    sf("chroma_pitch", chroma_pitch=-4)
    raw("reserved", reserved=(0, 1))
    raw("reserved", reserved=(3, -1))
    sf("standard", standard=4)
    sf("standard", standard=-1)
    sf("u_offset", u_offset=Hf * Wf - 1)                               # inside the luma plane
    sf("v_offset", v_offset=Wf * 3)                                    # the V plane inside the luma plane
    sf("overlap", u_offset=Hf * Wf, v_offset=Hf * Wf + 10)             # U and V planes overlap
    sf("overlap", u_offset=Hf * Wf + 10, v_offset=Hf * Wf)             # ... in the other order
    cw = (Wf + 1) // 2
    sf("v_offset", layout=SURF_NV12, pitch=2 * cw, v_offset=Hf * Wf * 2)   # one chroma plane: must be 0
    sf("v_offset", layout=SURF_P010, pitch=4 * cw, v_offset=Hf * Wf * 4)
    sf("extent", u_offset=2 ** 31)
    sf("extent", u_offset=2 ** 31 - 100)
    sf("extent", height=40000, pitch=60000, crop=(0, 0, 41, 83))
    if not output:
        sf("chroma_pitch", layout=SURF_NV12)                               # an odd width, tight: the chroma_pitch 0 resolves to is below a chroma row
        sf("chroma_pitch", layout=SURF_YUY2, chroma_pitch=4 * ((Wf + 1) // 2))   # 4:2:2: must be 0
        sf("u_offset", layout=SURF_UYVY, u_offset=4096)
        sf("v_offset", layout=SURF_YUY2, v_offset=4096)
        sf("std", std=(0.2, 0.0, 0.2))
        sf("std", std=(0.2, float("nan"), 0.2))
        sf("mean", mean=(0.2, float("inf"), 0.2))
        sf("downscale", layout=SURF_P010, height=2, width=16000, crop=None)   # two bytes per staged column: 16000 columns behind 65 are beyond one strip's LDS
    else:
        sf("YUY2", layout=SURF_YUY2)
        sf("UYVY", layout=SURF_UYVY)
        sf("crop_y", crop=(3, 6, 41, 83))
        sf("crop_x", crop=(2, 7, 41, 83))
    return out


def run_error_cases(e, mem, config, frame_ptr, ref_bits, H, W):
    """Every bad surface fails naming tdnet_set_input_surface and the field, and leaves `config` (already in force on `e`) serving `frame_ptr` with the
    bits `ref_bits`."""
    out = mem.out((1, 19, H, W), np.float32, 3e7)
    for match, t, mean, std in bad_surfaces():
        fifo = e.fifo_len()
        rc = e.lib.tdnet_set_input_surface(e.h, ctypes.byref(t), double3(mean), double3(std))
        msg = e.lib.tdnet_last_error().decode()
        assert rc < 0 and "tdnet_set_input_surface" in msg and match in msg, (match, msg)
        assert e.fifo_len() == fifo, match
    e.reset()
    e.forward_u8(frame_ptr, 0, mem.addr(out), mem.stream)
    assert np.array_equal(mem.get(out).view(np.uint32), ref_bits) and e.fifo_len() == 1, config
    rc = e.lib.tdnet_set_input_surface(e.h, None, None, None)
    assert rc < 0 and "tdnet_set_input_surface" in e.lib.tdnet_last_error().decode() and "NULL" in e.lib.tdnet_last_error().decode()


def run_output_error_cases(e, mem, frame_ptr, dsurf, H, W):
    """`e`: an Engine with a surface input, the overlay and the destination surface `dsurf` in force.  Every bad surface fails naming
    tdnet_set_output_surface and the field and leaves the destination, the FIFO and a pending encoded frame alone."""
    n = surface_extent(dsurf)
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
    for match, t, _, _ in bad_surfaces(output=True):
        rc = e.lib.tdnet_set_output_surface(e.h, ctypes.byref(t))
        msg = e.lib.tdnet_last_error().decode()
        assert rc < 0 and "tdnet_set_output_surface" in msg and match in msg, (match, msg)
        assert e.fifo_len() == 0, match
    e.propagate(mem.addr(out), s)                                      # ... is still pending, and is this frame
    assert np.array_equal(mem.get(out).view(np.uint32), ref_bits) and e.fifo_len() == 1
    kd2, pd2 = mem.up(np.full(n, 0xA5, np.uint8))
    e.reset()
    e.forward_u8_overlay(frame_ptr, 0, pd2, s)                         # the destination in force is still dsurf
    assert np.array_equal(mem.get(kd2), ref_dst)
    # overlap: the destination SURFACE's extent against the source's
    e.reset()
    launches = e.last_launch_count()
    for call in (lambda: e.forward_u8_overlay(frame_ptr, 1, frame_ptr + 8, s), lambda: e.forward_u8_overlay(frame_ptr, 1, frame_ptr - n + 1, s)):
        try:
            call()
            raise AssertionError("an overlapping destination was accepted")
        except _capi.TdnetError as err:
            assert "overlaps" in str(err), str(err)
        assert e.fifo_len() == 0 and e.last_launch_count() == launches
    rc = e.lib.tdnet_set_output_surface(None, None)
    assert rc < 0 and "tdnet_set_output_surface" in e.lib.tdnet_last_error().decode()
