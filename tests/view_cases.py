"""Cases, expected values and scenarios shared by tests/test_view_host.py (CPU, no library), tests/test_emu_view.py (CPU, through the emulator)
and tests/test_gpu_view.py (device memory): source views -- a rectangle of a pitched RGB / BGR / RGBA / BGRA / NV12 frame read in the frame's first
launch and, for the overlay, in its last (include/tdnet.h "source views").

The oracle is dataloader.view_to_rgb_u8 (pinned by hand in test_view_host.py) followed by what the uint8 entries already define on contiguous RGB
bytes (ingest_u8_cases.expected_image, the library's own packed-RGB route; dataloader.overlay_u8 for the overlay).  Every comparison is exact.

`mem` stands for the memory a scenario runs in: mem.up(array, off=0) -> (holder, address) -- the array's bytes `off` bytes into a holder of 0xA5;
mem.out(shape, dtype, fill) -> buffer; mem.addr(buffer); mem.get(buffer) -> numpy (synchronises); mem.stream."""
import ctypes
import functools

import numpy as np

import opcheck

import ingest_u8_cases as u8cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import (PIX_BGR, PIX_BGR24, PIX_BGRA32, PIX_NV12, PIX_RGB24, PIX_RGBA32, SourceView, nearest_index, nv12_extent, overlay_u8, pack_view,
                                  view_extent, view_to_rgb_u8)
from tdnet_amd.engine import view_struct

PACKED = (PIX_RGB24, PIX_BGR24, PIX_RGBA32, PIX_BGRA32)
NAMES = {PIX_RGB24: "rgb24", PIX_BGR24: "bgr24", PIX_RGBA32: "rgba32", PIX_BGRA32: "bgra32", PIX_NV12: "nv12"}
BPP = {PIX_RGB24: 3, PIX_BGR24: 3, PIX_RGBA32: 4, PIX_BGRA32: 4}
FRAME = (50, 90)                                                       # the packed cases' frame; pitch 90 bpp + 5 (odd: every row alignment mod 16)
NV_FRAME = (51, 91)                                                    # the NV12 cases' frame (odd)
# (name, rectangle (y, x, h, w), [network sizes])
PACKED_CASES = [
    ("down", (3, 7, 41, 83), [(33, 65)]),
    ("same", (5, 11, 33, 65), [(33, 65)]),
    ("up", (1, 1, 20, 37), [(33, 65)]),
    ("corner", (9, 7, 41, 83), [(33, 65)]),                            # the frame's bottom-right corner: the last chunk is assembled byte-wise
    ("last_pixel", (49, 89, 1, 1), [(1, 1), (5, 9)]),
    ("one_column", (0, 40, 50, 1), [(9, 5)]),
]
NV12_CASES = [
    ("phase_2_4", (2, 4, 41, 83), (33, 65)), ("phase_2_5", (2, 5, 41, 83), (33, 65)), ("phase_3_4", (3, 4, 41, 83), (33, 65)),
    ("phase_3_7", (3, 7, 41, 83), (33, 65)),
    ("same", (3, 7, 33, 65), (33, 65)),
    ("corner", (10, 8, 41, 83), (33, 65)),                             # ends at the frame's last, odd column and row
    ("last_pixel", (50, 90, 1, 1), (1, 1)),
]
# wider than one workgroup's strip (256 lanes x 4 columns): device only (the emulator runs a workgroup's lanes one after the other)
WIDE_FRAME, WIDE_NET = (9, 2200), (8, 2051)
WIDE_PACKED = (PIX_RGBA32, (0, 3, 9, 2100))
WIDE_NV12 = (1, 3, 8, 2100)                                            # "the same geometry at origin (1, 3)": 8 rows are what the 9-row frame leaves below row 1
double3 = u8cases.double3


@functools.lru_cache(maxsize=None)
def frame_rgb(Hf, Wf, seed=0):
    """Random RGB bytes [Hf, Wf, 3] of a whole frame."""
    f = np.random.default_rng(Hf * 40009 + Wf * 11 + seed).integers(0, 256, (Hf, Wf, 3), dtype=np.uint8)
    f.setflags(write=False)
    return f


def packed_view(fmt, rect, frame=FRAME, tight=False):
    Hf, Wf = frame
    return SourceView(fmt, Hf, Wf, pitch=0 if tight else Wf * BPP[fmt] + 5, crop=rect)


def packed_bytes(view, fill=0, seed=0, outside=None):
    """The frame's bytes in the view's format; pitch padding and x bytes hold `fill`; outside: that byte in every pixel outside the rectangle."""
    f = frame_rgb(view.height, view.width, seed)
    if outside is not None:
        y, x, h, w = view.rect
        g = np.full_like(f, outside)
        g[y:y + h, x:x + w] = f[y:y + h, x:x + w]
        f = g
    return pack_view(f, view, fill)


def nv12_layouts(Hf, Wf):
    """[(tag, pitch, uv_offset)]: tight, and padded (pitch 96 -- the wide frame: the next multiple of 256 -- and three rows of plane gap)."""
    row = 2 * ((Wf + 1) // 2)
    padded = 96 if row <= 96 else (row + 255) // 256 * 256
    return [("tight", row, Hf * row), ("padded", padded, (Hf + 3) * padded)]


def nv12_view(rect, layout, frame=NV_FRAME, standard=0):
    Hf, Wf = frame
    _, pitch, uv = nv12_layouts(Hf, Wf)[layout]
    return SourceView(PIX_NV12, Hf, Wf, pitch=pitch, crop=rect, standard=standard, uv_offset=uv)


@functools.lru_cache(maxsize=None)
def nv12_planes(Hf, Wf, seed=0):
    rng = np.random.default_rng(Hf * 20011 + Wf + seed)
    Y = rng.integers(0, 256, (Hf, Wf), dtype=np.uint8)
    UV = rng.integers(0, 256, ((Hf + 1) // 2, (Wf + 1) // 2, 2), dtype=np.uint8)
    return Y, UV


def nv12_bytes(view, fill=0, seed=0, outside=None):
    """The surface's bytes [0, extent); padding and plane gap hold `fill`; outside: that byte in every Y sample outside the rectangle and every
    chroma pair that covers none of its pixels."""
    Hf, Wf, pitch, uv = view.height, view.width, view.row_pitch, view.uv
    Y, UV = nv12_planes(Hf, Wf, seed)
    if outside is not None:
        y, x, h, w = view.rect
        Y2, UV2 = np.full_like(Y, outside), np.full_like(UV, outside)
        Y2[y:y + h, x:x + w] = Y[y:y + h, x:x + w]
        UV2[y >> 1:((y + h - 1) >> 1) + 1, x >> 1:((x + w - 1) >> 1) + 1] = UV[y >> 1:((y + h - 1) >> 1) + 1, x >> 1:((x + w - 1) >> 1) + 1]
        Y, UV = Y2, UV2
    s = np.full(nv12_extent(Hf, Wf, pitch, uv), fill, np.uint8)
    for r in range(Hf):
        s[r * pitch:r * pitch + Wf] = Y[r]
    for j in range(UV.shape[0]):
        s[uv + j * pitch:uv + j * pitch + 2 * UV.shape[1]] = UV[j].reshape(-1)
    return s


def view_bytes(view, fill=0, seed=0, outside=None):
    return (nv12_bytes if view.nv12 else packed_bytes)(view, fill, seed, outside)


def expected_image(view, H, W, seed=0, mean=None, std=None):
    """The fp32 NCHW tensor the frame must be: the host loader's image of the oracle's RGB bytes of the rectangle."""
    return u8cases.expected_image(view_to_rgb_u8(view_bytes(view, 0, seed), view), H, W, mean, std)


def cview(view):
    """(keepalive, pointer) for the test library's entries."""
    t = view_struct(view)
    return t, ctypes.byref(t)


def stem_buffer_size(lib, H, W, rows):
    return lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))


def stem_image_ref(lib, mem, H, W, rows, img):
    """The complete stem image buffer (border included) of an fp32 NCHW image through the fp32 kernels, as raw 32-bit words."""
    n = stem_buffer_size(lib, H, W, rows)
    out = mem.out((n,), np.float32, 1234.5)
    k, p = mem.up(img)
    assert lib.check(lib.tdnet_op_stem_image(p, None, 0, 0, H, W, None, None, rows, mem.addr(out), n, mem.stream)) == n
    return mem.get(out).view(np.uint32)


def stem_image_view(lib, mem, addr, view, H, W, rows, mean=None, std=None):
    n = stem_buffer_size(lib, H, W, rows)
    out = mem.out((n,), np.float32, 1234.5)
    t, pt = cview(view)
    assert lib.check(lib.tdnet_op_stem_image_view(addr, pt, H, W, double3(mean), double3(std), rows, mem.addr(out), n, mem.stream)) == n
    return mem.get(out).view(np.uint32)


def run_stem_case(lib, mem, view, nets, offsets=(0, 1, 3), fills=(0x00, 0xFF)):
    """One view against the fp32 route fed the oracle's image: both layouts of the stem image, the base at `offsets` into a holder of 0xA5 that must
    come back unchanged, and padding / x bytes / everything outside the rectangle filled with each of `fills` -- the same output."""
    for H, W in nets:
        want = {rows: stem_image_ref(lib, mem, H, W, rows, expected_image(view, H, W)) for rows in (1, 0)}
        for fill in fills:
            s = view_bytes(view, fill, 0, outside=fill)
            assert s.size == view_extent(view)
            for off in offsets:
                holder, addr = mem.up(s, off)
                for rows in (1, 0):
                    got = stem_image_view(lib, mem, addr, view, H, W, rows)
                    assert np.array_equal(got, want[rows]), (view, (H, W), rows, off, fill, int((got != want[rows]).sum()))
                h = mem.get(holder)
                assert (h[:off] == 0xA5).all() and (h[off + s.size:] == 0xA5).all() and np.array_equal(h[off:off + s.size], s), (view, off)


# ---- overlay -------------------------------------------------------------------------------------------------------------------------------
OVERLAY_NET, OVERLAY_LOW, OVERLAY_C = (33, 65), (5, 9), 19
OVERLAY_PACKED = (PIX_RGB24, PIX_BGR24, PIX_BGRA32)
OVERLAY_RECT = (3, 7, 41, 83)
OVERLAY_NV12_ORIGINS = ((2, 5), (3, 4))


def overlay_palette():
    """19 colours with alphas 0, 128 and 255 (and others) among them; 19 rows, so a label >= 19 shows the source."""
    rng = np.random.default_rng(77)
    pal = rng.integers(0, 256, (19, 4), dtype=np.uint8)
    pal[:, 3] = [0, 128, 255, 127, 1, 254, 64, 0, 128, 255, 200, 33, 90, 7, 180, 128, 0, 255, 128]
    return pal


def overlay_labels():
    """uint8 labels [33, 65] with every class and label 23 (>= n_colours) in them."""
    l = np.random.default_rng(78).integers(0, 19, OVERLAY_NET, dtype=np.uint8)
    l[4:9, 10:30] = 23
    return l


def expected_overlay(view, src_bytes, labels, pal):
    want = overlay_u8(view_to_rgb_u8(src_bytes, view), labels, pal)
    return want[..., ::-1] if view.format in PIX_BGR else want         # the picture is in the source's colour order


def op_overlay_view(lib, mem, view, src_bytes, src_off, out_off, pal, x=None, labels_u8=None):
    """tdnet_op_overlay_view: the picture `out_off` bytes into a holder of 0xEE whose other bytes must survive; the frame `src_off` bytes into a
    holder of 0xA5.  x: logits [C, h, w] (the fused kernel) or labels_u8 [H, W] (the label-map kernel).
    The logits go in between guard bands, once per band fill (opcheck.each_poison): the same bytes both times."""
    if x is None:
        return _op_overlay_view(lib, mem, view, src_bytes, src_off, out_off, pal, x, labels_u8, None)
    return opcheck.each_poison(x, mem.stream is not None, lambda px: _op_overlay_view(lib, mem, view, src_bytes, src_off, out_off, pal, x, labels_u8, px))


def _op_overlay_view(lib, mem, view, src_bytes, src_off, out_off, pal, x, labels_u8, px):
    H, W = OVERLAY_NET
    h, w = view.size
    n = h * w * 3
    ks, ps = mem.up(src_bytes, src_off)
    holder = mem.out((n + 16,), np.uint8, 0xEE)
    pal = np.ascontiguousarray(pal)
    t, pt = cview(view)
    if x is not None:
        C, lh, lw = x.shape
        pl = None
    else:
        C = lh = lw = 0
        px = None
        kl, pl = mem.up(labels_u8, 3)
    lib.check(lib.tdnet_op_overlay_view(px, C, lh, lw, H, W, pl, ps, pt, pal.ctypes.data, len(pal), mem.addr(holder) + out_off, mem.stream))
    host = mem.get(holder)
    assert (host[:out_off] == 0xEE).all() and (host[out_off + n:] == 0xEE).all(), (view, out_off)
    return host[out_off:out_off + n].reshape(h, w, 3)


def fused_labels(lib, mem, x):
    """int32 labels of the logits through the label kernel that predates the feature."""
    C, h, w = x.shape
    H, W = OVERLAY_NET
    kx, px = mem.up(x)
    out = mem.out((H * W,), np.int32, -1)
    lib.check(lib.tdnet_op_upsample_argmax(px, C, h, w, H, W, mem.addr(out), None, mem.stream))
    return mem.get(out).reshape(H, W)


def run_overlay_case(lib, mem, view):
    """Fused and label-map forms of one view at every output offset 0..3; the bytes outside the rectangle poisoned two ways give the same picture."""
    pal = overlay_palette()
    x = u8cases.lowres_logits("odd_w", OVERLAY_C, *OVERLAY_LOW)
    lab = fused_labels(lib, mem, x)
    l8 = overlay_labels()
    for fill in (0x00, 0xFF):
        s = view_bytes(view, fill, 1, outside=fill)
        want_f, want_l = expected_overlay(view, s, lab, pal), expected_overlay(view, s, l8, pal)
        for off in range(4):
            got = op_overlay_view(lib, mem, view, s, (0, 1, 5, 15)[off], off, pal, x=x)
            assert np.array_equal(got, want_f), (view, "fused", off, fill)
            got = op_overlay_view(lib, mem, view, s, (15, 5, 1, 0)[off], off, pal, labels_u8=l8)
            assert np.array_equal(got, want_l), (view, "labels", off, fill)
    sampled = l8[nearest_index(OVERLAY_NET[0], view.size[0])][:, nearest_index(OVERLAY_NET[1], view.size[1])]
    rgb = view_to_rgb_u8(s, view)
    src_order = rgb[..., ::-1] if view.format in PIX_BGR else rgb
    assert np.array_equal(want_l[sampled == 23], src_order[sampled == 23]) and (sampled == 23).any()   # a label >= n_colours shows the source


# ---- whole frames: one scenario for the emulator (numpy memory) and the device (torch memory) -------------------------------------------
FRAME_NET = (33, 65)
SCENARIO_RECT = (3, 7, 41, 83)


def scenario_views():
    """The two views the scenario runs: BGRA32 50 x 90, pitched; NV12 51 x 91 padded, both with the rectangle at (3, 7)."""
    return [packed_view(PIX_BGRA32, SCENARIO_RECT), nv12_view(SCENARIO_RECT, 1)]


def _equal_frames(mem, a, b, pa, pb, t, nc, H, W):
    """One frame on both handles: equal logit bits, cache entries, FIFO length and launch count."""
    lk, dk, dv = a.cache_dims()
    oa, ob = mem.out((1, nc, H, W), np.float32, 7e7), mem.out((1, nc, H, W), np.float32, -7e7)
    a.forward_u8(pa, t % 2, mem.addr(oa), mem.stream)
    b.forward_u8(pb, t % 2, mem.addr(ob), mem.stream)
    ga, gb = mem.get(oa), mem.get(ob)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), t
    assert a.last_launch_count() == b.last_launch_count() > 0, t
    for st, shp in (("cache_q", (lk, dk)), ("cache_k", (lk, dk)), ("cache_v", (lk, dv))):
        assert np.array_equal(a.stage(st, shp).view(np.uint32), b.stage(st, shp).view(np.uint32)), (t, st)
    assert a.fifo_len() == b.fifo_len()
    return ga


def run_view_scenario(a, mem):
    """`a`: a finalized td2-psp18 Engine at FRAME_NET.  Per view: handle A takes the oracle's RGB bytes after set_input_u8(41, 83), a shared handle B
    the WHOLE frame after set_input_view; five frames with equal logit bits, cache entries, fifo_len and last_launch_count, B switched to
    set_input_u8, then set_input_nv12, then back in the middle; then every other byte entry once against its counterpart."""
    (H, W), nc = FRAME_NET, 19
    for view in scenario_views():
        h, w = view.size
        a.reset()
        b = a.share()
        a.set_input_u8(h, w)
        before = b.memory_bytes()[1]
        b.set_input_view(view)
        assert b.memory_bytes()[1] > before                            # tdnet_memory_bytes grows with the tables
        grown = b.memory_bytes()[1]
        b.set_input_view(SourceView(view.format, view.height, view.width, view.pitch, view.crop, view.standard, view.uv_offset))   # idempotent
        assert b.memory_bytes()[1] == grown
        frames = [view_bytes(view, 0x5A, 10 + t) for t in range(5)]
        rgbs = [view_to_rgb_u8(s, view) for s in frames]
        logits = []
        for t in range(5):
            ka, pa = mem.up(rgbs[t])
            if t == 2:                                                 # B through the two siblings, then back to the view
                b.set_input_u8(h, w)
                logits.append(_equal_frames(mem, a, b, pa, pa, t, nc, H, W))
                nvv = nv12_view((0, 0, 0, 0), 0, frame=(h, w))
                b.set_input_nv12(h, w, nvv.row_pitch)
                b.set_input_view(view)
                continue
            kb, pb = mem.up(frames[t], t % 4)                          # base addresses 0..3 bytes into a buffer
            logits.append(_equal_frames(mem, a, b, pa, pb, t, nc, H, W))
        assert not np.array_equal(logits[0], logits[1])
        # the other byte entries, once each: C on the oracle's bytes, D on the frame
        c, d = a.share(), a.share()
        c.set_input_u8(h, w)
        d.set_input_view(view)
        (k1, pr), (k2, ps) = mem.up(rgbs[0]), mem.up(frames[0], 1)
        la, lb = mem.out((H, W), np.uint8, 0xEE), mem.out((H, W), np.uint8, 0xEE)
        c.forward_u8_labels(pr, 0, mem.addr(la), mem.stream); d.forward_u8_labels(ps, 0, mem.addr(lb), mem.stream)
        assert np.array_equal(mem.get(la), mem.get(lb)) and c.last_launch_count() == d.last_launch_count()
        pal3 = np.arange(19 * 3, dtype=np.uint8).reshape(19, 3)
        oh, ow = H // 4, W // 4
        ra, rb = mem.out((oh, ow, 3), np.uint8, 0xEE), mem.out((oh, ow, 3), np.uint8, 0xEE)
        for e in (c, d):
            e.set_output_rgb(oh, ow, pal3)
        c.forward_u8_rgb(pr, 1, mem.addr(ra), mem.stream); d.forward_u8_rgb(ps, 1, mem.addr(rb), mem.stream)
        assert np.array_equal(mem.get(ra), mem.get(rb))                # the colour map is untouched by the source's colour order
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
        # overlay: the fused entry, the split frame's and the label-map form; D's picture is in the source's colour order
        pal = overlay_palette()
        bgr = view.format in PIX_BGR
        for e in (c, d):
            e.set_output_overlay(pal)
        va, vb = mem.out((h, w, 3), np.uint8, 0xEE), mem.out((h, w, 3), np.uint8, 0xEE)
        c.forward_u8_overlay(pr, 1, mem.addr(va), mem.stream); d.forward_u8_overlay(ps, 1, mem.addr(vb), mem.stream)
        ga, gb = mem.get(va).copy(), mem.get(vb).copy()
        assert np.array_equal(ga[..., ::-1] if bgr else ga, gb) and c.last_launch_count() == d.last_launch_count()
        lab = mem.get(lb).copy()
        c.forward_u8_labels(pr, 0, mem.addr(la), mem.stream); d.forward_u8_labels(ps, 0, mem.addr(lb), mem.stream)
        lab = mem.get(lb).copy()
        c.encode_u8(pr, 1, mem.stream); d.encode_u8(ps, 1, mem.stream)
        c.propagate_overlay(pr, mem.addr(va), mem.stream); d.propagate_overlay(ps, mem.addr(vb), mem.stream)
        ga, gb = mem.get(va).copy(), mem.get(vb).copy()
        assert np.array_equal(ga[..., ::-1] if bgr else ga, gb) and c.fifo_len() == d.fifo_len()
        kl, pl = mem.up(lab)
        d.labels_overlay(pl, ps, mem.addr(vb), mem.stream)
        assert np.array_equal(mem.get(vb), expected_overlay(view, frames[0], lab, pal))
        # an overlay whose out overlaps the FRAME's extent but not the rectangle's pixels fails without enqueueing
        n_before, fifo = d.last_launch_count(), d.fifo_len()
        try:
            d.forward_u8_overlay(ps, 0, ps + 1, mem.stream)            # inside the frame's first row: above the rectangle (origin row 3)
            raise AssertionError("an overlapping out was accepted")
        except _capi.TdnetError as err:
            assert "overlaps" in str(err)
        assert d.fifo_len() == fifo and d.last_launch_count() == n_before
        for e in (b, c, d):
            e.close()


# ---- errors: (a word of the message, the view's constructor arguments or a raw TdnetView patch, mean, std) --------------------------------
def bad_views():
    """[(match, SourceView or patched TdnetView, kwargs)]: one case per failure include/tdnet.h lists for tdnet_set_input_view."""
    Hf, Wf = FRAME
    ok = dict(height=Hf, width=Wf, pitch=Wf * 4 + 5, crop=(3, 7, 41, 83))
    out = []

    def sv(match, fmt=PIX_BGRA32, mean=None, std=None, **kw):
        args = dict(ok)
        args.update(kw)
        out.append((match, view_struct(SourceView(fmt, **args)), mean, std))

    def raw(match, **fields):
        t = view_struct(SourceView(PIX_BGRA32, **ok))
        for k, v in fields.items():
            if k == "reserved":
                t.reserved[v[0]] = v[1]
            else:
                setattr(t, k, v)
        out.append((match, t, None, None))

    raw("format", format=5)
    raw("format", format=-1)
    sv("height", height=0, crop=None, pitch=0)
    sv("width", width=0, crop=None, pitch=0)
    raw("crop_height", crop_height=0)                                  # not all four zero: a rectangle below 1
    raw("crop_width", crop_width=-3)
    sv("crop_y", crop=(10, 7, 41, 83))                                 # 10 + 41 > 50
    sv("crop_x", crop=(3, 8, 41, 83))                                  # 8 + 83 > 90
    sv("crop_x", crop=(3, 2 ** 31 - 1, 41, 83))                        # the sum would overflow int32
    sv("crop_y", crop=(2 ** 31 - 40, 7, 41, 83))
    sv("negative", crop=(-1, 7, 41, 83))
    sv("negative", crop=(3, -7, 41, 83))
    sv("pitch", pitch=Wf * 4 - 1)
    sv("pitch", fmt=PIX_RGB24, pitch=Wf * 3 - 1)
    sv("pitch", pitch=-8)
    raw("reserved", reserved=(0, 1))
    raw("reserved", reserved=(4, -1))
    raw("standard", standard=1)
    raw("uv_offset", uv_offset=4096)
    sv("pitch", fmt=PIX_NV12, pitch=89)                                # the NV12 conditions of tdnet_set_input_nv12
    sv("uv_offset", fmt=PIX_NV12, pitch=96, uv_offset=50 * 96 - 1)
    sv("standard", fmt=PIX_NV12, pitch=96, standard=4)
    sv("extent", fmt=PIX_NV12, pitch=96, uv_offset=2 ** 31)
    sv("extent", height=40000, pitch=60000)
    sv("std", std=(0.2, 0.0, 0.2))
    sv("std", std=(0.2, float("nan"), 0.2))
    sv("mean", mean=(0.2, float("inf"), 0.2))
    sv("downscale", height=2, width=8000, pitch=0, crop=None)          # 32-bit pixels: 8000 columns behind 65 are beyond one strip's LDS (RGB24 still fits)
    return out


def run_error_cases(e, mem, config, frame_ptr, ref_bits, H, W):
    """Every bad view fails naming tdnet_set_input_view and the field, and leaves `config` (already in force on `e`) serving `frame_ptr` with the
    bits `ref_bits`."""
    out = mem.out((1, 19, H, W), np.float32, 3e7)
    for match, t, mean, std in bad_views():
        fifo = e.fifo_len()
        rc = e.lib.tdnet_set_input_view(e.h, ctypes.byref(t), double3(mean), double3(std))
        msg = e.lib.tdnet_last_error().decode()
        assert rc < 0 and "tdnet_set_input_view" in msg and match in msg, (match, msg)
        assert e.fifo_len() == fifo, match
        e.reset()
        e.forward_u8(frame_ptr, 0, mem.addr(out), mem.stream)
        assert np.array_equal(mem.get(out).view(np.uint32), ref_bits) and e.fifo_len() == 1, (config, match)
    rc = e.lib.tdnet_set_input_view(e.h, None, None, None)
    assert rc < 0 and "tdnet_set_input_view" in e.lib.tdnet_last_error().decode() and "NULL" in e.lib.tdnet_last_error().decode()
