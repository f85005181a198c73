"""Cases shared by tests/test_refine_host.py, tests/test_emu_refine.py (CPU, through the emulator) and tests/test_gpu_refine.py (device memory).

The refined matte (include/tdnet.h "refined matte") is defined in integers and single correctly rounded fp32 operations, so every comparison of the
kernels with the oracle dataloader.refine_matte_u8 is EXACT: the output bytes and the two coefficient planes.

Memory: every map goes into a holder of its own -- GUARD bytes of a band fill in front and behind, the map `off` bytes (0..3) behind the front band, its
rows `cols + pad` bytes apart with the padding filled with a byte of its own.  Neither fill may change the result, and after a call every byte of the
output's holder that is not a pixel's still holds what it held.  `mem` is the memory a scenario runs in: mem.up(uint8 array) -> (holder, address);
mem.get(holder) -> numpy (synchronises); mem.stream."""
import ctypes

import numpy as np

from tdnet_amd.dataloader import refine_matte_u8

GUARD = 64
FILLS = (0xA5, 0x00)                                                   # the bands around a map
PADS = (0x00, 0xFF)                                                    # the padding behind a map's rows
KINDS = ("random", "all255", "step", "const_matte", "ramp", "binary")
HOST_SIZES = ((1, 1), (1, 7), (7, 1), (5, 9), (33, 65), (41, 83), (70, 130))
RADII = (1, 4, 16)
EPSS = (4, 65, 65025)


def inputs(kind, h, w, seed=0):
    """(guide, matte) uint8 [h, w], read-only.  random: independent bytes; all255: the overflow witness of S_GG; step: a half-plane 0 / 255 step in both
    maps; const_matte: a constant matte over a random guide; ramp: a 16-pixel soft matte ramp over a 40-level guide edge with +-3 noise; binary: a
    binary matte over an 8-level guide edge (the largest slopes: a ~ 25 at eps = 4)."""
    g = np.random.default_rng(1000 * h + w + 7 * seed)
    x = np.broadcast_to(np.arange(w)[None, :], (h, w))
    right = x >= w // 2
    if kind == "random":
        G, M = g.integers(0, 256, (h, w)), g.integers(0, 256, (h, w))
    elif kind == "all255":
        G, M = np.full((h, w), 255), np.full((h, w), 255)
    elif kind == "step":
        G = M = np.where(right, 255, 0)
    elif kind == "const_matte":
        G, M = g.integers(0, 256, (h, w)), np.full((h, w), 37 + 50 * (seed % 4))
    elif kind == "ramp":
        G = 100 + 40 * right + g.integers(-3, 4, (h, w))
        M = np.clip(np.rint((x - (w // 2 - 8)) * (255.0 / 16.0)), 0, 255)
    elif kind == "binary":
        G, M = 100 + 8 * right, np.where(right, 255, 0)
    else:
        raise ValueError(kind)
    G, M = np.ascontiguousarray(G, dtype=np.uint8), np.ascontiguousarray(M, dtype=np.uint8)
    G.setflags(write=False)
    M.setflags(write=False)
    return G, M


def textbook_f64(G, M, r, eps):
    """(out int64 [h, w], max |a|) of He et al.'s guided filter in float64, the means over the same clipped windows: a = cov / (var + eps),
    b = mean_M - a mean_G, out = clamp8(rint(mean_a G + mean_b))."""
    from tdnet_amd.dataloader import _box_sum
    g = G.astype(np.float64)
    N = _box_sum(np.ones(G.shape, np.int64), r).astype(np.float64)
    box = lambda a: _box_sum(a, r) / N                                 # the integer sums are exact; one division
    mg, mm = box(G.astype(np.int64)), box(M.astype(np.int64))
    var = box(G.astype(np.int64) ** 2) - mg * mg
    cov = box(G.astype(np.int64) * M.astype(np.int64)) - mg * mm
    a = cov / (var + eps)
    b = mm - a * mg
    h, w = G.shape
    ys = [(max(0, y - r), min(h - 1, y + r) + 1) for y in range(h)]
    xs = [(max(0, x - r), min(w - 1, x + r) + 1) for x in range(w)]

    def fmean(v):                                                      # float64 means of float64 values over the clipped windows
        ii = np.zeros((h + 1, w + 1))
        ii[1:, 1:] = v.cumsum(0).cumsum(1)
        y0, y1 = np.array([p[0] for p in ys]), np.array([p[1] for p in ys])
        x0, x1 = np.array([p[0] for p in xs]), np.array([p[1] for p in xs])
        return (ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]) / N
    out = np.clip(np.rint(fmean(a) * g + fmean(b)), 0, 255).astype(np.int64)
    return out, float(np.abs(a).max())


# ---- the operator on any memory -------------------------------------------------------------------------------------------------------------
class Placed:
    """A byte map [h, w] inside its holder: host image, the offset of pixel (0, 0) and the pitch."""

    def __init__(self, a, off, pad, band, pad_fill):
        h, w = a.shape
        self.h, self.w, self.pitch, self.base = h, w, w + pad, GUARD + off
        self.host = np.full(GUARD + off + h * self.pitch + GUARD, band, np.uint8)
        body = self.host[self.base:self.base + h * self.pitch].reshape(h, self.pitch)
        body[:, w:] = pad_fill
        body[:, :w] = a

    def pixels(self, flat):
        return flat[self.base:self.base + self.h * self.pitch].reshape(self.h, self.pitch)[:, :self.w]

    def rest_unchanged(self, flat):
        """every byte that is not a pixel's still holds what the holder was made with"""
        keep = np.ones(self.host.size, bool)
        self.pixels(keep)[...] = False
        return bool((flat[:self.host.size][keep] == self.host[keep]).all())


def place(mem, a, off=0, pad=0, band=0xA5, pad_fill=0x00):
    p = Placed(np.asarray(a, np.uint8), off, pad, band, pad_fill)
    p.holder, addr = mem.up(p.host)
    p.addr = addr + p.base
    return p


def scratch(mem, eng, h, w):
    n = eng.refine_scratch_bytes(h, w)
    assert n == 6 * h * w
    return mem.up(np.full(n + 8, 0xEE, np.uint8))                      # mem.up's holders start at an aligned address


def refine_op(eng, mem, G, M, r, eps, offs=(0, 0, 0), pads=(0, 0, 0), band=0xA5, pad_fill=0x00, out_fill=0x5A):
    """One call of tdnet_refine_matte: the bytes written [h, w].  offs / pads: the byte offset and the row padding of guide, matte and output."""
    h, w = G.shape
    g, m = place(mem, G, offs[0], pads[0], band, pad_fill), place(mem, M, offs[1], pads[1], band, pad_fill)
    o = place(mem, np.full((h, w), out_fill, np.uint8), offs[2], pads[2], band, pad_fill)
    ks, ps = scratch(mem, eng, h, w)
    eng.refine_matte(g.addr, g.pitch, m.addr, m.pitch, o.addr, o.pitch, h, w, r, eps, ps, mem.stream)
    flat = np.asarray(mem.get(o.holder))
    assert o.rest_unchanged(flat), ("bytes around the output's pixels were written", G.shape, r, eps, offs, pads)
    for p in (g, m):
        assert np.array_equal(np.asarray(mem.get(p.holder))[:p.host.size], p.host), "an input was written"
    assert (np.asarray(mem.get(ks))[6 * h * w:6 * h * w + 8] == 0xEE).all(), "bytes behind the scratch were written"
    return o.pixels(flat).copy()


def coeff_op(lib, mem, G, M, r, eps, offs=(0, 0), pads=(0, 0), band=0xA5, pad_fill=0x00):
    """One call of tdnet_op_refine_coeff: (a_q int16 [h, w], b_q int32 [h, w])."""
    h, w = G.shape
    g, m = place(mem, G, offs[0], pads[0], band, pad_fill), place(mem, M, offs[1], pads[1], band, pad_fill)
    ka, pa = mem.up(np.full(2 * h * w + 8, 0xEE, np.uint8))
    kb, pb = mem.up(np.full(4 * h * w + 8, 0xEE, np.uint8))
    lib.check(lib.tdnet_op_refine_coeff(g.addr, g.pitch, m.addr, m.pitch, h, w, r, eps, pa, pb, mem.stream))
    fa, fb = np.asarray(mem.get(ka)), np.asarray(mem.get(kb))
    assert (fa[2 * h * w:2 * h * w + 8] == 0xEE).all() and (fb[4 * h * w:4 * h * w + 8] == 0xEE).all()
    return fa[:2 * h * w].copy().view(np.int16).reshape(h, w), fb[:4 * h * w].copy().view(np.int32).reshape(h, w)


_want = {}


def want(kind, h, w, r, eps, seed=0):
    """the oracle's (out, a_q, b_q) of a case, computed once, read-only"""
    key = (kind, h, w, r, eps, seed)
    if key not in _want:
        G, M = inputs(kind, h, w, seed)
        res = refine_matte_u8(G, M, r, eps, want_coeff=True)
        for a in res:
            a.setflags(write=False)
        _want[key] = (G, M) + res
    return _want[key]


def tile(lib):
    tx, cy, ay = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    lib.check(lib.tdnet_op_refine_tile(ctypes.byref(tx), ctypes.byref(cy), ctypes.byref(ay)))
    return tx.value, cy.value, ay.value


TILE = (64, 32, 16)                                                    # what tile() answers: the cases are sized from it, and a test holds it to the library


def exact_cases():
    """(kind, h, w, r, eps) of the operator tests: the smallest shapes at which the kernels can go wrong.
      * 1x1, 1x7, 7x1, 5x9 at r = 16: the window exceeds the map on both axes
      * one tile exactly and tile + 1 in each axis (the taller of the two launches' tiles, which is a multiple of the other), r = 1 and 16: halos across seams
      * a row wider than one workgroup's tile row (3 tiles and a bit), few rows
      * 41x83 and 17x29, the matte tests' source sizes; eps at both ends
      * all-255 and the half-plane step at r = 16: the overflow witnesses"""
    tx, cy, ay = TILE
    ty = max(cy, ay)
    assert ty % cy == 0 and ty % ay == 0
    out = [("random", h, w, 16, 65) for h, w in ((1, 1), (1, 7), (7, 1), (5, 9))]
    for r in (1, 16):
        out += [("random", ty, tx, r, 65), ("random", ty + 1, tx, r, 65), ("random", ty, tx + 1, r, 65), ("ramp", ty + 1, tx + 1, r, 65)]
    out += [("random", 5, 3 * tx + 9, 16, 65), ("binary", 3, 2 * tx + 1, 4, 4)]
    out += [("random", 41, 83, 4, 4), ("ramp", 41, 83, 16, 65025), ("random", 17, 29, 8, 65), ("binary", 17, 29, 2, 4)]
    out += [("all255", ty + 1, tx + 1, 16, 4), ("step", ty + 1, tx + 1, 16, 4), ("all255", 41, 83, 16, 65025)]
    return out


def case_id(c):
    return "%s-%dx%d-r%d-e%d" % c


def check_operator(lib, eng, mem, case, offsets=((0, 0, 0),), fills=FILLS):
    """The operator and the coefficient launch of one case against the oracle, at every (offsets, band fill, padding fill): exact."""
    kind, h, w, r, eps = case
    G, M, out, aq, bq = want(kind, h, w, r, eps)
    for i, offs in enumerate(offsets):
        for band, pad_fill in zip(fills, PADS):
            pads = (0, 0, 0) if i == 0 and band == fills[0] else ((i + 1) % 5, (i + 3) % 7, (i + 2) % 5)
            got = refine_op(eng, mem, G, M, r, eps, offs, pads, band, pad_fill)
            bad = got != out
            assert not bad.any(), (case, offs, pads, band, int(bad.sum()), tuple(int(v) for v in np.argwhere(bad)[0]), int(got[bad][0]), int(out[bad][0]))
    ga, gb = coeff_op(lib, mem, G, M, r, eps, offsets[-1][:2], (3, 1), fills[-1], PADS[-1])
    assert np.array_equal(ga, aq), (case, "a_q", int((ga != aq).sum()), tuple(int(v) for v in np.argwhere(ga != aq)[0]))
    assert np.array_equal(gb, bq), (case, "b_q", int((gb != bq).sum()), tuple(int(v) for v in np.argwhere(gb != bq)[0]))


ALL_OFFSETS = tuple((a, b, c) for a in range(4) for b in range(4) for c in range(4))
FEW_OFFSETS = ((0, 0, 0), (1, 2, 3), (3, 1, 2), (2, 3, 1))


def check_exact_properties(eng, mem, h, w):
    """Exact by construction: a constant matte comes back unchanged for any guide, r and eps; all-255 gives 255."""
    G, _ = inputs("random", h, w, 3)
    for c, r, eps in ((0, 1, 4), (37, 16, 65), (255, 7, 65025), (128, 16, 4)):
        got = refine_op(eng, mem, G, np.full((h, w), c, np.uint8), r, eps, (1, 0, 2), (2, 0, 1))
        assert (got == c).all(), (c, r, eps, np.unique(got))
    G, M = inputs("all255", h, w)
    for r, eps in ((16, 4), (1, 65025)):
        assert (refine_op(eng, mem, G, M, r, eps, (3, 3, 3), (1, 1, 1)) == 255).all(), (r, eps)


def refused(eng, mem):
    """[(call, message pattern)]: every refused argument of tdnet_refine_matte, and the holder of an output none of them may touch"""
    G, M = inputs("random", 5, 9)
    g, m = place(mem, G), place(mem, M)
    o = place(mem, np.full((5, 9), 0x5A, np.uint8))
    ks, ps = scratch(mem, eng, 5, 9)
    big, pbig = mem.up(np.zeros(5 * 9 * 8, np.uint8))

    def call(**kw):
        a = dict(guide=g.addr, gp=g.pitch, matte=m.addr, mp=m.pitch, out=o.addr, op=o.pitch, rows=5, cols=9, r=4, eps=65, scratch=ps)
        a.update(kw)
        return lambda: eng.refine_matte(a["guide"], a["gp"], a["matte"], a["mp"], a["out"], a["op"], a["rows"], a["cols"], a["r"], a["eps"], a["scratch"], mem.stream)
    cases = [(call(r=0), "radius = 0"), (call(r=17), "radius = 17"), (call(eps=3), "eps = 3"), (call(eps=65026), "eps = 65026"),
             (call(gp=8), "guide_pitch = 8"), (call(mp=8), "matte_pitch = 8"), (call(op=8), "out_pitch = 8"),
             (call(rows=0), "0 x 9"), (call(cols=0), "5 x 0"), (call(rows=65536), "65536 x 9"), (call(rows=40000, cols=40000), "40000 x 40000"),
             (call(guide=None), "null"), (call(matte=None), "null"), (call(out=None), "null"), (call(scratch=None), "null"),
             (call(scratch=ps + 2), "not 4-byte aligned"),
             (call(out=g.addr + 3), "out overlaps the guide"), (call(out=m.addr + 44), "out overlaps the matte"),
             (call(out=pbig + 6 * 45 - 1, scratch=pbig), "out overlaps the scratch"),
             (call(guide=pbig + 4, scratch=pbig, out=pbig + 6 * 45), "scratch overlaps the guide"),
             (call(matte=pbig + 6 * 45 - 1, scratch=pbig, out=pbig + 7 * 45), "scratch overlaps the matte")]
    return cases, (o, (g, m, ks, big))


# ---- the frame's end: gather, the refined entries, the composite through the refined matte --------------------------------------------------------
# `dev` is the memory the frames live in: dev.put(array) -> buffer; dev.ptr(buffer) -> what an Engine method takes; dev.get(buffer) -> numpy
# (synchronises); dev.stream.
H, W, HS, WS = 33, 65, 41, 83
MOVING = tuple(range(11, 19))
BG = (200, 30, 90)
FRAME_R, FRAME_EPS = 4, 65


def gather_op(lib, mem, src, x=None, ids=(), matte=None):
    """One call of tdnet_op_refine_gather on a source of matte_cases.comp_source: (luma, M_src) [Hs, Ws].  x: the ADDRESS of logits [19, 5, 9], or matte: a
    map [33, 65] (uploaded at an odd address)."""
    import matte_cases as mc
    import surface_cases as sc
    import view_cases as vc
    from tdnet_amd.dataloader import SourceView
    desc, sbytes, rgb = src[0], src[1], src[2]
    hs, ws = rgb.shape[:2]
    ks, ps = mem.up(sbytes, 1)
    kl, pl = mem.up(np.full(hs * ws + 8, 0xEE, np.uint8))
    km, pm = mem.up(np.full(hs * ws + 8, 0xEE, np.uint8))
    is_surf = not isinstance(desc, SourceView)
    keep, pts = sc.csurf(desc) if is_surf else vc.cview(desc)
    cls = mc.ids_array(ids)
    kk, pk = mem.up(matte, 1) if matte is not None else (None, None)
    lib.check(lib.tdnet_op_refine_gather(None if matte is not None else x, 19, 5, 9, 33, 65, cls.ctypes.data if len(ids) else None, len(ids), pk, ps,
                                         None if is_surf else pts, pts if is_surf else None, pl, pm, mem.stream))
    fl, fm = np.asarray(mem.get(kl)), np.asarray(mem.get(km))
    assert (fl[hs * ws:hs * ws + 8] == 0xEE).all() and (fm[hs * ws:hs * ws + 8] == 0xEE).all()
    return fl[:hs * ws].reshape(hs, ws).copy(), fm[:hs * ws].reshape(hs, ws).copy()


def check_gather(lib, mem, kind, size, px, ids, matte):
    """luma == luma_u8(the source as r g b) and M_src == matte[ys][:, xs], fused and from the map `matte` (the matte operator's bytes for the logits at px)"""
    import matte_cases as mc
    from tdnet_amd.dataloader import luma_u8, nearest_index
    src = mc.comp_source(kind, size)
    want_l = luma_u8(src[2])
    want_m = matte[nearest_index(33, size[0])][:, nearest_index(65, size[1])]
    for how in (dict(x=px, ids=ids), dict(matte=matte)):
        gl, gm = gather_op(lib, mem, src, **how)
        assert np.array_equal(gl, want_l), (kind, size, list(how), int((gl != want_l).sum()))
        assert np.array_equal(gm, want_m), (kind, size, list(how), int((gm != want_m).sum()))


def check_frames(dev, owner, frames, P, opts_note=""):
    """Whole frames on shared handles of `owner` (an Engine with weights at 33 x 65): the refined entry, the composite entries with refinement on (colour into
    the block, alpha into a BGRA32 view, the unfused entry), the split frame, launch counts, radius 0 restoring today's bytes and counts, the workspace in
    tdnet_memory_bytes, the error paths.  Every comparison is exact against the oracles on the matte entry's own bytes."""
    import pytest
    import matte_cases as mc
    from tdnet_amd import _capi
    from tdnet_amd.dataloader import PIX_BGRA32, composite_u8, luma_u8, nearest_index, view_extent
    ys, xs = nearest_index(H, HS), nearest_index(W, WS)
    a, b, c = owner.share(), owner.share(), owner.share()
    for e in (a, b, c):
        e.set_matte(MOVING)
    a.set_input_u8(HS, WS)
    b.set_matte_refine(FRAME_R, FRAME_EPS)                             # before the byte input: the workspace follows it
    mem0 = b.memory_bytes()[1]
    b.set_input_u8(HS, WS)
    b.set_output_composite(BG)
    grown = b.memory_bytes()[1] - mem0
    b.set_matte_refine(FRAME_R, FRAME_EPS)                             # idempotent
    assert b.memory_bytes()[1] - mem0 == grown and grown >= 9 * HS * WS + 4 * (HS + WS)
    c.set_input_u8(HS, WS)
    c.set_output_composite(None)                                       # the alpha mode into a BGRA32 view
    dview = mc.comp_dest(PIX_BGRA32, (HS, WS))
    c.set_output_view(dview)
    c.set_matte_refine(16, 4)                                          # after the byte input; another radius and eps per handle
    n = view_extent(dview)
    put = lambda arr: dev.put(np.ascontiguousarray(arr))
    for t, src in enumerate(frames):
        s = put(src)
        l8, m8 = put(np.full((H, W), 0xEE, np.uint8)), put(np.full((H, W), 0xEE, np.uint8))
        a.forward_u8_matte(dev.ptr(s), t % P, dev.ptr(l8), dev.ptr(m8), dev.stream)
        L = a.last_launch_count()
        m = dev.get(m8).reshape(H, W)
        guide, msrc = luma_u8(src), m[ys][:, xs]
        want = refine_matte_u8(guide, msrc, FRAME_R, FRAME_EPS)
        hold = put(np.full(HS * WS + 32, 0xEE, np.uint8))
        off = 16 + (t & 3)
        if t % 2 == 0:
            b.forward_u8_matte_refined(dev.ptr(s), t % P, dev.ptr(hold) + off, dev.stream)
            assert b.last_launch_count() == L + 2, (t, b.last_launch_count(), L)
        else:                                                          # the split frame
            b.encode_u8(dev.ptr(s), t % P, dev.stream)
            b.propagate_matte_refined(dev.ptr(s), dev.ptr(hold) + off, dev.stream)
        got = dev.get(hold)
        assert (got[:off] == 0xEE).all() and (got[off + HS * WS:] == 0xEE).all(), t
        assert np.array_equal(got[off:off + HS * WS].reshape(HS, WS), want), (opts_note, t, int((got[off:off + HS * WS].reshape(HS, WS) != want).sum()))
        # the composite entries through the refined matte, on the handle a's FIFO twin c (alpha) and through the unfused entry on b
        pic = composite_u8(src, want, HS, WS, BG)
        un = put(np.full((HS, WS, 3), 0xEE, np.uint8))
        b.matte_composite(dev.ptr(m8), dev.ptr(s), dev.ptr(un), dev.stream)
        assert np.array_equal(dev.get(un).reshape(HS, WS, 3), pic), (opts_note, t)
        prefill = np.full(n, 0xA5, np.uint8)
        dst = put(prefill.copy())
        if t % 2 == 0:
            c.forward_u8_composite(dev.ptr(s), t % P, dev.ptr(dst), dev.stream)
            assert c.last_launch_count() == L + 3, (t, c.last_launch_count(), L)
        else:
            c.encode_u8(dev.ptr(s), t % P, dev.stream)
            c.propagate_composite(dev.ptr(s), dev.ptr(dst), dev.stream)
        rgba = composite_u8(src, refine_matte_u8(guide, msrc, 16, 4), HS, WS, None)
        assert np.array_equal(dev.get(dst).reshape(-1), mc.expected_dest(prefill, dview, np.ascontiguousarray(rgba[..., :3]), rgba[..., 3])), (opts_note, t)
    assert a.fifo_len() == b.fifo_len() == c.fifo_len()
    # the colour composite fused, then radius 0 on the SAME handle: today's bytes and launch count
    src = frames[-1]
    t = len(frames)
    s = put(src)
    l8, m8 = put(np.full((H, W), 0xEE, np.uint8)), put(np.full((H, W), 0xEE, np.uint8))
    a.forward_u8_matte(dev.ptr(s), t % P, dev.ptr(l8), dev.ptr(m8), dev.stream)
    L = a.last_launch_count()
    m = dev.get(m8).reshape(H, W)
    out = put(np.full((HS, WS, 3), 0xEE, np.uint8))
    b.forward_u8_composite(dev.ptr(s), t % P, dev.ptr(out), dev.stream)
    assert b.last_launch_count() == L + 3
    assert np.array_equal(dev.get(out).reshape(HS, WS, 3), composite_u8(src, refine_matte_u8(luma_u8(src), m[ys][:, xs], FRAME_R, FRAME_EPS), HS, WS, BG))
    with_ws = b.memory_bytes()[1]
    b.set_matte_refine(0)
    assert b.memory_bytes()[1] == with_ws - (9 * HS * WS + 4 * (HS + WS))
    t += 1
    a.forward_u8_matte(dev.ptr(s), t % P, dev.ptr(l8), dev.ptr(m8), dev.stream)
    L = a.last_launch_count()
    m = dev.get(m8).reshape(H, W)
    b.forward_u8_composite(dev.ptr(s), t % P, dev.ptr(out), dev.stream)
    assert b.last_launch_count() == L
    assert np.array_equal(dev.get(out).reshape(HS, WS, 3), composite_u8(src, m, H, W, BG))
    b.matte_composite(dev.ptr(m8), dev.ptr(s), dev.ptr(out), dev.stream)
    assert np.array_equal(dev.get(out).reshape(HS, WS, 3), composite_u8(src, m, H, W, BG))
    # the error paths name the missing call and leave a pending frame alone
    e = owner.share()
    out1 = put(np.full((HS, WS), 0xEE, np.uint8))
    for bad in ((17, 65), (-1, 65), (4, 3), (4, 65026)):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_matte_refine.*(radius|eps)"):
            e.set_matte_refine(*bad)
    e.set_input_u8(HS, WS)
    e.encode_u8(dev.ptr(s), 0, dev.stream)                             # a pending frame: every failure below must leave it pending
    calls = (("tdnet_forward_u8_matte_refined", lambda: e.forward_u8_matte_refined(dev.ptr(s), 1, dev.ptr(out1), dev.stream)),
             ("tdnet_propagate_matte_refined", lambda: e.propagate_matte_refined(dev.ptr(s), dev.ptr(out1), dev.stream)))
    for name, call in calls:
        with pytest.raises(_capi.TdnetError, match=name + ".*tdnet_set_matte"):
            call()
    e.set_matte(MOVING)
    for name, call in calls:
        with pytest.raises(_capi.TdnetError, match=name + ".*tdnet_set_matte_refine"):
            call()
    e.set_matte_refine(FRAME_R, FRAME_EPS)
    with pytest.raises(_capi.TdnetError, match="tdnet_propagate_matte_refined.*overlaps"):
        e.propagate_matte_refined(dev.ptr(s), dev.ptr(s) + 5, dev.stream)
    with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_matte_refined.*waiting for tdnet_propagate"):
        e.forward_u8_matte_refined(dev.ptr(s), 1, dev.ptr(out1), dev.stream)
    with pytest.raises(_capi.TdnetError, match="tdnet_propagate_matte_refined: null"):
        e.propagate_matte_refined(dev.ptr(s), None, dev.stream)
    assert e.fifo_len() == 0 and (dev.get(out1) == 0xEE).all()
    e.propagate_matte_refined(dev.ptr(s), dev.ptr(out1), dev.stream)   # ... which is still there
    assert e.fifo_len() == 1 and not (dev.get(out1) == 0xEE).all()
    nob = owner.share()                                                # no byte input
    nob.set_matte(MOVING)
    nob.set_matte_refine(FRAME_R, FRAME_EPS)
    with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_matte_refined.*tdnet_set_input_u8"):
        nob.forward_u8_matte_refined(dev.ptr(s), 0, dev.ptr(out1), dev.stream)
    for h in (a, b, c, e, nob):
        h.close()
