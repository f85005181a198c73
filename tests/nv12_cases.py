"""Cases and expected values shared by tests/test_nv12_host.py (CPU, no library), tests/test_emu_nv12.py (CPU, through the emulator) and
tests/test_gpu_nv12.py (device memory): NV12 surfaces into the frame's first launch (include/tdnet.h "NV12 frames in").

The oracle is dataloader.nv12_to_rgb_u8 (pinned by hand in test_nv12_host.py) followed by what the uint8 entries already define on RGB bytes
(ingest_u8_cases.expected_image, the library's own packed-RGB route).  Every comparison the three files make is exact."""
import functools
import itertools

import numpy as np

import ingest_u8_cases as u8cases
from tdnet_amd.dataloader import nv12_extent, nv12_to_rgb_u8, resize_linear_u8

# (Y, U, V) -> (R, G, B) for standard 0, derived by hand from the specification's integers (1220542, 2116026, -409993, -852492, 1673527)
PINS = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)),
        ((41, 240, 110), (0, 0, 255)), ((128, 128, 128), (130, 130, 130)), ((0, 0, 0), (0, 154, 0)), ((255, 255, 255), (255, 125, 255)),
        ((255, 0, 0), (74, 255, 20))]
# standard -> (yoff, CY, CUB, CUG, CVG, CVR) as the specification's table states them
TABLE = {0: (16, 1220542, 2116026, -409993, -852492, 1673527), 1: (16, 1220542, 2214593, -223347, -558891, 1880097),
         2: (0, 1048576, 1858077, -360853, -748826, 1470104), 3: (0, 1048576, 1945738, -196423, -490864, 1651297)}
DECIMALS = {0: (1.164, 2.018, -0.391, -0.813, 1.596), 1: (1.164, 2.112, -0.213, -0.533, 1.793),
            2: (1.0, 1.772, -0.344136, -0.714136, 1.402), 3: (1.0, 1.8556, -0.187324, -0.468124, 1.5748)}

# (name, (Hs, Ws), (H, W)): the op-level cases
STEM_CASES = [
    ("same_33x65_all_y", (33, 65), (33, 65)),
    ("same_8x12", (8, 12), (8, 12)),
    ("same_7x31", (7, 31), (7, 31)),
    ("same_1x1", (1, 1), (1, 1)),
    ("same_2x2", (2, 2), (2, 2)),
    ("down_41x83", (41, 83), (33, 65)),
    ("down_exact_2x", (66, 130), (33, 65)),
    ("up_20x37", (20, 37), (33, 65)),
    ("aniso_50x40", (50, 40), (33, 65)),
    ("one_row_1x9", (1, 9), (5, 9)),
    ("one_col_9x1", (9, 1), (9, 5)),
    ("corners_2x250", (2, 250), (2, 250)),
]
# wider than one workgroup's strip (256 lanes x 4 columns): device only (the emulator runs a workgroup's lanes one after the other)
WIDE_CASES = [("same_6x2051", (6, 2051), (6, 2051)), ("down_9x2100", (9, 2100), (8, 2051))]
CORNER_VALUES = (0, 16, 128, 235, 255)


def layouts(Hs, Ws):
    """[(tag, pitch, uv_offset)]: the tight surface and a padded one (pitch 96, or 256 where a row is longer -- the wide cases: the next
    multiple of 256 --, and three rows of gap between the planes)."""
    row = 2 * ((Ws + 1) // 2)
    padded = 96 if row <= 96 else (row + 255) // 256 * 256
    return [("tight", row, Hs * row), ("padded", padded, (Hs + 3) * padded)]


@functools.lru_cache(maxsize=None)
def planes(name, Hs, Ws):
    """(Y [Hs, Ws], UV [ceil(Hs/2), ceil(Ws/2), 2]) random bytes; the first case's Y holds all 256 values; the corners case one (Y, U, V) of
    CORNER_VALUES^3 per 2 x 2 block."""
    rng = np.random.default_rng(Hs * 20011 + Ws)
    hc, wc = (Hs + 1) // 2, (Ws + 1) // 2
    Y = rng.integers(0, 256, (Hs, Ws), dtype=np.uint8)
    UV = rng.integers(0, 256, (hc, wc, 2), dtype=np.uint8)
    if name == "same_33x65_all_y":
        Y.reshape(-1)[:256] = np.roll(np.arange(256, dtype=np.uint8), 17)
    if name == "corners_2x250":
        combos = np.array(list(itertools.product(CORNER_VALUES, repeat=3)), dtype=np.uint8)   # 125 blocks
        assert (Hs, Ws) == (2, 2 * len(combos))
        Y[:] = np.repeat(combos[:, 0], 2)[None, :]
        UV[0] = combos[:, 1:]
    Y.setflags(write=False)
    UV.setflags(write=False)
    return Y, UV


def surface(name, Hs, Ws, pitch, uv_offset, fill=0, swap_uv=False):
    """The bytes [0, extent) of the case's surface in that layout; pitch padding and the gap between the planes hold `fill`."""
    Y, UV = planes(name, Hs, Ws)
    hc, wc = UV.shape[:2]
    s = np.full(nv12_extent(Hs, Ws, pitch, uv_offset), fill, np.uint8)
    for y in range(Hs):
        s[y * pitch:y * pitch + Ws] = Y[y]
    for j in range(hc):
        s[uv_offset + j * pitch:uv_offset + j * pitch + 2 * wc] = (UV[j, :, ::-1] if swap_uv else UV[j]).reshape(-1)
    return s


def offset_copy(s, off):
    """(holder, address): the surface's bytes `off` bytes into a larger buffer whose other bytes are 0xA5."""
    return u8cases.offset_copy(s, off)


@functools.lru_cache(maxsize=None)
def expected_rgb(name, Hs, Ws, standard=0):
    """The oracle's RGB bytes [Hs, Ws, 3] of the case (the layout does not matter: taken from the tight surface)."""
    _, pitch, uv = layouts(Hs, Ws)[0]
    rgb = nv12_to_rgb_u8(surface(name, Hs, Ws, pitch, uv), Hs, Ws, pitch, uv, standard)
    rgb.setflags(write=False)
    return rgb


def expected_image(name, Hs, Ws, H, W, standard=0, mean=None, std=None):
    """The fp32 NCHW tensor the frame must be: the host loader's image of the oracle's RGB bytes."""
    return u8cases.expected_image(expected_rgb(name, Hs, Ws, standard), H, W, mean, std)


def convert_pixels(Y, U, V, standard=0):
    """The oracle applied pixel by pixel to full-resolution planes [..]: each pixel becomes a 1 x 2 surface with its own chroma pair."""
    Y, U, V = (np.asarray(a, dtype=np.uint8).reshape(-1) for a in (Y, U, V))
    n = Y.size
    s = np.concatenate([np.repeat(Y, 2), np.stack([U, V], axis=1).reshape(-1)])
    return nv12_to_rgb_u8(s, 1, 2 * n, 2 * n, 2 * n, standard)[0, ::2]


def resized_rgb(name, Hs, Ws, H, W):
    """uint8 [H, W, 3]: the oracle's order -- convert every source pixel, then resize."""
    return resize_linear_u8(expected_rgb(name, Hs, Ws), (W, H))


def resized_yuv_then_converted(name, Hs, Ws, H, W):
    """uint8 [H, W, 3]: the WRONG order -- resize Y and the replicated chroma, convert afterwards."""
    Y, UV = planes(name, Hs, Ws)
    full = np.stack([Y, UV[np.arange(Hs) >> 1][:, np.arange(Ws) >> 1, 0], UV[np.arange(Hs) >> 1][:, np.arange(Ws) >> 1, 1]], axis=-1)
    r = resize_linear_u8(np.ascontiguousarray(full), (W, H))
    return convert_pixels(r[..., 0], r[..., 1], r[..., 2]).reshape(H, W, 3)


def scalar_convert(Y, U, V, standard=0):
    """The specification in plain Python integers (>> on a negative int is arithmetic), one pixel."""
    yoff, CY, CUB, CUG, CVG, CVR = TABLE[standard]
    yy, u, v = max(0, Y - yoff) * CY, U - 128, V - 128
    raw = ((yy + (1 << 19) + CVR * v) >> 20, (yy + (1 << 19) + CVG * v + CUG * u) >> 20, (yy + (1 << 19) + CUB * u) >> 20)
    return tuple(min(255, max(0, c)) for c in raw), raw


double3 = u8cases.double3
ALT_MEAN, ALT_STD = u8cases.ALT_MEAN, u8cases.ALT_STD


# ---- whole frames: one scenario for the emulator (numpy memory) and the device (torch memory) -------------------------------------------
FRAME_NET, FRAME_SRC, FRAME_PITCH = (33, 65), (42, 84), 96


@functools.lru_cache(maxsize=None)
def frame_surfaces(n=5, Hs=42, Ws=84, pitch=96):
    """n random surfaces [extent] (tight planes, padded pitch; padding 0x5A) and their oracle RGB bytes."""
    rng = np.random.default_rng(Hs * 7 + Ws)
    out = []
    for _ in range(n):
        s = np.full(nv12_extent(Hs, Ws, pitch, Hs * pitch), 0x5A, np.uint8)
        hc, wc = (Hs + 1) // 2, (Ws + 1) // 2
        for y in range(Hs):
            s[y * pitch:y * pitch + Ws] = rng.integers(0, 256, Ws, dtype=np.uint8)
        for j in range(hc):
            s[(Hs + j) * pitch:(Hs + j) * pitch + 2 * wc] = rng.integers(0, 256, 2 * wc, dtype=np.uint8)
        s.setflags(write=False)
        out.append((s, nv12_to_rgb_u8(s, Hs, Ws, pitch, Hs * pitch, 0)))
    return out


def run_frame_scenario(a, mem):
    """`a`: a finalized td2-psp18 Engine at FRAME_NET.  mem.up(array) -> (keepalive, address); mem.out(shape, dtype, fill) -> buffer;
    mem.addr(buffer); mem.get(buffer) -> numpy (synchronises).  Handle A gets the oracle's RGB bytes through the uint8 entries, handle B -- a
    shared handle -- the surfaces after set_input_nv12: identical logits, cache entries and launch counts at every step, with B switched to
    set_input_u8 and back in the middle; then every other byte entry once against its RGB-byte counterpart, and an odd-sized surface."""
    (H, W), (Hs, Ws), pitch, nc = FRAME_NET, FRAME_SRC, FRAME_PITCH, 19
    spec_dv = a.cache_dims()[2]
    b = a.share()
    a.set_input_u8(Hs, Ws)
    b.set_input_nv12(Hs, Ws, pitch)
    b.set_input_nv12(Hs, Ws, pitch, Hs * pitch, 0)                     # idempotent (uv_offset None = Hs * pitch)
    lk, dk, dv = a.cache_dims()
    frames = frame_surfaces()

    def step(t, via_u8_on_b=False):
        s, rgb = frames[t]
        ka, pa = mem.up(rgb)
        oa, ob = mem.out((1, nc, H, W), np.float32, 7e7), mem.out((1, nc, H, W), np.float32, -7e7)
        a.forward_u8(pa, t % 2, mem.addr(oa))
        if via_u8_on_b:
            b.set_input_u8(Hs, Ws)
            b.forward_u8(pa, t % 2, mem.addr(ob))
            b.set_input_nv12(Hs, Ws, pitch)
        else:
            ks, ps = mem.up(s, off=t % 3)                              # base addresses 0, 1, 2 bytes into a buffer
            b.forward_u8(ps, t % 2, mem.addr(ob))
        ga, gb = mem.get(oa), mem.get(ob)
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), t
        assert a.last_launch_count() == b.last_launch_count() > 0, t
        for st, shp in (("cache_q", (lk, dk)), ("cache_k", (lk, dk)), ("cache_v", (lk, dv))):
            assert np.array_equal(a.stage(st, shp).view(np.uint32), b.stage(st, shp).view(np.uint32)), (t, st)
        assert a.fifo_len() == b.fifo_len()
        return ga

    for t in range(5):
        logits = step(t, via_u8_on_b=(t == 2))
    assert spec_dv == dv
    # the other byte entries, once each: C on RGB bytes, D on the surface
    c, d = a.share(), a.share()
    c.set_input_u8(Hs, Ws)
    before = d.memory_bytes()[1]
    d.set_input_nv12(Hs, Ws, pitch)
    assert d.memory_bytes()[1] > before                                # the tables are counted in the handle's bytes
    s, rgb = frames[0]
    (k1, pr), (k2, ps) = mem.up(rgb), mem.up(s, off=1)
    la, lb = mem.out((H, W), np.uint8, 0xEE), mem.out((H, W), np.uint8, 0xEE)
    c.forward_u8_labels(pr, 0, mem.addr(la)); d.forward_u8_labels(ps, 0, mem.addr(lb))
    assert np.array_equal(mem.get(la), mem.get(lb)) and c.last_launch_count() == d.last_launch_count()
    pal = np.arange(19 * 3, dtype=np.uint8).reshape(19, 3)
    oh, ow = H // 4, W // 4
    ra, rb = mem.out((oh, ow, 3), np.uint8, 0xEE), mem.out((oh, ow, 3), np.uint8, 0xEE)
    for e in (c, d):
        e.set_output_rgb(oh, ow, pal)
    c.forward_u8_rgb(pr, 1, mem.addr(ra)); d.forward_u8_rgb(ps, 1, mem.addr(rb))
    assert np.array_equal(mem.get(ra), mem.get(rb))
    gt = np.random.default_rng(3).integers(0, 19, (H, W), dtype=np.uint8)
    kg, pg = mem.up(gt)
    for e in (c, d):
        e.set_score(None)
    c.forward_u8_score(pr, 0, pg, mem.addr(la)); d.forward_u8_score(ps, 0, pg, mem.addr(lb))
    assert np.array_equal(mem.get(la), mem.get(lb))
    cm_c, cm_d = c.score_read(), d.score_read()
    assert np.array_equal(cm_c, cm_d) and int(cm_c.sum()) == H * W
    ca, cb = mem.out((H, W), np.uint8, 0xEE), mem.out((H, W), np.uint8, 0xEE)
    c.forward_u8_labels_conf(pr, 1, mem.addr(la), mem.addr(ca)); d.forward_u8_labels_conf(ps, 1, mem.addr(lb), mem.addr(cb))
    assert np.array_equal(mem.get(la), mem.get(lb)) and np.array_equal(mem.get(ca), mem.get(cb))
    c.encode_u8(pr, 0); d.encode_u8(ps, 0)
    c.propagate_labels_u8(mem.addr(la)); d.propagate_labels_u8(mem.addr(lb))
    assert np.array_equal(mem.get(la), mem.get(lb)) and c.fifo_len() == d.fifo_len()
    # an odd-sized surface, tight pitch
    Ho, Wo = 41, 83
    _, po, uo = layouts(Ho, Wo)[0]
    so = surface("down_41x83", Ho, Wo, po, uo)
    c.set_input_u8(Ho, Wo); d.set_input_nv12(Ho, Wo, po, uo)
    (k3, pr), (k4, ps) = mem.up(expected_rgb("down_41x83", Ho, Wo)), mem.up(so, off=1)
    oa, ob = mem.out((1, nc, H, W), np.float32, 7e7), mem.out((1, nc, H, W), np.float32, -7e7)
    c.forward_u8(pr, 1, mem.addr(oa)); d.forward_u8(ps, 1, mem.addr(ob))
    assert np.array_equal(mem.get(oa).view(np.uint32), mem.get(ob).view(np.uint32))
    assert not np.array_equal(mem.get(oa), logits)
    for e in (b, c, d):
        e.close()
