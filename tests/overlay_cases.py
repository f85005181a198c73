"""Cases, expected values and scenarios shared by tests/test_emu_overlay.py (CPU, through the emulator) and tests/test_gpu_overlay.py (device memory):
the class colours blended over the source frame (include/tdnet.h "overlay out").

Expected values come from code that predates the feature wherever possible: labels from tdnet_op_upsample_argmax / forward_u8_labels, the sampling
from dataloader.nearest_index, NV12 source pixels from dataloader.nv12_to_rgb_u8; the blend from dataloader.overlay_u8, itself pinned by the
hand-computed BLEND_PINS in a host-only test.  Every comparison is exact.

A scenario takes `mem`: mem.up(array, off=0) -> (keepalive, address) -- the array's bytes `off` bytes into a holder of 0xA5; mem.out(nbytes) -> a
holder of 0xEE bytes; mem.addr(holder); mem.get(holder) -> numpy uint8 (synchronises); mem.stream."""
import functools

import numpy as np

import opcheck

from ingest_u8_cases import ARGMAX_CASES, lowres_logits  # noqa: F401  (re-exported: the logits of the operator cases)
from rgb_out_cases import expected_picture, logits40, out_sizes, palette19  # noqa: F401
from tdnet_amd.dataloader import nv12_extent, nv12_to_rgb_u8, overlay_u8, rgb_to_nv12

# (c, s, a) -> out, by hand from A = a + (a >> 7), out = (c A + s (256 - A) + 128) >> 8:
#   a = 0 -> A = 0: s;  a = 255 -> A = 256: c;  a = 127 -> A = 127: (200 * 127 + 100 * 129 + 128) >> 8 = 38428 >> 8 = 150;
#   a = 128 -> A = 129: (200 * 129 + 100 * 127 + 128) >> 8 = 38628 >> 8 = 150;  (255, 0, 127): 32513 >> 8 = 127;  (255, 0, 128): 33023 >> 8 = 128;
#   (0, 255, 127): (255 * 129 + 128) >> 8 = 33023 >> 8 = 128;  (0, 255, 128): (255 * 127 + 128) >> 8 = 32513 >> 8 = 127;
#   (255, 255, 77): (255 * 256 + 128) >> 8 = 255;  (1, 0, 1): (1 + 128) >> 8 = 0;  (0, 1, 254): A = 255: (1 + 128) >> 8 = 0;  (3, 250, 64): (192 + 48000 + 128) >> 8 = 188
BLEND_PINS = [((200, 100, 0), 100), ((200, 100, 255), 200), ((200, 100, 127), 150), ((200, 100, 128), 150), ((255, 0, 127), 127), ((255, 0, 128), 128),
              ((0, 255, 127), 128), ((0, 255, 128), 127), ((255, 255, 77), 255), ((1, 0, 1), 0), ((0, 1, 254), 0), ((3, 250, 64), 188)]
WEIGHT_PINS = {0: 0, 1: 1, 127: 127, 128: 129, 254: 255, 255: 256}
SRC_OFFSETS = (0, 1, 5, 15)
# wider than one workgroup's strip (256 lanes x 4 pixels): device only.  (name, (h, w), (H, W), [(Hs, Ws), ...])
WIDE_CASES = [("wide", (2, 300), (6, 2051), [(6, 2051), (9, 2100)]), ("native_769x1537", (97, 193), (769, 1537), [(1024, 2048)])]


def rgba(palette_rgb, alpha):
    """[n, 4] bytes: the colours with the byte(s) `alpha` (a scalar or one per class) behind them."""
    p = np.asarray(palette_rgb, np.uint8)
    out = np.empty((len(p), 4), np.uint8)
    out[:, :3] = p
    out[:, 3] = alpha
    return out


def pal_half():
    """Cityscapes at one alpha (128: weight 129)."""
    return rgba(palette19(), 128)


def pal_mixed():
    """Per-class alpha with zeros in it: "tint some classes, leave the others alone"."""
    return rgba(palette19(), [0, 255, 127, 128, 0, 64, 1, 254, 0, 200, 33, 0, 90, 255, 0, 7, 180, 0, 128])


@functools.lru_cache(maxsize=None)
def source_rgb(Hs, Ws, seed=0):
    s = np.random.default_rng(Hs * 30011 + Ws * 7 + seed).integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
    s.setflags(write=False)
    return s


def nv12_layouts(Hs, Ws):
    """[(tag, pitch, uv_offset)]: tight, and padded (pitch larger than the row, three rows of gap between the planes)."""
    row = 2 * ((Ws + 1) // 2)
    padded = 96 if row <= 90 else (row + 6 + 255) // 256 * 256
    return [("tight", row, Hs * row), ("padded", padded, (Hs + 3) * padded)]


def nv12_surface(rgb, pitch, uv_offset, standard=0, pad_fill=0, gap_fill=0):
    """The bytes [0, extent) of an NV12 surface of `rgb` (planes from dataloader.rgb_to_nv12) in that layout; the pitch padding holds pad_fill,
    the gap between the planes gap_fill."""
    Hs, Ws = rgb.shape[:2]
    hc, wc = (Hs + 1) // 2, (Ws + 1) // 2
    tight = rgb_to_nv12(rgb, pitch=2 * wc, standard=standard)
    s = np.full(nv12_extent(Hs, Ws, pitch, uv_offset), gap_fill, np.uint8)
    for y in range(Hs):
        s[y * pitch:(y + 1) * pitch] = pad_fill
        s[y * pitch:y * pitch + Ws] = tight[y, :Ws]
    for j in range(hc):
        a = uv_offset + j * pitch
        s[a:min(a + pitch, s.size)] = pad_fill
        s[a:a + 2 * wc] = tight[Hs + j, :2 * wc]
    return s


def labels_of(lib, mem, x, C, h, w, H, W):
    """int32 labels [H, W] of the logits through the uint8-free label kernel (code that predates the feature)."""
    kx, px = mem.up(x)
    out = mem.out(H * W * 4)
    lib.check(lib.tdnet_op_upsample_argmax(px, C, h, w, H, W, mem.addr(out), None, mem.stream))
    l32 = mem.get(out).view(np.int32).reshape(H, W).copy()
    assert l32.min() >= 0 and l32.max() < C
    return l32


def op_overlay(lib, mem, H, W, Hs, Ws, pal, src_bytes, src_off, out_off, nv=None, x=None, labels_u8=None):
    """tdnet_op_overlay: the picture written `out_off` bytes into a holder of 0xEE (the guard bytes around it must survive), the source `src_off`
    bytes into a holder of 0xA5.  nv: None (packed RGB) or (pitch, uv_offset, standard).  x: logits [C, h, w] (fused kernel) or labels_u8 [H, W].
    The logits go in between guard bands, once per band fill (opcheck.each_poison): the same bytes both times."""
    if x is None:
        return _op_overlay(lib, mem, H, W, Hs, Ws, pal, src_bytes, src_off, out_off, nv, x, labels_u8, None)
    return opcheck.each_poison(x, mem.stream is not None, lambda px: _op_overlay(lib, mem, H, W, Hs, Ws, pal, src_bytes, src_off, out_off, nv, x, labels_u8, px))


def _op_overlay(lib, mem, H, W, Hs, Ws, pal, src_bytes, src_off, out_off, nv, x, labels_u8, px):
    n = Hs * Ws * 3
    ks, ps = mem.up(src_bytes, src_off)
    holder = mem.out(n + 16)
    pal = np.ascontiguousarray(pal)
    if x is not None:
        C, h, w = x.shape
        pl = None
    else:
        C = h = w = 0
        px = None
        kl, pl = mem.up(labels_u8, 3)                                  # a label map at an odd address
    pitch, uv, std = nv if nv is not None else (0, 0, 0)
    lib.check(lib.tdnet_op_overlay(px, C, h, w, H, W, pl, ps, 0 if nv is None else 1, Hs, Ws, pitch, uv, std, pal.ctypes.data, len(pal),
                                   mem.addr(holder) + out_off, mem.stream))
    host = mem.get(holder)
    assert (host[:out_off] == 0xEE).all() and (host[out_off + n:] == 0xEE).all(), (Hs, Ws, out_off)
    return host[out_off:out_off + n].reshape(Hs, Ws, 3)


def run_operator_case(lib, mem, name, C, lo, hi, sizes=None, nv12_offs=(0, 3)):
    """One ARGMAX case crossed with the source sizes: fused and label-map kernels, packed RGB at every out offset 0..3 (source offsets 0, 1, 5, 15)
    and NV12 in the padded layout at an odd base."""
    (h, w), (H, W) = lo, hi
    x = lowres_logits(name, C, h, w)
    labels = labels_of(lib, mem, x, C, h, w, H, W)
    l8 = np.ascontiguousarray(labels.astype(np.uint8))
    pal = pal_half()
    for Hs, Ws in (sizes or out_sizes(H, W)):
        src = source_rgb(Hs, Ws)
        want = overlay_u8(src, labels, pal)
        for off in range(4):
            got = op_overlay(lib, mem, H, W, Hs, Ws, pal, src, SRC_OFFSETS[off], off, x=x)
            assert np.array_equal(got, want), (name, "rgb fused", Hs, Ws, off)
        for off in (0, 1):
            got = op_overlay(lib, mem, H, W, Hs, Ws, pal, src, SRC_OFFSETS[3 - off], off, labels_u8=l8)
            assert np.array_equal(got, want), (name, "rgb labels", Hs, Ws, off)
        _, pitch, uv = nv12_layouts(Hs, Ws)[1]
        surf = nv12_surface(src, pitch, uv, 0, 0x5A, 0xC3)
        want = overlay_u8(nv12_to_rgb_u8(surf, Hs, Ws, pitch, uv, 0), labels, pal)
        for off in nv12_offs:
            got = op_overlay(lib, mem, H, W, Hs, Ws, pal, surf, 1 + off, off, nv=(pitch, uv, 0), x=x)
            assert np.array_equal(got, want), (name, "nv12 fused", Hs, Ws, off)
        got = op_overlay(lib, mem, H, W, Hs, Ws, pal, surf, 2, 1, nv=(pitch, uv, 0), labels_u8=l8)
        assert np.array_equal(got, want), (name, "nv12 labels", Hs, Ws)
    return labels


def run_nv12_layouts_and_standards(lib, mem):
    """One case: tight and padded layouts, all four standards, odd sizes; the pitch padding and the plane gap filled with two different poison
    bytes in two runs that must give the same picture."""
    name, C, (h, w), (H, W) = ARGMAX_CASES[0]
    x = lowres_logits(name, C, h, w)
    labels = labels_of(lib, mem, x, C, h, w, H, W)
    pal = pal_mixed()
    for Hs, Ws in ((41, 83), (8, 16), (7, 17), (1, 1), (3, 2)):
        src = source_rgb(Hs, Ws, 1)
        for std in range(4):
            for tag, pitch, uv in nv12_layouts(Hs, Ws):
                pics = []
                for pad_fill, gap_fill in ((0x11, 0xEE), (0xF0, 0x0F)):
                    surf = nv12_surface(src, pitch, uv, std, pad_fill, gap_fill)
                    want = overlay_u8(nv12_to_rgb_u8(surf, Hs, Ws, pitch, uv, std), labels, pal)
                    got = op_overlay(lib, mem, H, W, Hs, Ws, pal, surf, 5, 2, nv=(pitch, uv, std), x=x)
                    assert np.array_equal(got, want), (Hs, Ws, std, tag)
                    pics.append(got)
                assert np.array_equal(pics[0], pics[1]), (Hs, Ws, std, tag)
    assert not np.array_equal(nv12_to_rgb_u8(nv12_surface(source_rgb(41, 83, 1), 84, 41 * 84, 0), 41, 83, 84, 41 * 84, 0),
                              nv12_to_rgb_u8(nv12_surface(source_rgb(41, 83, 1), 84, 41 * 84, 0), 41, 83, 84, 41 * 84, 1))   # the standards differ


def run_palettes(lib, mem):
    """A per-class alpha with zeros in it; 40 classes against 19 colours (labels 19..39 show the source); all-zero and all-255 alpha."""
    name, C, (h, w), (H, W) = ARGMAX_CASES[0]
    x = lowres_logits(name, C, h, w)
    labels = labels_of(lib, mem, x, C, h, w, H, W)
    x40 = logits40(h, w)
    l40 = labels_of(lib, mem, x40, 40, h, w, H, W)
    assert (l40 >= 19).any() and (l40 < 19).any()
    for Hs, Ws in out_sizes(H, W):
        src = source_rgb(Hs, Ws, 2)
        for pal in (pal_mixed(), rgba(palette19(), 0), rgba(palette19(), 255)):
            got = op_overlay(lib, mem, H, W, Hs, Ws, pal, src, 1, 3, x=x)
            assert np.array_equal(got, overlay_u8(src, labels, pal)), (Hs, Ws)
        assert np.array_equal(got, expected_picture(labels, Hs, Ws, palette19()))   # all-255: the colour map of that size
        got = op_overlay(lib, mem, H, W, Hs, Ws, rgba(palette19(), 0), src, 5, 0, x=x)
        assert np.array_equal(got, src)                                 # all-zero: the source bytes
        got = op_overlay(lib, mem, H, W, Hs, Ws, rgba(palette19(), 255), src, 0, 1, x=x40)
        assert np.array_equal(got, overlay_u8(src, l40, rgba(palette19(), 255))), (Hs, Ws)
    full = op_overlay(lib, mem, H, W, H, W, rgba(palette19(), 255), source_rgb(H, W, 2), 0, 0, x=x40)
    outside = l40 >= 19
    assert np.array_equal(full[outside], source_rgb(H, W, 2)[outside]) and np.array_equal(full[~outside], palette19()[l40[~outside]])


def run_exhaustive_blend(lib, mem):
    """k_labels_overlay on a 256 x 256 label map with label = row, palette entry l with a = l, the source s = column in every channel: every
    (a, s) pair for six colour values against Python integers."""
    labels = np.ascontiguousarray(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1))
    src = np.ascontiguousarray(np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 256, axis=0).repeat(3, axis=2))
    for colours in ((0, 127, 255), (1, 128, 254)):
        pal = rgba(np.tile(np.array(colours, np.uint8), (256, 1)), np.arange(256))
        got = op_overlay(lib, mem, 256, 256, 256, 256, pal, src, 1, 1, labels_u8=labels)
        want = np.empty((256, 256, 3), np.uint8)
        for a in range(256):
            A = a + (a >> 7)
            for ch, c in enumerate(colours):
                want[a, :, ch] = [(c * A + s * (256 - A) + 128) >> 8 for s in range(256)]
        assert np.array_equal(got, want), colours


def run_wide_case(lib, mem, name, lo, hi, sizes):
    """Rows wider than one workgroup's strip (device only): RGB and NV12, fused and label-map kernels."""
    (h, w), (H, W) = lo, hi
    C = 19
    x = np.random.default_rng(H + W).standard_normal((C, h, w)).astype(np.float32)
    labels = labels_of(lib, mem, x, C, h, w, H, W)
    l8 = np.ascontiguousarray(labels.astype(np.uint8))
    pal = pal_mixed()
    for Hs, Ws in sizes:
        src = source_rgb(Hs, Ws, 3)
        want = overlay_u8(src, labels, pal)
        for off in (0, 3):
            assert np.array_equal(op_overlay(lib, mem, H, W, Hs, Ws, pal, src, SRC_OFFSETS[off], off, x=x), want), (name, Hs, Ws, off)
        assert np.array_equal(op_overlay(lib, mem, H, W, Hs, Ws, pal, src, 5, 1, labels_u8=l8), want), (name, Hs, Ws)
        _, pitch, uv = nv12_layouts(Hs, Ws)[1]
        surf = nv12_surface(src, pitch, uv, 1, 0x5A, 0xC3)
        want = overlay_u8(nv12_to_rgb_u8(surf, Hs, Ws, pitch, uv, 1), labels, pal)
        assert np.array_equal(op_overlay(lib, mem, H, W, Hs, Ws, pal, surf, 1, 2, nv=(pitch, uv, 1), x=x), want), (name, "nv12", Hs, Ws)
        assert np.array_equal(op_overlay(lib, mem, H, W, Hs, Ws, pal, surf, 3, 0, nv=(pitch, uv, 1), labels_u8=l8), want), (name, "nv12 labels", Hs, Ws)


# ---- whole frames: td4-resnet18 at 33x65, six frames of random bytes at 41x83 (test_emu_rgb_out.py's clip), the same clip as NV12 surfaces ------------
H, W, HS, WS, T = 33, 65, 41, 83, 6
HS2, WS2 = 20, 37                                                       # the second source size
PITCH = 96


@functools.lru_cache(maxsize=None)
def clip_frames():
    rng = np.random.default_rng(21)
    frames = [rng.integers(0, 256, (HS, WS, 3), dtype=np.uint8) for _ in range(T)]
    for f in frames:
        f.setflags(write=False)
    return frames


def clip_surface(t):
    """(surface bytes, its RGB by the oracle): frame t as an NV12 surface, pitch 96, poisoned padding."""
    s = nv12_surface(clip_frames()[t], PITCH, HS * PITCH, 0, 0x5A, 0xC3)
    return s, nv12_to_rgb_u8(s, HS, WS, PITCH, HS * PITCH, 0)


def frame_labels(owner, mem, src_rgb, pos, Hs, Ws):
    """The labels forward_u8_labels gives for the RGB bytes on `owner` (configured for them here), and its launch count."""
    owner.set_input_u8(Hs, Ws)
    k, p = mem.up(src_rgb)
    out = mem.out(H * W)
    owner.forward_u8_labels(p, pos, mem.addr(out), mem.stream)
    return mem.get(out).reshape(H, W).copy(), owner.last_launch_count()


def overlay_frame(e, mem, src_bytes, pos, Hs, Ws, src_off=0, out_off=0, how="forward", labels=None):
    """One frame asked for as an overlay on `e` (configured by the caller): how = "forward" | "labels" (forward_u8_labels + labels_overlay) |
    "split" (encode_u8 + propagate_overlay).  Returns the picture; the guard bytes of the 0xEE holder must survive."""
    n = Hs * Ws * 3
    k, p = mem.up(src_bytes, src_off)
    holder = mem.out(n + 16)
    dst = mem.addr(holder) + out_off
    if how == "forward":
        e.forward_u8_overlay(p, pos, dst, mem.stream)
    elif how == "labels":
        lab = mem.out(H * W)
        e.forward_u8_labels(p, pos, mem.addr(lab), mem.stream)
        if labels is not None:
            assert np.array_equal(mem.get(lab).reshape(H, W), labels)
        e.labels_overlay(mem.addr(lab), p, dst, mem.stream)
    else:
        e.encode_u8(p, pos, mem.stream)
        e.propagate_overlay(p, dst, mem.stream)
    host = mem.get(holder)
    assert (host[:out_off] == 0xEE).all() and (host[out_off + n:] == 0xEE).all()
    return host[out_off:out_off + n].reshape(Hs, Ws, 3)


def run_frames_follow_the_input(owner, mem, overlay_first):
    """forward_u8_overlay on a shared handle == overlay_u8(source, labels of forward_u8_labels on the owner, palette) for every frame, in as many
    launches, while the input configuration switches between RGB and NV12 and between two source sizes from frame to frame.  overlay_first:
    set_output_overlay is called once BEFORE any input configuration, else once after the first."""
    a = owner.share()
    pal = pal_mixed()
    if overlay_first:
        a.set_output_overlay(pal)
    owner.reset()
    base = a.memory_bytes()[1]
    for t in range(T):
        kind = t % 3                                                   # 0: RGB 41x83, 1: NV12 41x83, 2: RGB 20x37
        if kind == 1:
            src_bytes, rgb = clip_surface(t)
            Hs, Ws = HS, WS
        elif kind == 0:
            src_bytes = rgb = clip_frames()[t]
            Hs, Ws = HS, WS
        else:
            src_bytes = rgb = source_rgb(HS2, WS2, t)
            Hs, Ws = HS2, WS2
        labels, launches = frame_labels(owner, mem, rgb, t % 4, Hs, Ws)
        if kind == 1:
            a.set_input_nv12(Hs, Ws, PITCH)
        else:
            a.set_input_u8(Hs, Ws)
        if not overlay_first and t == 0:
            a.set_output_overlay(pal)
            a.set_output_overlay(pal)                                  # idempotent
        got = overlay_frame(a, mem, src_bytes, t % 4, Hs, Ws, src_off=t % 3, out_off=t % 4)
        assert np.array_equal(got, overlay_u8(rgb, labels, pal)), t
        assert a.last_launch_count() == launches > 0, t
    assert a.fifo_len() == owner.fifo_len()
    assert a.memory_bytes()[1] > base                                  # the tables are counted in the handle's bytes
    a.close()


def run_entries_mixed(owner, mem):
    """In turn forward_u8_overlay, forward_u8_labels + labels_overlay, encode_u8 + propagate_overlay on ONE handle, RGB on even frames and NV12
    on odd ones: the pictures of the definition."""
    c = owner.share()
    pal = pal_half()
    c.set_output_overlay(pal)
    owner.reset()
    for t in range(T):
        if t % 2:
            src_bytes, rgb = clip_surface(t)
            c.set_input_nv12(HS, WS, PITCH)
        else:
            src_bytes = rgb = clip_frames()[t]
            c.set_input_u8(HS, WS)
        labels, launches = frame_labels(owner, mem, rgb, t % 4, HS, WS)
        got = overlay_frame(c, mem, src_bytes, t % 4, HS, WS, src_off=1, out_off=t % 4, how=("forward", "labels", "split")[t % 3], labels=labels)
        assert np.array_equal(got, overlay_u8(rgb, labels, pal)), t
        if t % 3 == 0:
            assert c.last_launch_count() == launches
    assert c.fifo_len() == owner.fifo_len()
    c.close()


def run_alpha_extremes_and_rejection(owner, mem):
    """All-zero alpha returns the source bytes (NV12: nv12_to_rgb_u8 of the surface); all-255 alpha what forward_u8_rgb gives at (Hs, Ws);
    forward_u8_labels_conf with a threshold that rejects some pixels, then labels_overlay: rejected pixels are the bare frame."""
    e, r = owner.share(), owner.share()
    owner.reset()
    rgb = clip_frames()[0]
    surf, srgb = clip_surface(1)
    e.set_output_overlay(rgba(palette19(), 0))
    e.set_input_u8(HS, WS)
    assert np.array_equal(overlay_frame(e, mem, rgb, 0, HS, WS, 5, 1), rgb)
    e.set_input_nv12(HS, WS, PITCH)
    assert np.array_equal(overlay_frame(e, mem, surf, 1, HS, WS, 1, 2), srgb)
    e.set_output_overlay(rgba(palette19(), 255))
    e.set_input_u8(HS, WS)
    r.set_input_u8(HS, WS)
    r.set_output_rgb(HS, WS, palette19())
    for t in (0, 1):                                                   # r follows e's frames so far
        k, p = mem.up(clip_frames()[0] if t == 0 else srgb)
        pic = mem.out(HS * WS * 3)
        r.forward_u8_rgb(p, t, mem.addr(pic), mem.stream)
    k, p = mem.up(clip_frames()[2])
    pic = mem.out(HS * WS * 3)
    r.forward_u8_rgb(p, 2, mem.addr(pic), mem.stream)
    assert np.array_equal(overlay_frame(e, mem, clip_frames()[2], 2, HS, WS), mem.get(pic).reshape(HS, WS, 3))
    # rejection: labels with reject_label 255 >= n_colours, then the unfused overlay
    pal = rgba(palette19(), 255)
    k, p = mem.up(clip_frames()[3], 1)
    lab, conf = mem.out(H * W), mem.out(H * W)
    probe = owner.share()
    probe.set_input_u8(HS, WS)
    probe.forward_u8_labels_conf(p, 0, mem.addr(lab), mem.addr(conf), mem.stream)   # a first frame: its confidences choose the threshold
    cvals = np.sort(mem.get(conf).reshape(-1))
    thr = min(255, int(cvals[cvals.size // 3]) + 1)                   # rejects the lower third at least (unless every pixel is certain)
    probe.close()
    f = owner.share()
    f.set_input_u8(HS, WS)
    f.set_output_overlay(pal)
    f.set_confidence(thr, 255)
    f.forward_u8_labels_conf(p, 0, mem.addr(lab), mem.addr(conf), mem.stream)
    l8 = mem.get(lab).reshape(H, W).copy()
    rejected = l8 == 255
    assert rejected.any() and not rejected.all()
    out = mem.out(HS * WS * 3)
    f.labels_overlay(mem.addr(lab), p, mem.addr(out), mem.stream)
    got = mem.get(out).reshape(HS, WS, 3)
    assert np.array_equal(got, overlay_u8(clip_frames()[3], l8, pal))
    from tdnet_amd.dataloader import nearest_index
    rej_src = rejected[nearest_index(H, HS)][:, nearest_index(W, WS)]
    assert rej_src.any() and np.array_equal(got[rej_src], clip_frames()[3][rej_src])   # rejected pixels are the bare frame
    assert np.array_equal(got[~rej_src], palette19()[l8[nearest_index(H, HS)][:, nearest_index(W, WS)][~rej_src]])
    for h_ in (e, r, f):
        h_.close()


def run_pspnet_single_frame(e, mem):
    """A single-frame PSPNet handle `e`: forward_u8_overlay against the labels of forward_u8_labels, in as many launches."""
    rgb = clip_frames()[4]
    labels, launches = frame_labels(e, mem, rgb, 0, HS, WS)
    e.set_output_overlay(pal_mixed())
    got = overlay_frame(e, mem, rgb, 0, HS, WS, 15, 3)
    assert np.array_equal(got, overlay_u8(rgb, labels, pal_mixed())) and e.last_launch_count() == launches > 0
    surf, srgb = clip_surface(5)
    labels, _ = frame_labels(e, mem, srgb, 0, HS, WS)
    e.set_input_nv12(HS, WS, PITCH)
    assert np.array_equal(overlay_frame(e, mem, surf, 0, HS, WS, 2, 1), overlay_u8(srgb, labels, pal_mixed()))


def run_errors(owner, mem, lib, fresh_engine, error_type):
    """Each failure leaves the FIFO and a pending frame alone, and the message names what is missing."""
    import pytest
    e = owner.share()
    owner.reset()
    pal = pal_half()
    rgb = clip_frames()[0]
    k, p = mem.up(rgb)
    n = HS * WS * 3
    out, lab = mem.out(n), mem.out(H * W)
    po, pl = mem.addr(out), mem.addr(lab)
    calls = (lambda: e.forward_u8_overlay(p, 1, po, mem.stream), lambda: e.propagate_overlay(p, po, mem.stream), lambda: e.labels_overlay(pl, p, po, mem.stream))
    for call in calls:                                                 # nothing configured: the overlay is named first
        with pytest.raises(error_type, match="tdnet_set_output_overlay"):
            call()
    e.set_output_overlay(pal)
    for call in calls:                                                 # the overlay alone: the byte input is named
        with pytest.raises(error_type, match="tdnet_set_input_u8 or tdnet_set_input_nv12"):
            call()
    e.set_input_u8(HS, WS)
    e.encode_u8(p, 0, mem.stream)                                      # a pending frame: every failure below must leave it pending
    for bad, match in ((np.zeros((0, 4), np.uint8), "n_colours"), (np.zeros((257, 4), np.uint8), "n_colours")):
        with pytest.raises(error_type, match=match):
            e.set_output_overlay(bad)
    assert lib.tdnet_set_output_overlay(e.h, None, 19) < 0 and b"NULL" in lib.tdnet_last_error()   # a NULL palette
    for args in ((None, 1, po), (p, 1, None)):
        assert lib.tdnet_forward_u8_overlay(e.h, args[0], args[1], args[2], mem.stream) < 0 and b"null argument" in lib.tdnet_last_error()
    assert lib.tdnet_propagate_overlay(e.h, None, po, mem.stream) < 0 and b"null argument" in lib.tdnet_last_error()
    assert lib.tdnet_propagate_overlay(e.h, p, None, mem.stream) < 0 and b"null argument" in lib.tdnet_last_error()
    assert lib.tdnet_labels_overlay(e.h, None, p, po, mem.stream) < 0 and b"null argument" in lib.tdnet_last_error()
    assert lib.tdnet_labels_overlay(e.h, pl, None, po, mem.stream) < 0 and b"null argument" in lib.tdnet_last_error()
    assert lib.tdnet_labels_overlay(e.h, pl, p, None, mem.stream) < 0 and b"null argument" in lib.tdnet_last_error()
    for dst in (p, p + n - 1, p - n + 1):                              # out overlapping the packed image: both ends
        with pytest.raises(error_type, match="overlaps"):
            e.propagate_overlay(p, dst, mem.stream)
        with pytest.raises(error_type, match="overlaps"):
            e.labels_overlay(pl, p, dst, mem.stream)
    with pytest.raises(error_type, match="waiting for tdnet_propagate"):   # the forward form respects the pending frame like its siblings
        e.forward_u8_overlay(p, 1, po, mem.stream)
    assert e.fifo_len() == 0
    labels, _ = frame_labels(owner, mem, rgb, 0, HS, WS)
    e.propagate_overlay(p, po, mem.stream)                             # ... which is still there, and is the frame it was
    assert e.fifo_len() == 1 and np.array_equal(mem.get(out).reshape(HS, WS, 3), overlay_u8(rgb, labels, pal))
    with pytest.raises(error_type, match="no encoded frame"):
        e.propagate_overlay(p, po, mem.stream)
    # a pointer inside an NV12 surface's UV plane
    surf, _ = clip_surface(1)
    ks, ps = mem.up(surf)
    e.set_input_nv12(HS, WS, PITCH)
    ext = nv12_extent(HS, WS, PITCH, HS * PITCH)
    for dst in (ps + HS * PITCH + 10, ps + ext - 1):
        with pytest.raises(error_type, match="overlaps"):
            e.forward_u8_overlay(ps, 1, dst, mem.stream)
    assert e.fifo_len() == 1
    kb, pb = mem.up(np.concatenate([surf, np.zeros(n, np.uint8)]))     # right behind the extent is legal
    e.forward_u8_overlay(pb, 1, pb + ext, mem.stream)
    assert e.fifo_len() == 2
    fresh = fresh_engine()
    with pytest.raises(error_type, match="not finalized"):
        fresh.set_output_overlay(pal)
    fresh.close()
    e.close()
