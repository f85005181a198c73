"""Source views on the host (no library): the oracle dataloader.view_to_rgb_u8 pinned by hand on a 3 x 4 frame per format, NV12 at each origin
parity, view_extent, and pack_view's round trip with its padding and x bytes."""
import numpy as np
import pytest

import view_cases as cases
from tdnet_amd.dataloader import (PIX_BGR24, PIX_BGRA32, PIX_NV12, PIX_RGB24, PIX_RGBA32, SourceView, nv12_to_rgb_u8, pack_view, view_extent,
                                  view_to_rgb_u8)


def _px(y, x):
    """The frame's pixel (y, x): r, g, b = 10 y + x, 100 + 10 y + x, 200 + 10 y + x."""
    return [10 * y + x, 100 + 10 * y + x, 200 + 10 * y + x]


def test_packed_formats_pinned_by_hand_on_a_3x4_frame():
    # RGB24, pitch 14 (2 bytes of padding, 0xEE): rows written out byte by byte
    rows = [[v for x in range(4) for v in _px(y, x)] + [0xEE, 0xEE] for y in range(3)]
    buf = np.array(sum(rows, [])[:2 * 14 + 12], np.uint8)
    v = SourceView(PIX_RGB24, 3, 4, pitch=14, crop=(1, 1, 2, 2))
    assert view_extent(v) == 2 * 14 + 12 == buf.size
    assert view_to_rgb_u8(buf, v).tolist() == [[_px(1, 1), _px(1, 2)], [_px(2, 1), _px(2, 2)]]
    assert view_to_rgb_u8(buf, SourceView(PIX_RGB24, 3, 4, pitch=14)).tolist() == [[_px(y, x) for x in range(4)] for y in range(3)]
    # BGR24, tight: b g r
    buf = np.array([c for y in range(3) for x in range(4) for c in _px(y, x)[::-1]], np.uint8)
    v = SourceView(PIX_BGR24, 3, 4, crop=(0, 2, 3, 1))
    assert view_extent(v) == 36
    assert view_to_rgb_u8(buf, v).tolist() == [[_px(0, 2)], [_px(1, 2)], [_px(2, 2)]]
    # RGBA32, pitch 17: r g b x, x = 0x77 never shows
    rows = [[c for x in range(4) for c in _px(y, x) + [0x77]] + [0xEE] for y in range(3)]
    buf = np.array(sum(rows, [])[:2 * 17 + 16], np.uint8)
    v = SourceView(PIX_RGBA32, 3, 4, pitch=17, crop=(2, 3, 1, 1))
    assert view_extent(v) == 2 * 17 + 16
    assert view_to_rgb_u8(buf, v).tolist() == [[_px(2, 3)]]
    # BGRA32, tight: b g r x
    buf = np.array([c for y in range(3) for x in range(4) for c in _px(y, x)[::-1] + [0x77]], np.uint8)
    v = SourceView(PIX_BGRA32, 3, 4, crop=(1, 0, 2, 3))
    assert view_extent(v) == 48
    assert view_to_rgb_u8(buf, v).tolist() == [[_px(y, x) for x in range(3)] for y in (1, 2)]
    assert view_to_rgb_u8(buf, SourceView(PIX_BGRA32, 3, 4, crop=(0, 0, 0, 0))).shape == (3, 4, 3)   # all four zero: the whole frame


def test_nv12_chroma_goes_by_the_frames_coordinates_at_every_origin_parity():
    """3 x 4 surface, pitch 6, one row of gap: Y = 16 + 20 (4 y + x); chroma pairs chosen so that the four 2 x 2 blocks differ.  With standard 2
    (BT.601 full: yoff 0, CY = 2^20) and U = V = 128 a pixel is (Y, Y, Y); the pair (128, 228) adds rint(1.402 * 100) = 140 to R."""
    pitch, uv = 6, 4 * 6
    s = np.full(uv + 1 * pitch + 4, 0xEE, np.uint8)
    for y in range(3):
        s[y * pitch:y * pitch + 4] = [16 + 20 * (4 * y + x) for x in range(4)]
    s[uv:uv + 4] = [128, 128, 128, 228]                                # chroma row 0: block (0, 0) grey, block (0, 1) red-shifted
    s[uv + pitch:uv + pitch + 4] = [128, 228, 128, 128]                # chroma row 1: block (1, 0) red-shifted, block (1, 1) grey
    whole = nv12_to_rgb_u8(s, 3, 4, pitch, uv, 2)

    def want(y, x):
        Y = 16 + 20 * (4 * y + x)
        red = (y >> 1, x >> 1) in ((0, 1), (1, 0))
        # V - 128 = 100: R += (1470104 * 100 + 2^19) >> 20 = 140 (clamped), G += (-748826 * 100) >> 20 -> -71.4: computed below in integers
        if not red:
            return [Y, Y, Y]
        yy = Y * 1048576 + (1 << 19)
        return [min(255, max(0, (yy + 1470104 * 100) >> 20)), min(255, max(0, (yy - 748826 * 100) >> 20)), Y]
    assert whole.tolist() == [[want(y, x) for x in range(4)] for y in range(3)]
    for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1), (1, 2), (2, 3)):
        h, w = 3 - oy, 4 - ox
        v = SourceView(PIX_NV12, 3, 4, pitch=pitch, crop=(oy, ox, h, w), standard=2, uv_offset=uv)
        assert view_extent(v) == s.size
        got = view_to_rgb_u8(s, v)
        assert got.tolist() == [[want(oy + y, ox + x) for x in range(w)] for y in range(h)], (oy, ox)
    # the pixel (1, 1) of the rectangle at (1, 1) is frame pixel (2, 2): block (1, 1), grey -- NOT the rectangle's own block (0, 0)
    v = SourceView(PIX_NV12, 3, 4, pitch=pitch, crop=(1, 1, 2, 3), standard=2, uv_offset=uv)
    assert view_to_rgb_u8(s, v)[1, 1].tolist() == [16 + 20 * 10] * 3 and view_to_rgb_u8(s, v)[0, 0].tolist() == want(1, 1)
    tight = SourceView(PIX_NV12, 3, 5)
    assert tight.row_pitch == 6 and tight.uv == 18 and view_extent(tight) == 18 + 6 + 6


@pytest.mark.parametrize("fmt", cases.PACKED, ids=[cases.NAMES[f] for f in cases.PACKED])
def test_pack_view_round_trips_and_fills_padding_and_x_bytes(fmt):
    f = cases.frame_rgb(*cases.FRAME)
    for tight in (True, False):
        v = cases.packed_view(fmt, (3, 7, 41, 83), tight=tight)
        whole = SourceView(fmt, v.height, v.width, pitch=v.pitch)
        a, b = pack_view(f, v, 0x00), pack_view(f, v, 0xFF)
        assert a.size == view_extent(v) == (v.height - 1) * v.row_pitch + v.width * v.bpp
        assert np.array_equal(view_to_rgb_u8(a, whole), f) and np.array_equal(view_to_rgb_u8(b, whole), f)
        assert np.array_equal(view_to_rgb_u8(a, v), f[3:44, 7:90]) and view_to_rgb_u8(a, v).flags["C_CONTIGUOUS"]
        differ = int((a != b).sum())                                   # exactly the padding and the x bytes
        pad = (v.row_pitch - v.width * v.bpp) * (v.height - 1)
        assert differ == pad + (v.height * v.width if v.bpp == 4 else 0), (fmt, tight)
    # the colour order: the first pixel's first byte is r or b
    one = pack_view(f, cases.packed_view(fmt, None, tight=True))
    assert one[0] == (f[0, 0, 2] if fmt in (PIX_BGR24, PIX_BGRA32) else f[0, 0, 0])


def test_the_cases_poison_reaches_everything_outside_the_rectangle():
    for view in (cases.packed_view(PIX_BGRA32, (3, 7, 41, 83)), cases.nv12_view((3, 7, 41, 83), 1)):
        a, b = cases.view_bytes(view, 0x00, 0, outside=0x00), cases.view_bytes(view, 0xFF, 0, outside=0xFF)
        assert np.array_equal(view_to_rgb_u8(a, view), view_to_rgb_u8(b, view))
        n_in = 41 * 83 * 3 if not view.nv12 else 41 * 83 + 2 * 21 * 42   # the rectangle's colour bytes; NV12: its Y bytes and the 21 x 42 pairs covering it
        assert int((a == b).sum()) >= n_in and int((a != b).sum()) > a.size - n_in - a.size // 100
