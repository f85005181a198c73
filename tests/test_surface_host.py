"""The host oracles of "surfaces" (include/tdnet.h): dataloader.surface_to_rgb_u8 and dataloader.write_surface pinned by hand-derived values, by
cross-identities with the oracles that predate them (nv12_to_rgb_u8, write_view) on the same samples, and by poison invariance.  CPU, no library."""
import numpy as np
import pytest

import surface_cases as cases
from tdnet_amd.dataloader import (PIX_NV12, SURF_DST, SURF_I420, SURF_NV12, SURF_NV21, SURF_P010, SURF_UYVY, SURF_YUY2, SourceView, Surface, nv12_to_rgb_u8,
                                  pack_surface, surface_extent, surface_from_samples, surface_sample_index, surface_to_rgb_u8, view_extent, write_surface,
                                  write_view)

# (standard, (Y, U, V)) -> (R, G, B), worked out by hand from the header's integer constants: black, white and one saturated primary per standard
PINS_8 = {0: [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (254, 0, 0))],
          1: [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((63, 102, 240), (255, 1, 0))],
          2: [((0, 128, 128), (0, 0, 0)), ((255, 128, 128), (255, 255, 255)), ((76, 85, 255), (254, 0, 0))],
          3: [((0, 128, 128), (0, 0, 0)), ((255, 128, 128), (255, 255, 255)), ((54, 99, 255), (254, 0, 0))]}
# the same for 10-bit samples, K = rint(c * 2^18): BT.709 limited is CY 305136, CUB 553648, CUG -55837, CVG -139723, CVR 470024
PINS_10 = {0: [((64, 512, 512), (0, 0, 0)), ((940, 512, 512), (255, 255, 255)), ((324, 360, 960), (254, 0, 0))],
           1: [((64, 512, 512), (0, 0, 0)), ((940, 512, 512), (255, 255, 255)), ((252, 408, 960), (255, 1, 0))],
           2: [((0, 512, 512), (0, 0, 0)), ((1023, 512, 512), (255, 255, 255)), ((304, 340, 1020), (254, 0, 0))],
           3: [((0, 512, 512), (0, 0, 0)), ((1023, 512, 512), (255, 255, 255)), ((216, 396, 1020), (254, 0, 0))]}


def one_pixel(layout, yuv, standard, low=0):
    s = Surface(layout, 1, 1, standard=standard)
    Y, U, V = (np.array([[v]]) for v in yuv)
    return surface_to_rgb_u8(surface_from_samples(Y, U, V, s, 0x5A, low), s)[0, 0]


@pytest.mark.parametrize("standard", [0, 1, 2, 3])
def test_conversion_in_is_pinned_by_hand(standard):
    for layout in (SURF_NV12, SURF_NV21, SURF_I420, SURF_YUY2, SURF_UYVY):
        for yuv, rgb in PINS_8[standard]:
            assert tuple(one_pixel(layout, yuv, standard)) == rgb, (layout, yuv)
    for yuv, rgb in PINS_10[standard]:
        for low in (0, 63):                                            # the low 6 bits of every word are ignored
            assert tuple(one_pixel(SURF_P010, yuv, standard, low)) == rgb, (yuv, low)


def test_p010_rounds_once_from_ten_bits():
    """BT.709 limited grey: Y10 = 527 gives ((527 - 64) * 305136 + 2^19) >> 20 = 135; truncated to the byte 131 first it would be
    ((131 - 16) * 1220542 + 2^19) >> 20 = 134."""
    assert tuple(one_pixel(SURF_P010, (527, 512, 512), 1)) == (135, 135, 135)
    assert tuple(one_pixel(SURF_NV12, (131, 128, 128), 1)) == (134, 134, 134)


def test_sample_addresses_word_packing_and_byte_order():
    """A 2 x 4 frame by the header's table: where each sample's byte lies, P010's little-endian word, the 4:2:2 byte order."""
    Y = np.array([[1, 2, 3, 4], [5, 6, 7, 8]])
    U, V = np.array([[10, 11]]), np.array([[20, 21]])
    assert surface_from_samples(Y, U, V, Surface(SURF_NV12, 2, 4), 0).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 10, 20, 11, 21]
    assert surface_from_samples(Y, U, V, Surface(SURF_NV21, 2, 4), 0).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 20, 10, 21, 11]
    assert surface_from_samples(Y, U, V, Surface(SURF_I420, 2, 4), 0).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 20, 21]
    yv12 = Surface(SURF_I420, 2, 4, u_offset=10, v_offset=8)           # YV12: the two chroma offsets exchanged
    assert surface_from_samples(Y, U, V, yv12, 0).tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 20, 21, 10, 11]
    U2, V2 = np.array([[10, 11], [12, 13]]), np.array([[20, 21], [22, 23]])
    assert surface_from_samples(Y, U2, V2, Surface(SURF_YUY2, 2, 4), 0).tolist() == [1, 10, 2, 20, 3, 11, 4, 21, 5, 12, 6, 22, 7, 13, 8, 23]
    assert surface_from_samples(Y, U2, V2, Surface(SURF_UYVY, 2, 4), 0).tolist() == [10, 1, 20, 2, 11, 3, 21, 4, 12, 5, 22, 6, 13, 7, 23, 8]
    # P010: value << 6 | low bits, low byte first: 0x3FF -> 0xFFC0 (+ 0x3F), 1 -> 0x0040
    p = surface_from_samples(np.array([[1023, 1]]), np.array([[512]]), np.array([[2]]), Surface(SURF_P010, 1, 2), 0, 0x3F)
    assert p.tolist() == [0xFF, 0xFF, 0x7F, 0x00, 0x3F, 0x80, 0xBF, 0x00]
    # an odd width: 4:2:2 rows hold whole pairs, the chroma planes ceil(width / 2) samples
    assert Surface(SURF_YUY2, 3, 5).luma_row_bytes == 12 and surface_extent(Surface(SURF_YUY2, 3, 5)) == 36
    assert surface_extent(Surface(SURF_I420, 3, 5)) == 15 + 2 * 2 * 3 and Surface(SURF_I420, 3, 5).cpitch == 3
    assert surface_extent(Surface(SURF_P010, 3, 5)) == 30 + 10 + 12 and surface_extent(Surface(SURF_NV12, 3, 5)) == 15 + 5 + 6
    # a pitched NV12 surface with a chroma pitch of its own: the extent is the chroma plane's end
    s = Surface(SURF_NV12, 3, 5, pitch=8, chroma_pitch=7, u_offset=40)
    assert surface_extent(s) == 40 + 7 + 6 and surface_sample_index(s)[2][1, 2] == 40 + 7 + 4 + 1


@pytest.mark.parametrize("layout", cases.LAYOUTS, ids=[cases.NAMES[l] for l in cases.LAYOUTS])
def test_an_odd_origin_shifts_the_chroma_phase(layout):
    """The rectangle is a slice of the whole frame's conversion: pixel (y, x) of a rectangle at (oy, ox) takes chroma sample ((oy + y) >> 1, (ox + x) >> 1)
    -- 4:2:2: (oy + y, (ox + x) >> 1) -- checked sample by sample against a scalar restatement for every phase."""
    whole = cases.surface(layout, None, "padded", standard=1)
    b = cases.surface_bytes(whole, 0x11, 4)
    full = surface_to_rgb_u8(b, whole)
    Y, U, V = cases.samples(layout, *cases.FRAME, 4)
    for name, rect, _ in cases.RECTS:
        s = cases.surface(layout, rect, "padded", standard=1)
        got = surface_to_rgb_u8(b, s)
        oy, ox, h, w = rect
        assert np.array_equal(got, full[oy:oy + h, ox:ox + w]), name
        for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w // 3)):
            cy = oy + y if s.packed422 else (oy + y) >> 1
            lone = Surface(layout, 1, 1, standard=1)
            one = surface_to_rgb_u8(surface_from_samples(Y[oy + y:oy + y + 1, ox + x:ox + x + 1], U[cy:cy + 1, (ox + x) >> 1:((ox + x) >> 1) + 1],
                                                         V[cy:cy + 1, (ox + x) >> 1:((ox + x) >> 1) + 1], lone, 0), lone)[0, 0]
            assert np.array_equal(got[y, x], one), (name, y, x)


@pytest.mark.parametrize("variant", ["tight", "padded"])
def test_nv12_surface_is_the_nv12_oracle_and_the_other_layouts_are_nv12_rearranged(variant):
    Hf, Wf = cases.FRAME
    Y, U, V = cases.samples(SURF_NV12, Hf, Wf, 0)
    for standard in range(4):
        nv = cases.surface(SURF_NV12, None, variant, standard=standard)
        b = surface_from_samples(Y, U, V, nv, 0)
        want = surface_to_rgb_u8(b, nv)
        if variant == "tight":                                         # one pitch for both planes: the surface nv12_to_rgb_u8 reads
            assert np.array_equal(want, nv12_to_rgb_u8(b, Hf, Wf, nv.row_pitch, nv.u_off, standard))
        for layout in (SURF_NV21, SURF_I420):                          # the same samples swapped / de-interleaved
            for v2 in cases.variants(layout):
                s = cases.surface(layout, None, v2, standard=standard)
                assert np.array_equal(surface_to_rgb_u8(surface_from_samples(Y, U, V, s, 0xC3), s), want), (layout, v2)
        for layout in (SURF_YUY2, SURF_UYVY):                          # 4:2:2 with every chroma row given twice is the 4:2:0 picture
            s = cases.surface(layout, None, variant, standard=standard)
            rows = np.arange(Hf) >> 1
            assert np.array_equal(surface_to_rgb_u8(surface_from_samples(Y, U[rows], V[rows], s, 0), s), want), layout
    grey = np.full((2, 2), 128)                                        # 10-bit samples 4 v: black and white at the mid-point agree with the bytes v
    for y8 in (16, 235):
        a = surface_to_rgb_u8(surface_from_samples(np.full((2, 2), y8), grey[:1, :1], grey[:1, :1], Surface(SURF_NV12, 2, 2), 0), Surface(SURF_NV12, 2, 2))
        b = surface_to_rgb_u8(surface_from_samples(np.full((2, 2), 4 * y8), 4 * grey[:1, :1], 4 * grey[:1, :1], Surface(SURF_P010, 2, 2), 0), Surface(SURF_P010, 2, 2))
        assert np.array_equal(a, b)


@pytest.mark.parametrize("layout", cases.LAYOUTS, ids=[cases.NAMES[l] for l in cases.LAYOUTS])
def test_the_input_oracle_ignores_every_byte_that_is_no_covering_sample(layout):
    for variant in cases.variants(layout):
        for name, rect, _ in cases.RECTS:
            s = cases.surface(layout, rect, variant)
            want = surface_to_rgb_u8(cases.surface_bytes(s, 0, 0), s)
            for fill in (0x00, 0xFF):
                assert np.array_equal(surface_to_rgb_u8(cases.surface_bytes(s, fill, 0, poison=True), s), want), (variant, name, fill)
            assert cases.covering(s).sum() < surface_extent(s) or rect[2:] == cases.FRAME


# ---- conversion out -------------------------------------------------------------------------------------------------------------------------
def test_write_surface_p010_is_pinned_by_hand():
    """BT.709 limited, K = rint(c * 2^20): white -> 940 / 511 / 512 (BT.601 limited: 940 / 512 / 512); black -> 64 / 512 / 512; a lone red pixel (n = 1, m = 4):
    Y10 = (191889 * 255 + (16 << 20) + 2^17) >> 18 = 251, U10 = (4 * -105906 * 255 + (128 << 22) + 2^19) >> 20 = 409, V10 = (4 * 460325 * 255 + ...) >> 20 = 960.
    The words are value << 6, little-endian, the low bits zero."""
    s = Surface(SURF_P010, 2, 2, standard=1)
    li, ui, vi = surface_sample_index(s)

    def words(pic):
        b = write_surface(np.full(surface_extent(s), 0xFF, np.uint8), s, pic).astype(np.int64)
        return [int(b[i] | (b[i + 1] << 8)) for i in (li[0, 0], ui[0, 0], vi[0, 0])]

    # white: the U row of the BT.709 limited decimals sums to -0.001, so U10 = (1020 * -1049 + (128 << 22) + 2^19) >> 20 = 511 (the byte form rounds the same
    # -0.26 away: 128); BT.601 limited, whose rows sum to 0, gives 940 / 512 / 512
    assert words(np.full((2, 2, 3), 255, np.uint8)) == [940 << 6, 511 << 6, 512 << 6]
    s0 = Surface(SURF_P010, 2, 2, standard=0)
    b0 = write_surface(np.zeros(surface_extent(s0), np.uint8), s0, np.full((2, 2, 3), 255, np.uint8)).astype(np.int64)
    assert [int(b0[i] | (b0[i + 1] << 8)) for i in (li[0, 0], ui[0, 0], vi[0, 0])] == [940 << 6, 512 << 6, 512 << 6]
    assert words(np.zeros((2, 2, 3), np.uint8)) == [64 << 6, 512 << 6, 512 << 6]
    one = Surface(SURF_P010, 1, 1, standard=1)
    b = write_surface(np.full(surface_extent(one), 0xFF, np.uint8), one, np.array([[[255, 0, 0]]], np.uint8)).astype(np.int64)
    assert [int(b[i] | (b[i + 1] << 8)) for i in (0, 2, 4)] == [251 << 6, 409 << 6, 960 << 6]
    full = Surface(SURF_P010, 1, 1, standard=3)                        # BT.709 full: white is 1020 (255 * 4: the 8-bit picture's range), never above 1023
    b = write_surface(np.zeros(surface_extent(full), np.uint8), full, np.full((1, 1, 3), 255, np.uint8)).astype(np.int64)
    assert int(b[0] | (b[1] << 8)) == 1020 << 6


@pytest.mark.parametrize("standard", [0, 1, 2, 3])
def test_write_surface_nv12_is_write_view_and_the_other_layouts_rearrange_it(standard):
    frame, rect = cases.dst_rect("corner_odd")
    Hf, Wf = frame
    pic = np.random.default_rng(5 + standard).integers(0, 256, rect[2:] + (3,), dtype=np.uint8)
    nv = Surface(SURF_NV12, Hf, Wf, pitch=112, crop=rect, standard=standard, u_offset=(Hf + 2) * 112)
    view = SourceView(PIX_NV12, Hf, Wf, pitch=112, crop=rect, standard=standard, uv_offset=(Hf + 2) * 112)
    assert surface_extent(nv) == view_extent(view)
    prefill = np.full(surface_extent(nv), 0x3C, np.uint8)
    want = write_surface(prefill, nv, pic)
    assert np.array_equal(want, write_view(prefill, view, pic))
    li, ui, vi = surface_sample_index(nv)
    for layout in (SURF_NV21, SURF_I420):
        for variant in cases.variants(layout):
            s = cases.surface(layout, rect, variant, frame=frame, standard=standard)
            got = write_surface(np.full(surface_extent(s), 0x3C, np.uint8), s, pic)
            for a, b_ in zip(surface_sample_index(s), (li, ui, vi)):
                assert np.array_equal(got[a], want[b_]), (layout, variant)   # the same samples (0x3C where the picture does not reach), placed elsewhere
            assert got.size == surface_extent(s)


@pytest.mark.parametrize("layout", SURF_DST, ids=[cases.NAMES[l] for l in SURF_DST])
def test_the_output_oracle_writes_only_the_rectangles_samples(layout):
    for case in cases.DST_CASES:
        frame, rect = cases.dst_rect(case)
        pic = np.random.default_rng(9).integers(0, 256, rect[2:] + (3,), dtype=np.uint8)
        for variant in cases.variants(layout):
            s = cases.surface(layout, rect, variant, frame=frame, standard=1)
            n = surface_extent(s)
            a, b = write_surface(np.zeros(n, np.uint8), s, pic), write_surface(np.full(n, 255, np.uint8), s, pic)
            decided = a == b                                           # the bytes the picture decides: exactly the covering samples
            assert np.array_equal(decided, cases.covering(s)), (case, variant)
            assert (a[~decided] == 0).all() and (b[~decided] == 255).all()
            back = surface_to_rgb_u8(a, s).astype(np.int64)            # the round trip stays near the picture's luma: a coarse sanity bound, not the definition
            assert np.abs(back.sum(axis=2) - pic.astype(np.int64).sum(axis=2)).mean() < 3 * 48


def test_pack_surface_is_a_function_of_the_frame_in_every_layout():
    rgb = np.random.default_rng(2).integers(0, 256, cases.FRAME + (3,), dtype=np.uint8)
    for layout in cases.LAYOUTS:
        s = cases.surface(layout, None, "padded")
        a, b = pack_surface(rgb, s, 0x00), pack_surface(rgb, s, 0xFF)
        assert a.size == surface_extent(s) and np.array_equal(surface_to_rgb_u8(a, s), surface_to_rgb_u8(b, s))
        flat = np.full(cases.FRAME + (3,), 77, np.uint8)                # a grey frame comes back grey, within the two roundings
        back = surface_to_rgb_u8(pack_surface(flat, s), s).astype(np.int64)
        assert np.abs(back - 77).max() <= 2, layout


def test_descriptions_reject_what_they_cannot_derive_from():
    with pytest.raises(ValueError):
        Surface(6, 4, 4)
    with pytest.raises(ValueError):
        Surface(SURF_NV12, 4, 4, crop=(0, 0, 4))
    with pytest.raises(AssertionError):
        write_surface(np.zeros(64, np.uint8), Surface(SURF_YUY2, 4, 4), np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(AssertionError):
        write_surface(np.zeros(64, np.uint8), Surface(SURF_NV12, 4, 4, crop=(1, 0, 2, 2)), np.zeros((2, 2, 3), np.uint8))
    assert Surface("p010", 4, 4).layout == SURF_P010
