"""The NV12 specification on the host (include/tdnet.h "NV12 frames in"; dataloader.nv12_to_rgb_u8 is the oracle of the device tests): pinned
by hand-derived answers, by its integer tables recomputed from the decimals, by a scalar restatement on a source that reaches both clamps, and
shown to distinguish the two mistakes a kernel is most likely to make.  No library, no device."""
import numpy as np
import pytest

import nv12_cases as cases
from tdnet_amd import dataloader as dl


def test_hand_derived_pins():
    for (Y, U, V), rgb in cases.PINS:
        s = np.array([Y, 0x77, U, V], np.uint8)                        # a 1 x 1 surface: pitch 2, one byte of padding, the UV pair at byte 2
        assert tuple(dl.nv12_to_rgb_u8(s, 1, 1, 2, 2, 0)[0, 0]) == rgb, (Y, U, V)
        assert cases.scalar_convert(Y, U, V)[0] == rgb, (Y, U, V)


@pytest.mark.parametrize("standard", [0, 1, 2, 3])
def test_integer_tables_are_the_rounded_decimals(standard):
    yoff, dec = dl.NV12_STANDARDS[standard]
    assert dec == cases.DECIMALS[standard]
    want = (16 if standard < 2 else 0,) + tuple(int(np.rint(c * 2 ** 20)) for c in cases.DECIMALS[standard])
    assert dl.nv12_coeffs(standard) == want == cases.TABLE[standard]
    # the worst sum stays inside int32
    yo, CY, CUB, CUG, CVG, CVR = want
    worst = 255 * CY + (1 << 19) + 128 * max(abs(CVR), abs(CUB), abs(CVG) + abs(CUG))
    assert worst < 2 ** 31 and worst <= 6.1e8


def test_corners_source_against_a_scalar_loop():
    name, (Hs, Ws), _ = cases.STEM_CASES[-1]
    assert name == "corners_2x250"
    Y, UV = cases.planes(name, Hs, Ws)
    got = cases.expected_rgb(name, Hs, Ws)
    below = above = 0
    for y in range(Hs):
        for x in range(Ws):
            rgb, raw = cases.scalar_convert(int(Y[y, x]), int(UV[y >> 1, x >> 1, 0]), int(UV[y >> 1, x >> 1, 1]))
            assert tuple(got[y, x]) == rgb, (y, x)
            below += sum(c < 0 for c in raw)
            above += sum(c > 255 for c in raw)
    assert below > 0 and above > 0                                     # both clamps occur
    assert len({(int(Y[0, 2 * i]), int(UV[0, i, 0]), int(UV[0, i, 1])) for i in range(125)}) == 125


@pytest.mark.parametrize("standard", [1, 2, 3])
def test_other_standards_against_the_scalar_loop(standard):
    rng = np.random.default_rng(standard)
    yuv = rng.integers(0, 256, (200, 3), dtype=np.uint8)
    got = cases.convert_pixels(yuv[:, 0], yuv[:, 1], yuv[:, 2], standard)
    for i in range(200):
        assert tuple(got[i]) == cases.scalar_convert(*(int(v) for v in yuv[i]), standard=standard)[0], i
    assert not np.array_equal(got, cases.convert_pixels(yuv[:, 0], yuv[:, 1], yuv[:, 2], 0))


def test_layout_padding_and_gap_do_not_matter():
    name, (Hs, Ws) = "down_41x83", (41, 83)
    want = cases.expected_rgb(name, Hs, Ws)
    for _, pitch, uv in cases.layouts(Hs, Ws):
        for fill in (0x00, 0xFF):
            assert np.array_equal(dl.nv12_to_rgb_u8(cases.surface(name, Hs, Ws, pitch, uv, fill), Hs, Ws, pitch, uv), want)
    # chroma is replicated: the four pixels of a block share their pair
    Y, UV = cases.planes(name, Hs, Ws)
    assert tuple(want[40, 82]) == cases.scalar_convert(int(Y[40, 82]), int(UV[20, 41, 0]), int(UV[20, 41, 1]))[0]


def test_the_cases_see_the_two_likely_mistakes():
    """case down_41x83: "interpolate YUV, then convert" and "U and V swapped" both give another image than the oracle."""
    name, (Hs, Ws), (H, W) = cases.STEM_CASES[5]
    assert name == "down_41x83"
    want = cases.resized_rgb(name, Hs, Ws, H, W)
    assert not np.array_equal(cases.resized_yuv_then_converted(name, Hs, Ws, H, W), want)
    _, pitch, uv = cases.layouts(Hs, Ws)[0]
    swapped = dl.resize_linear_u8(dl.nv12_to_rgb_u8(cases.surface(name, Hs, Ws, pitch, uv, swap_uv=True), Hs, Ws, pitch, uv), (W, H))
    assert not np.array_equal(swapped, want)
    # and at the same size the wrong order is the right one (nothing to interpolate): the difference above is the order's alone
    assert np.array_equal(cases.resized_yuv_then_converted(name, Hs, Ws, Hs, Ws), cases.expected_rgb(name, Hs, Ws))


def test_rgb_to_nv12_is_a_deterministic_generator():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (41, 83, 3), dtype=np.uint8)
    s = dl.rgb_to_nv12(img)
    assert s.dtype == np.uint8 and s.shape == (41 + 21, 256) and np.array_equal(s, dl.rgb_to_nv12(img.copy()))
    assert not s[:, 84:].any() and not s[:41, 83:].any()               # zero padding
    t = dl.rgb_to_nv12(img, pitch=84)
    assert t.shape == (62, 84) and np.array_equal(t[:, :84], s[:, :84])
    # near-inverse on a flat grey image (no chroma to lose): within one level
    grey = np.full((6, 10, 3), 100, np.uint8)
    g = dl.rgb_to_nv12(grey, pitch=10)
    back = dl.nv12_to_rgb_u8(g, 6, 10, 10, 60)
    assert np.abs(back.astype(int) - 100).max() <= 1
    # a loader item carries the surface and the picture's size
    assert dl.nv12_extent(41, 83, 256, 41 * 256) == 41 * 256 + 20 * 256 + 84 <= s.size
