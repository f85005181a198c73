"""The host oracles of the destination views (include/tdnet.h "destination views") pinned by hand, on the CPU, without the library:
dataloader.nv12_from_rgb_u8 -- the integer definition of the NV12 destination -- and dataloader.write_view, which pastes a picture into a frame's bytes
in any of the five formats.  tests/dst_view_cases.py measures the kernels against these two."""
import numpy as np
import pytest

from tdnet_amd.dataloader import (PIX_BGR24, PIX_BGRA32, PIX_NV12, PIX_RGB24, PIX_RGBA32, SourceView, nv12_forward_coeffs, nv12_from_rgb_u8, view_extent, write_view)

STANDARDS = (0, 1, 2, 3)


def one(colour, standard):
    """(Y, U, V) of a 1 x 1 picture."""
    Y, UV = nv12_from_rgb_u8(np.array([[colour]], np.uint8), standard, planes=True)
    return int(Y[0, 0]), int(UV[0, 0, 0]), int(UV[0, 0, 1])


@pytest.mark.parametrize("standard", STANDARDS)
def test_grey_has_neutral_chroma_and_white_and_black_sit_on_the_range_ends(standard):
    """A grey level g gives m K S = 4 g * (the rounded chroma row's sum).  The decimals of every chroma row sum to 0 -- the rounded row to 0 +- 1 --
    except BT709 limited's U row, whose three-decimal coefficients sum to -.001: -1048 after rounding.  Either way 4 * 255 * 1048 = 1068960 is below
    the rounding term 2^21 = 2097152 on both sides of it: ((128 << 22) + (1 << 21) +- 1068960) >> 22 = 128 for every grey level.  The Y row sums to
    0.859 (limited) or 1.0 (full) +- 1.5 ulp: white = 16 + 219.045 -> 235 (255 * 0.859 = 219.045, + 0.5 rounds down) or 255, black = the offset."""
    yoff, K = nv12_forward_coeffs(standard)
    sums = [abs(int(K[1].sum())), abs(int(K[2].sum()))]
    assert sums == ([1048, 0] if standard == 1 else sums) and max(sums) <= (1048 if standard == 1 else 1) and 4 * 255 * max(sums) < 1 << 21
    for g in range(256):
        y, u, v = one((g, g, g), standard)
        assert (u, v) == (128, 128), (g, u, v)
    assert one((255, 255, 255), standard)[0] == (235 if standard < 2 else 255)
    assert one((0, 0, 0), standard)[0] == (16 if standard < 2 else 0)
    assert yoff == (16 if standard < 2 else 0)


def test_one_saturated_colour_per_standard_worked_by_hand():
    """A 1 x 1 picture: n = 1, m = 4.  2^20 = 1048576, 2^22 = 4194304, (128 << 22) + (1 << 21) = 538968064, (16 << 20) + (1 << 19) = 17301504.
    BT601 limited, red (255, 0, 0):  KYR = rint(.257 * 2^20) = 269484;  Y = (255 * 269484 + 17301504) >> 20 = 86019924 >> 20 = 82
        KUR = rint(-.148 * 2^20) = -155189;  U = (4 * 255 * -155189 + 538968064) >> 22 = 380675284 >> 22 = 90
        KVR = rint(.439 * 2^20) = 460325;    V = (4 * 255 * 460325 + 538968064) >> 22 = 1008499564 >> 22 = 240
    BT709 limited, green (0, 255, 0):  KYG = rint(.614 * 2^20) = 643826;  Y = (255 * 643826 + 17301504) >> 20 = 181477134 >> 20 = 173
        KUG = rint(-.339 * 2^20) = -355467;  U = (4 * 255 * -355467 + 538968064) >> 22 = 176391724 >> 22 = 42
        KVG = rint(-.399 * 2^20) = -418382;  V = (4 * 255 * -418382 + 538968064) >> 22 = 112218424 >> 22 = 26
    BT601 full, blue (0, 0, 255):  KYB = rint(.114 * 2^20) = 119538;  Y = (255 * 119538 + 524288) >> 20 = 31006478 >> 20 = 29
        KUB = .5 * 2^20 = 524288;  U = (4 * 255 * 524288 + 538968064) >> 22 = 2^30 >> 22 = 256 -> clamped to 255
        KVB = rint(-.081312 * 2^20) = -85262;  V = (4 * 255 * -85262 + 538968064) >> 22 = 452000824 >> 22 = 107
    BT709 full, yellow (255, 255, 0):  KYR + KYG = 222927 + 749942 = 972869;  Y = (255 * 972869 + 524288) >> 20 = 248605883 >> 20 = 237
        KUR + KUG = -120137 - 404151 = -524288;  U = (4 * 255 * -524288 + 538968064) >> 22 = 4194304 >> 22 = 1
        KVR + KVG = 524288 - 476214 = 48074;     V = (4 * 255 * 48074 + 538968064) >> 22 = 588003544 >> 22 = 140"""
    assert one((255, 0, 0), 0) == (82, 90, 240)
    assert one((0, 255, 0), 1) == (173, 42, 26)
    assert one((0, 0, 255), 2) == (29, 255, 107)
    assert one((255, 255, 0), 3) == (237, 1, 140)


def test_blocks_of_one_two_and_four_pixels_at_an_odd_edge():
    """A 3 x 3 picture has the pairs (0, 0) of n = 4, (0, 1) and (1, 0) of n = 2, (1, 1) of n = 1.  Uniform red: m S = 4 * 255 in every pair, so every
    pair is the 1 x 1 answer (90, 240).  Red beside black in a pair of two (the top right block: column 2 of rows 0, 1): S_R = 255, m = 2:
        U = (2 * 255 * -155189 + 538968064) >> 22 = 459821674 >> 22 = 109;  V = (2 * 255 * 460325 + 538968064) >> 22 = 773733814 >> 22 = 184
    and in the block of four with one red pixel, S_R = 255, m = 1:
        U = (255 * -155189 + 538968064) >> 22 = 499394869 >> 22 = 119;  V = (255 * 460325 + 538968064) >> 22 = 656350939 >> 22 = 156."""
    red = np.zeros((3, 3, 3), np.uint8)
    red[..., 0] = 255
    Y, UV = nv12_from_rgb_u8(red, 0, planes=True)
    assert Y.shape == (3, 3) and UV.shape == (2, 2, 2) and (Y == 82).all() and (UV[..., 0] == 90).all() and (UV[..., 1] == 240).all()
    img = np.zeros((3, 3, 3), np.uint8)
    img[0, 2, 0] = 255                                                 # the pair of two
    img[1, 1, 0] = 255                                                 # the block of four
    img[2, 2, 0] = 255                                                 # the single pixel
    Y, UV = nv12_from_rgb_u8(img, 0, planes=True)
    assert UV[0, 1].tolist() == [109, 184] and UV[0, 0].tolist() == [119, 156] and UV[1, 1].tolist() == [90, 240] and UV[1, 0].tolist() == [128, 128]
    assert Y[0, 2] == 82 and Y[0, 0] == 16
    surf = nv12_from_rgb_u8(img, 0)                                    # the tight surface: 3 + 2 rows of 4 bytes, a zero byte behind every Y row
    assert surf.shape == (5, 4) and np.array_equal(surf[:3, :3], Y) and not surf[:3, 3].any() and np.array_equal(surf[3:].reshape(2, 2, 2), UV)


@pytest.mark.parametrize("standard", STANDARDS)
def test_every_sum_fits_int32_over_all_colours(standard):
    """n = 4, m = 1, S = 4 c for every colour c of the 2^24: the luma sum, the chroma sums and every partial sum of their three products, whatever
    the order they are added in, stay below 2^31 in magnitude."""
    yoff, K = nv12_forward_coeffs(standard)
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    worst = 0
    for r in range(256):
        c = np.stack([np.full_like(g, r), g, b], axis=-1)
        luma = c @ np.abs(K[0]) + (yoff << 20) + (1 << 19)
        chroma = (4 * c) @ np.abs(K[1:]).T + (128 << 22) + (1 << 21)   # |products| added: bounds every partial sum
        worst = max(worst, int(luma.max()), int(chroma.max()))
    assert worst < 2 ** 31, worst
    assert worst <= 1.08e9 + (128 << 22) + (1 << 21)                   # the bound the header states for the products alone


def test_write_view_packed_formats():
    pic = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) + 10   # pixel (y, x) = (10 + 9 y + 3 x, + 1, + 2)
    for fmt, bpp, order in ((PIX_RGB24, 3, (0, 1, 2)), (PIX_BGR24, 3, (2, 1, 0)), (PIX_RGBA32, 4, (0, 1, 2)), (PIX_BGRA32, 4, (2, 1, 0))):
        view = SourceView(fmt, 4, 6, pitch=6 * bpp + 3, crop=(1, 2, 2, 3))
        n = view_extent(view)
        assert n == 3 * (6 * bpp + 3) + 6 * bpp
        frame = np.full(n, 0xA5, np.uint8)
        out = write_view(frame, view, pic)
        assert (frame == 0xA5).all()                                   # a copy
        want = frame.copy()
        for y in range(2):
            for x in range(3):
                at = (1 + y) * (6 * bpp + 3) + (2 + x) * bpp
                for k in range(3):
                    want[at + k] = pic[y, x, order[k]]
                if bpp == 4:
                    want[at + 3] = 255
        assert np.array_equal(out, want), fmt
        assert int((out != frame).sum()) == 2 * 3 * bpp


def test_write_view_nv12_touches_its_y_bytes_and_the_covering_pairs_only():
    view = SourceView(PIX_NV12, 7, 9, pitch=12, crop=(2, 4, 3, 3), standard=2, uv_offset=8 * 12)
    n = view_extent(view)
    assert n == 8 * 12 + 3 * 12 + 10
    pic = np.random.default_rng(5).integers(0, 256, (3, 3, 3), dtype=np.uint8)
    Y, UV = nv12_from_rgb_u8(pic, 2, planes=True)
    frame = np.full(n, 0x5A, np.uint8)
    out = write_view(frame, view, pic)
    want = frame.copy()
    for y in range(3):
        want[(2 + y) * 12 + 4:(2 + y) * 12 + 7] = Y[y]
    for j in range(2):                                                 # chroma rows 1, 2 of the frame, pairs 2, 3: bytes 4 .. 7
        want[96 + (1 + j) * 12 + 4:96 + (1 + j) * 12 + 8] = UV[j].reshape(-1)
    assert np.array_equal(out, want)
    with pytest.raises(AssertionError, match="chroma grid"):
        write_view(frame, SourceView(PIX_NV12, 7, 9, pitch=12, crop=(1, 4, 3, 3), uv_offset=96), pic)
