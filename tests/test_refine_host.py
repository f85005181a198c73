"""The refined matte's definition (include/tdnet.h "refined matte", dataloader.refine_matte_u8), on the host: the integer restatement IS a guided filter.

It differs from He et al.'s filter in float64 -- the means over the same clipped windows, a = cov / (var + eps), b = mean_M - a mean_G,
rint(mean_a G + mean_b) -- by AT MOST 1 BYTE.  The bound is derived, not measured: Q10 of a costs <= 255 / 2048 of a byte (half a step of 1 / 1024 times
G <= 255), Q6 of b <= 1 / 128, the fp32 roundings < 1e-3, and the two final roundings 1 / 2 each: below 1.14 in all, so the integers differ by at most 1.
The condition, asserted here, is that no a_q was clamped.  The three exact properties and hand-computed small maps are pinned with ==."""
import numpy as np
import pytest

import refine_cases as cases
from tdnet_amd.dataloader import luma_u8, refine_matte_u8


@pytest.mark.parametrize("size", cases.HOST_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_the_integer_definition_is_within_one_byte_of_the_float64_guided_filter(kind, size):
    h, w = size
    worst, amax = 0, 0.0
    for r in cases.RADII:
        for eps in cases.EPSS:
            G, M, out, aq, bq = cases.want(kind, h, w, r, eps)
            ref, a = cases.textbook_f64(G, M, r, eps)
            assert np.abs(aq.astype(np.int64)).max() < 32767, (kind, size, r, eps)   # the condition of the bound: no clamp
            d = int(np.abs(out.astype(np.int64) - ref).max())
            assert d <= 1, (kind, size, r, eps, d)
            worst, amax = max(worst, d), max(amax, a)
            if kind == "const_matte":
                assert np.array_equal(out, M), (size, r, eps)          # exact: cov = 0 and 1024 N c is representable
                assert (aq == 0).all() and (bq == 64 * M.astype(np.int32)).all()
            if kind == "all255":
                assert (out == 255).all(), (size, r, eps)              # the overflow witness of S_GG
    print("refine host %s %dx%d: max difference %d, max |a| %.2f" % (kind, h, w, worst, amax))
    assert amax < 32.0                                                 # |a| <= sigma_M / (2 sqrt(eps)) with eps >= 4


def test_a_one_pixel_map_and_a_row_of_three_by_hand():
    # 1 x 1: N = 1, the window is the pixel: cov = G M - G M = 0, den = eps > 0, a_q = 0, b_q = rint(1024 M / 16) = 64 M, out = rint(16 * 64 M / 1024) = M
    for g, m in ((0, 0), (255, 255), (17, 200), (200, 17)):
        out, aq, bq = refine_matte_u8(np.array([[g]], np.uint8), np.array([[m]], np.uint8), 16, 4, want_coeff=True)
        assert out[0, 0] == m and aq[0, 0] == 0 and bq[0, 0] == 64 * m
    # 1 x 3, r = 1, eps = 4, G = M = (0, 0, 255): windows {0, 1}, {0, 1, 2}, {1, 2}
    #   x = 0: N = 2, all sums 0: a_q = 0, b_q = 0
    #   x = 1: N = 3, S_G = S_M = 255, S_GG = S_GM = 65025: cov = 3 * 65025 - 65025 = 130050, den = 130050 + 4 * 9 = 130086
    #          a = 0.99972326..., a_q = rint(1023.7166) = 1024, b_q = rint((1024 * 255 - 1024 * 255) / 48) = 0
    #   x = 2: N = 2, S = 255, S_GG = 65025: cov = 2 * 65025 - 65025 = 65025, den = 65025 + 16 = 65041, a = 0.999754, a_q = rint(1023.748) = 1024, b_q = 0
    #   stage 2: A = (1024, 2048, 2048), B = 0: out = rint(A G / (1024 N)) = (0, 0, rint(2048 * 255 / 2048)) = (0, 0, 255)
    G = np.array([[0, 0, 255]], np.uint8)
    out, aq, bq = refine_matte_u8(G, G, 1, 4, want_coeff=True)
    assert aq.tolist() == [[0, 1024, 1024]] and bq.tolist() == [[0, 0, 0]] and out.tolist() == [[0, 0, 255]]
    # the same matte over a FLAT guide: a = 0 everywhere, b_q = 64 mean_M, and the output is the box mean of the box mean
    #   b_q = (rint(0), rint(1024 * 255 / 48) = 5440, rint(1024 * 255 / 32) = 8160);  B = (5440, 13600, 13600)
    #   out = rint(16 B / (1024 N)) = (rint(42.5) = 42, rint(70.83) = 71, rint(106.25) = 106)          -- 42.5 rounds to even
    out, aq, bq = refine_matte_u8(np.full((1, 3), 90, np.uint8), G, 1, 4, want_coeff=True)
    assert aq.tolist() == [[0, 0, 0]] and bq.tolist() == [[0, 5440, 8160]] and out.tolist() == [[42, 71, 106]]


def test_the_result_keeps_an_edge_the_guide_has_and_smooths_where_it_has_none():
    """What the filter is for: a soft matte ramp over a sharp guide edge comes back sharper; over a flat guide it is just blurred."""
    G, M = cases.inputs("ramp", 41, 83)
    sharp = refine_matte_u8(G, M, 8, 65).astype(np.int64)
    flat = refine_matte_u8(np.full_like(G, 100), M, 8, 65).astype(np.int64)
    row = 20
    jump = lambda o: int(o[row, 83 // 2]) - int(o[row, 83 // 2 - 1])   # across the guide's edge
    step = jump(M)                                                     # the ramp's own slope: 16 a pixel
    assert step == 16
    assert jump(flat) <= step + 1                                      # a mean of means of a ramp is no steeper than the ramp
    assert jump(sharp) > 2 * step                                      # the guide's edge is put back into the matte


def test_luma_of_black_white_and_the_primaries():
    px = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [90, 90, 90]], np.uint8)
    # (77 * 255 + 128) >> 8 = 19763 >> 8 = 77;  (150 * 255 + 128) >> 8 = 38378 >> 8 = 149;  (29 * 255 + 128) >> 8 = 7523 >> 8 = 29
    assert luma_u8(px).tolist() == [0, 255, 77, 149, 29, 90]
    assert luma_u8(px.reshape(2, 3, 3)).shape == (2, 3)


def test_the_oracle_refuses_what_the_library_refuses():
    G = np.zeros((3, 3), np.uint8)
    for r, eps in ((0, 65), (17, 65), (4, 3), (4, 65026)):
        with pytest.raises(AssertionError):
            refine_matte_u8(G, G, r, eps)
    with pytest.raises(AssertionError):
        refine_matte_u8(G, np.zeros((3, 4), np.uint8), 4, 65)
