"""The host oracle of regions out (tdnet_amd.dataloader.regions_u8), which tests/regions_cases.py holds the kernels to: against answers written out by
hand on 5x7 maps, and -- where scipy is installed; it is not required -- against scipy.ndimage.label per class with both structuring elements.  No
library, no device."""
import numpy as np
import pytest

import regions_cases as cases
from tdnet_amd.dataloader import REGION_DTYPE, REGIONS_HEADER_DTYPE, RegionTable, region_table, regions_u8, regions_unpack

#       x: 0  1  2  3  4  5  6
MAP = np.array([[3, 3, 1, 7, 7, 1, 3],      # two member classes side by side never merge; 1 is no member; 255 is no class
                [1, 3, 1, 7, 1, 1, 1],
                [1, 1, 3, 1, 1, 3, 1],
                [3, 1, 1, 255, 3, 1, 1],
                [3, 3, 1, 3, 255, 1, 7]], np.uint8)


def rec(label, area, x0, y0, x1, y1, fy, fx, sx, sy):
    return (label, area, x0, y0, x1, y1, fy, fx, sx, sy)


def test_hand_written_answer_4_neighbours():
    ids, count, table = regions_u8(MAP, (3, 7), 4)
    want = np.array([[1, 1, 0, 2, 2, 0, 3],
                     [0, 1, 0, 2, 0, 0, 0],
                     [0, 0, 4, 0, 0, 5, 0],
                     [6, 0, 0, 0, 7, 0, 0],
                     [6, 6, 0, 8, 0, 0, 9]], np.int32)
    assert count == 9 and ids.dtype == np.int32 and np.array_equal(ids, want)
    assert table.dtype == REGION_DTYPE and REGION_DTYPE.itemsize == 48 and REGIONS_HEADER_DTYPE.itemsize == 16
    assert table.tolist() == [rec(3, 3, 0, 0, 1, 1, 0, 0, 2, 1), rec(7, 3, 3, 0, 4, 1, 0, 3, 10, 1), rec(3, 1, 6, 0, 6, 0, 0, 6, 6, 0),
                              rec(3, 1, 2, 2, 2, 2, 2, 2, 2, 2), rec(3, 1, 5, 2, 5, 2, 2, 5, 5, 2), rec(3, 3, 0, 3, 1, 4, 3, 0, 1, 11),
                              rec(3, 1, 4, 3, 4, 3, 3, 4, 4, 3), rec(3, 1, 3, 4, 3, 4, 4, 3, 3, 4), rec(7, 1, 6, 4, 6, 4, 4, 6, 6, 4)]


def test_hand_written_answer_8_neighbours():
    ids, count, table = regions_u8(MAP, (3, 7), 8)
    want = np.array([[1, 1, 0, 2, 2, 0, 3],      # (1,1)-(2,2) joins the first region to the single pixel; (2,5)-(3,4)-(4,3) is one diagonal chain
                     [0, 1, 0, 2, 0, 0, 0],
                     [0, 0, 1, 0, 0, 4, 0],
                     [5, 0, 0, 0, 4, 0, 0],
                     [5, 5, 0, 4, 0, 0, 6]], np.int32)
    assert count == 6 and np.array_equal(ids, want)
    assert table.tolist() == [rec(3, 4, 0, 0, 2, 2, 0, 0, 4, 3), rec(7, 3, 3, 0, 4, 1, 0, 3, 10, 1), rec(3, 1, 6, 0, 6, 0, 0, 6, 6, 0),
                              rec(3, 3, 3, 2, 5, 4, 2, 5, 12, 9), rec(3, 3, 0, 3, 1, 4, 3, 0, 1, 11), rec(7, 1, 6, 4, 6, 4, 4, 6, 6, 4)]


def test_min_area_renumbers_and_max_regions_cuts_the_table_only():
    ids, count, table = regions_u8(MAP, (3, 7), 8, min_area=3)
    want = np.array([[1, 1, 0, 2, 2, 0, 0],
                     [0, 1, 0, 2, 0, 0, 0],
                     [0, 0, 1, 0, 0, 3, 0],
                     [4, 0, 0, 0, 3, 0, 0],
                     [4, 4, 0, 3, 0, 0, 0]], np.int32)
    assert count == 4 and np.array_equal(ids, want) and table["area"].tolist() == [4, 3, 3, 3]
    ids2, count2, table2 = regions_u8(MAP, (3, 7), 8, min_area=3, max_regions=2)
    assert count2 == 4 and np.array_equal(ids2, want) and table2.tolist() == table[:2].tolist()
    ids, count, table = regions_u8(MAP, (), 8)
    assert count == 0 and not ids.any() and table.shape == (0,) and table.dtype == REGION_DTYPE
    ids, count, table = regions_u8(MAP, (7,), 4)
    assert count == 2 and table["label"].tolist() == [7, 7] and (ids > 0).sum() == 4
    ids, count, table = regions_u8(MAP, (255,), 8)                     # the oracle takes any byte as a class; the library refuses ids >= nclass
    assert count == 1 and table["area"].tolist() == [2]


def test_one_pixel_and_one_row():
    ids, count, table = regions_u8(np.array([[5]], np.uint8), (5,), 4)
    assert count == 1 and ids.tolist() == [[1]] and table.tolist() == [rec(5, 1, 0, 0, 0, 0, 0, 0, 0, 0)]
    ids, count, table = regions_u8(np.array([[5, 5, 0, 5]], np.uint8), (5,), 8)
    assert count == 2 and ids.tolist() == [[1, 1, 0, 2]] and table["sum_x"].tolist() == [1, 3]


def test_the_table_as_the_library_lays_it_out():
    _, count, table = regions_u8(MAP, (3, 7), 8)
    raw = np.zeros(16 + 48 * 8, np.uint8)
    raw[:16].view(REGIONS_HEADER_DTYPE)[0] = (count, count, 0, 0)
    raw[16:16 + 48 * count] = table.view(np.uint8)
    hdr, recs = regions_unpack(raw, 8)
    assert int(hdr["count"]) == 6 and recs.shape == (8,) and recs[:6].tolist() == table.tolist() and not recs[6:].view(np.uint8).any()
    t = region_table(raw.tobytes(), 8)
    assert isinstance(t, RegionTable) and t.count == 6 and t.status == 0 and len(t) == 6 and t.tolist() == table.tolist()
    assert float(t["sum_x"][0]) / t["area"][0] == 1.0                  # the centroid is sum / area


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", cases.PATTERNS)
def test_against_scipy_label_per_class(name, conn):
    """scipy.ndimage.label of one class's mask numbers its components in raster order of their first pixel: the oracle's numbering restricted to that
    class, and its pixel sets."""
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), int) if conn == 8 else ndimage.generate_binary_structure(2, 1)
    for H, W in ((5, 7), (17, 67), (35, 70)):
        labels, classes = cases.pattern(name, H, W, 16, 64)
        ids, count, table = regions_u8(labels, classes, conn, 1, 1 << 16)
        assert count == len(table) == ids.max()
        seen = 0
        for c in classes:
            want, n = ndimage.label(labels == c, structure=structure)
            mine = np.flatnonzero(table["label"] == c) + 1             # this class's regions, by growing key
            assert len(mine) == n, (name, conn, c)
            got = np.zeros_like(want)
            for k, i in enumerate(mine):
                got[ids == i] = k + 1
            assert np.array_equal(got, want), (name, conn, c)
            seen += n
            objs = ndimage.find_objects(want)
            for k, i in enumerate(mine):
                r = table[i - 1]
                sl = objs[k]
                assert (r["y0"], r["y1"] + 1, r["x0"], r["x1"] + 1) == (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)
                assert r["area"] == (want == k + 1).sum()
        assert seen == count and not ids[~np.isin(labels, classes)].any()
