"""The oracle of tracks out (tdnet_amd.dataloader.TrackOracle, include/tdnet.h "tracks out") held to answers written by hand: split, merge, the two ties,
birth numbering, the class rule, min_overlap, the table limit and reset; the record layouts; the text of the command line's CSV.  No GPU, no library."""
import numpy as np
import pytest

from tdnet_amd.dataloader import TRACK_DTYPE, TRACKS_HEADER_DTYPE, TrackOracle, track_table, tracks_unpack


def frame(rows):
    """a label map from strings: '.' is class 1 (outside the set), a digit the class"""
    return np.array([[1 if ch == "." else int(ch) for ch in row] for row in rows], np.uint8)


def fields(recs, *names):
    return [tuple(int(r[n]) for n in names) for r in recs]


def test_the_layouts_are_those_of_the_header():
    assert TRACKS_HEADER_DTYPE.itemsize == 16 and TRACK_DTYPE.itemsize == 24
    assert TRACK_DTYPE.names == ("track", "age", "prev_region", "overlap", "origin_track", "reserved")
    assert TRACKS_HEADER_DTYPE.names == ("count", "matched", "ended", "status")
    raw = np.zeros(16 + 24 * 3, np.uint8)
    raw[:16].view("<u4")[:] = (2, 1, 4, 0)
    raw[16:].view("<u4")[:12] = (7, 3, 2, 5, 7, 0, 9, 1, 0, 0, 7, 0)
    hdr, recs = tracks_unpack(raw, 3)
    assert int(hdr["count"]) == 2 and recs.shape == (3,) and fields(recs[:2], "track", "age", "prev_region", "overlap", "origin_track") == [(7, 3, 2, 5, 7), (9, 1, 0, 0, 7)]
    t = track_table(raw.tobytes(), 3)
    assert len(t) == 2 and (t.matched, t.ended, t.status) == (1, 4, 0) and t["track"].tolist() == [7, 9]
    with pytest.raises(AssertionError):
        tracks_unpack(raw[:-1], 3)


def test_first_frame_everything_is_born_in_region_order():
    o = TrackOracle((3, 7))
    ids, table, tmap, hdr, recs = o.step(frame(["33.7", "....", "3..."]))
    assert ids.tolist() == [[1, 1, 0, 2], [0, 0, 0, 0], [3, 0, 0, 0]] and table["label"].tolist() == [3, 7, 3]
    assert fields(recs, "track", "age", "prev_region", "overlap", "origin_track", "reserved") == [(1, 1, 0, 0, 0, 0), (2, 1, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0)]
    assert (int(hdr["count"]), int(hdr["matched"]), int(hdr["ended"]), int(hdr["status"])) == (3, 0, 0, 0)
    assert tmap.tolist() == [[1, 1, 0, 2], [0, 0, 0, 0], [3, 0, 0, 0]] and tmap.dtype == np.int32


def test_split_the_larger_piece_continues_and_the_other_names_its_origin():
    o = TrackOracle((3,))
    o.step(frame(["3333333"]))
    _, _, tmap, hdr, recs = o.step(frame(["33.3333"]))
    assert fields(recs, "track", "age", "prev_region", "overlap", "origin_track") == [(2, 1, 0, 0, 1), (1, 2, 1, 4, 1)]
    assert (int(hdr["matched"]), int(hdr["ended"])) == (1, 0) and tmap.tolist() == [[2, 2, 0, 1, 1, 1, 1]]


def test_merge_one_track_continues_and_one_ends():
    o = TrackOracle((3,))
    o.step(frame(["33.3333"]))
    _, _, _, hdr, recs = o.step(frame(["3333333"]))
    assert fields(recs, "track", "age", "prev_region", "overlap", "origin_track") == [(2, 2, 2, 4, 2)]
    assert (int(hdr["count"]), int(hdr["matched"]), int(hdr["ended"])) == (1, 1, 1)
    _, _, _, hdr, recs = o.step(frame(["......."]))
    assert (int(hdr["count"]), int(hdr["matched"]), int(hdr["ended"])) == (0, 0, 1) and len(recs) == 0
    _, _, _, hdr, recs = o.step(frame(["3333333"]))                     # memory of one frame: not found again
    assert fields(recs, "track", "age", "origin_track") == [(3, 1, 0)] and int(hdr["ended"]) == 0


def test_ties_go_to_the_smallest_number_on_both_sides():
    o = TrackOracle((3,))
    o.step(frame(["33.33"]))                                           # regions 1, 2: tracks 1, 2
    _, _, _, hdr, recs = o.step(frame([".333."]))                       # one pixel of each: bp = 1
    assert fields(recs, "track", "age", "prev_region", "overlap") == [(1, 2, 1, 1)] and int(hdr["ended"]) == 1
    _, _, _, hdr, recs = o.step(frame(["33.33"]))                       # one pixel in each: bc(1) = 1; region 2 is born out of track 1
    assert fields(recs, "track", "age", "prev_region", "overlap", "origin_track") == [(1, 3, 1, 1, 1), (3, 1, 0, 0, 1)]
    assert (int(hdr["matched"]), int(hdr["ended"])) == (1, 0)


def test_the_best_partner_must_be_mutual():
    """c2 overlaps p1 in 2 pixels but p1 prefers c1 (3 pixels): c2 is born although it overlaps a track"""
    o = TrackOracle((3,))
    o.step(frame(["333333"]))
    _, _, _, hdr, recs = o.step(frame(["333.33"]))
    assert fields(recs, "track", "prev_region", "overlap", "origin_track") == [(1, 1, 3, 1), (2, 0, 0, 1)]


def test_a_track_keeps_its_class():
    o = TrackOracle((3, 7))
    o.step(frame(["33", "33"]))
    _, _, _, hdr, recs = o.step(frame(["77", "77"]))
    assert fields(recs, "track", "age", "origin_track") == [(2, 1, 0)] and (int(hdr["matched"]), int(hdr["ended"])) == (0, 1)
    _, _, _, hdr, recs = o.step(frame(["73", "77"]))                    # region 1 is the 7s (first pixel 0), region 2 the 3
    assert fields(recs, "track", "age", "overlap", "origin_track") == [(2, 2, 3, 2), (3, 1, 0, 0)]


def test_min_overlap_and_min_area():
    o = TrackOracle((3,), min_overlap=3)
    o.step(frame(["3333.."]))
    _, _, _, hdr, recs = o.step(frame(["..3333"]))                      # 2 pixels in common: mutual, but below min_overlap -- born, out of track 1
    assert fields(recs, "track", "age", "prev_region", "overlap", "origin_track") == [(2, 1, 0, 0, 1)] and int(hdr["ended"]) == 1
    _, _, _, hdr, recs = o.step(frame([".3333."]))                      # 3 pixels
    assert fields(recs, "track", "age", "prev_region", "overlap") == [(2, 2, 1, 3)]
    o = TrackOracle((3,), min_area=2)
    o.step(frame(["3.33"]))                                            # the single pixel is dropped: one region
    ids, table, tmap, hdr, recs = o.step(frame(["33.3"]))
    assert ids.tolist() == [[1, 1, 0, 0]] and tmap.tolist() == [[2, 2, 0, 0]] and fields(recs, "track", "origin_track") == [(2, 0)] and int(hdr["ended"]) == 1


def test_regions_beyond_the_table_are_background_to_the_match():
    o = TrackOracle((3,), connectivity=4, max_regions=2)
    ids, table, tmap, hdr, recs = o.step(frame(["3.3.3"]))
    assert ids.tolist() == [[1, 0, 2, 0, 3]] and len(table) == 2 and int(hdr["count"]) == 2 and tmap.tolist() == [[1, 0, 2, 0, 0]]
    ids, table, tmap, hdr, recs = o.step(frame(["..3.3"]))              # the old third region is now the second: it had no record, so it is born
    assert fields(recs, "track", "age", "prev_region") == [(2, 2, 2), (3, 1, 0)] and (int(hdr["matched"]), int(hdr["ended"])) == (1, 1)


def test_reset_restarts_the_ids():
    o = TrackOracle((3,))
    o.step(frame(["33.3"]))
    o.step(frame(["33.3"]))
    o.reset()
    _, _, _, hdr, recs = o.step(frame(["33.3"]))
    assert fields(recs, "track", "age", "origin_track") == [(1, 1, 0), (2, 1, 0)] and (int(hdr["matched"]), int(hdr["ended"])) == (0, 0)


def test_the_csv_gains_three_columns_and_is_unchanged_without_tracks():
    from tdnet_amd.test import regions_csv
    o = TrackOracle((3,))
    o.step(frame(["3333333"]))
    _, table, _, _, recs = o.step(frame(["33.3333"]))
    plain = regions_csv(table)
    assert plain == "id,label,area,x0,y0,x1,y1,cx,cy\n1,3,2,0,0,1,0,0.500,0.000\n2,3,4,3,0,6,0,4.500,0.000\n"
    assert regions_csv(table, recs) == "id,label,area,x0,y0,x1,y1,cx,cy,track,age,origin\n1,3,2,0,0,1,0,0.500,0.000,2,1,1\n2,3,4,3,0,6,0,4.500,0.000,1,2,1\n"
