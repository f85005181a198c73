"""The host-side oracles of runs out (tdnet_amd.dataloader.runs_of / runs_decode / run_table) against hand-written answers, and against each other on
random maps.  No device, no library."""
import numpy as np
import pytest

from tdnet_amd.dataloader import RUN_DTYPE, RUNS_HEADER_DTYPE, RUNS_OVERFLOW, run_table, runs_decode, runs_of


def _recs(pairs):
    return np.array(pairs, dtype=RUN_DTYPE)


def test_a_two_by_three_map():
    m = np.array([[4, 4, 7], [7, 7, 7]], np.uint8)                     # the 7 goes on into the next row: the row start still starts a run
    hdr, recs = runs_of(m)
    assert (int(hdr["count"]), int(hdr["stored"]), int(hdr["status"]), int(hdr["reserved"])) == (3, 3, 0, 0)
    assert np.array_equal(recs, _recs([(0, 4), (2, 7), (3, 7), (6, 0)]))
    hdr, recs = runs_of(m, 2)                                          # overflow: the closing record is the start of run 3
    assert (int(hdr["count"]), int(hdr["stored"]), int(hdr["status"])) == (3, 2, RUNS_OVERFLOW)
    assert np.array_equal(recs, _recs([(0, 4), (2, 7), (3, 0)]))
    assert np.array_equal(runs_decode(hdr, recs, 2, 3, 9, np.uint8), [[4, 4, 7], [9, 9, 9]])
    hdr, recs = runs_of(m, 3)                                          # max_runs == count: no overflow, the closing start is H W
    assert int(hdr["status"]) == 0 and int(recs["start"][-1]) == 6


def test_a_one_pixel_map():
    hdr, recs = runs_of(np.array([[200]], np.uint8))
    assert (int(hdr["count"]), int(hdr["stored"]), int(hdr["status"])) == (1, 1, 0)
    assert np.array_equal(recs, _recs([(0, 200), (1, 0)]))
    assert np.array_equal(runs_decode(hdr, recs, 1, 1, 0, np.uint8), [[200]])


def test_equal_values_across_a_row_end_and_negative_ids():
    m = np.array([[-1, -1], [-1, 5], [5, 5]], np.int32)
    hdr, recs = runs_of(m)
    assert int(hdr["count"]) == 4
    assert np.array_equal(recs, _recs([(0, -1), (2, -1), (3, 5), (4, 5), (6, 0)]))
    assert np.array_equal(runs_decode(hdr, recs, 3, 2, 0), m)
    assert np.array_equal(runs_decode(hdr, recs, 3, 2, 0, np.uint8), m.astype(np.uint8))   # the low byte


def test_the_constant_and_the_alternating_map_bound_the_count():
    assert int(runs_of(np.zeros((7, 9), np.uint8))[0]["count"]) == 7
    assert int(runs_of((np.arange(63).reshape(7, 9) % 2).astype(np.uint8))[0]["count"]) == 63   # W odd: the value flips across row ends too


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (13, 1), (9, 21), (33, 65)])
def test_decode_inverts_encode_on_random_maps(shape, dtype):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for k in (2, 3, 200):
        m = rng.integers(0, k, shape).astype(dtype) if dtype == np.uint8 else rng.integers(-k, k, shape).astype(dtype) * 123457
        hdr, recs = runs_of(m)
        assert np.array_equal(runs_decode(hdr, recs, *shape, 0, dtype), m)
        assert (np.diff(recs["start"].astype(np.int64)) > 0).all() and int(recs["start"][0]) == 0
        cut = max(int(hdr["count"]) // 2, 1)
        hdr2, recs2 = runs_of(m, cut)
        got = runs_decode(hdr2, recs2, *shape, 77, dtype).reshape(-1)
        end = int(recs2["start"][-1])
        assert np.array_equal(got[:end], m.reshape(-1)[:end]) and (got[end:] == 77).all()


def test_run_table_reads_what_the_library_writes_and_nothing_behind_it():
    m = np.array([[1, 1, 2, 2], [3, 3, 3, 3]], np.uint8)
    hdr, recs = runs_of(m, 8)
    raw = np.full(16 + 8 * 9, 0xEE, np.uint8)                          # a table of max_runs = 8: the bytes behind the closing record are never written
    raw[:16] = np.array([hdr], RUNS_HEADER_DTYPE).view(np.uint8)
    raw[16:16 + recs.nbytes] = recs.view(np.uint8)
    for buf in (raw, raw.tobytes()):
        h2, r2 = run_table(buf)
        assert int(h2["count"]) == 3 and np.array_equal(r2, recs) and r2.shape == (4,)
