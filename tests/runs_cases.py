"""Cases and checks of runs out (include/tdnet.h "runs out"), shared by tests/test_emu_runs.py (CPU, through the emulator) and tests/test_gpu_runs.py
(device memory).  The expected tables come from tdnet_amd.dataloader.runs_of, which tests/test_runs_host.py holds to hand-written answers.  Every
comparison is exact: everything is an integer.

The maps and the table of an operator call sit between opcheck's guard bands, bytes and int32 words inside float32 holders.  The table is an output of
which only the header, the stored records and the closing record may be written: the rows behind the closing record are handed to the mem as
unwritten_rows, and verify() holds them to the fill bit for bit.  A record's words are arbitrary integers (-1 is a NaN's pattern), so every verify() here
runs with finite=False; bands and "fully written" are checked as always."""
import functools

import numpy as np

from tdnet_amd.dataloader import RUN_DTYPE, RUNS_HEADER_DTYPE, RUNS_OVERFLOW, runs_decode, runs_of

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
U8_PATTERNS = ("constant", "alternating", "stripes1", "stripes2", "stripes3", "stripes4", "stripes5", "stripes64", "singles-1", "singles+0", "singles+1",
               "noise3", "bytes_0_255")
I32_PATTERNS = ("alternating", "noise3", "extremes")


def block(lib):
    b = int(lib.tdnet_op_runs_block())
    assert b >= 8 and b % 4 == 0
    return b


def shapes(B):
    """The sizes at which the lane split, a block boundary or the scan's chunk carry can go wrong, from the kernels' real block of B pixels; the last has
    at least 257 blocks."""
    assert (2 * B + 1) % 3 == 0
    return ((1, 1), (1, 3), (1, B - 1), (1, B), (1, B + 1), (3, (2 * B + 1) // 3), (B + 1, 1), (5, 7), (33, 65), (128, 256), (513, 513))


@functools.lru_cache(maxsize=None)
def pattern(name, H, W, B, i32=False):
    yy, xx = np.mgrid[0:H, 0:W]
    flat = yy * W + xx
    if name == "constant":
        m = np.full((H, W), 5)
    elif name == "alternating":                                        # every pixel differs from its left neighbour; the value goes on across row ends
        m = 3 + 4 * (xx % 2)
    elif name.startswith("stripes"):
        m = 2 + (xx // int(name[7:])) % 3
    elif name.startswith("singles"):
        d = int(name[7:])
        m = np.full((H, W), 5)
        for step in (64, 256, B):
            m[(flat - d) % step == 0] = 9
    elif name == "noise3":
        m = np.random.default_rng(H * 1000 + W).integers(0, 3, (H, W))
    elif name == "bytes_0_255":
        m = 255 * np.random.default_rng(H * 1000 + W + 1).integers(0, 2, (H, W))
    elif name == "extremes":                                           # 2^24 + 1 against 2^24: equal once routed through a float
        m = np.random.default_rng(H * 1000 + W + 2).choice(np.array([-1, INT_MIN, INT_MAX, 2 ** 24 + 1, 2 ** 24], np.int64), size=(H, W))
    else:
        raise KeyError(name)
    m = np.ascontiguousarray(m.astype(np.int32 if i32 else np.uint8))
    m.setflags(write=False)
    return m


def words(nbytes):
    return (int(nbytes) + 3) // 4


def put_at(mem, a, off):
    """array `a` (uint8 or int32) at byte offset `off` of a guarded input: (holder, address)"""
    raw8 = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    raw = np.zeros(4 * words(raw8.size + off), np.uint8)
    raw[off:off + raw8.size] = raw8
    t = mem.put(raw.view(np.float32))
    return t, mem.ptr(t) + off


def get_bytes(mem, t, nbytes, off=0):
    return np.ascontiguousarray(np.asarray(mem.get(t))).view(np.uint8).reshape(-1)[off:off + nbytes].copy()


def table_holder(mem, max_runs, stored):
    """the table as 8-byte rows (2 of header, max_runs + 1 of records); the rows behind the closing record must stay unwritten"""
    keep = np.zeros(max_runs + 3, bool)
    keep[2 + stored + 1:] = True
    return mem.empty((max_runs + 3, 2), unwritten_rows=keep)


def compare(hdr, recs, m, max_runs, what=()):
    """header and records [max_runs + 1] as the library wrote them against runs_of(m); returns count"""
    whdr, wrecs = runs_of(m, max_runs)
    H, W = m.shape
    count, stored = int(whdr["count"]), int(whdr["stored"])
    assert H <= count <= H * W
    assert (int(hdr["count"]), int(hdr["stored"]), int(hdr["status"]), int(hdr["reserved"])) == (count, stored, RUNS_OVERFLOW if count > max_runs else 0, 0), \
        what + ("header", hdr, count, stored)
    for f in RUN_DTYPE.names:
        bad = recs[f][:stored + 1] != wrecs[f]
        assert not bad.any(), what + ("record field " + f, int(np.argmax(bad)), recs[:stored + 1][bad][:1], wrecs[bad][:1])
    assert int(recs["start"][stored]) == (H * W if stored == count else int(runs_of(m)[1]["start"][stored])) and int(recs["value"][stored]) == 0
    return count


def run_op(lib, mem, m, max_runs, off=0, what=()):
    """One call of tdnet_op_runs on a map (uint8 at byte offset off; int32 at byte offset 4 * off) between guard bands, compared with the oracle; returns
    (header, records [stored + 1], raw table bytes)."""
    H, W = m.shape
    i32 = m.dtype == np.int32
    stored = min(int(runs_of(m, max_runs)[0]["count"]), max_runs)
    boff = 4 * off if i32 else off
    map_t, map_p = put_at(mem, m, boff)
    tab_t = table_holder(mem, max_runs, stored)
    lib.check(lib.tdnet_op_runs(None, 0, 0, 0, H, W, None, None if i32 else map_p, map_p if i32 else None, max_runs, mem.ptr(tab_t), mem.stream))
    raw = get_bytes(mem, tab_t, 16 + 8 * (max_runs + 1))
    assert np.array_equal(get_bytes(mem, map_t, m.nbytes, boff), m.reshape(-1).view(np.uint8))   # the map is only read
    mem.verify(finite=False)                                           # bands intact, the rows behind the closing record still the fill
    hdr, recs = raw[:16].view(RUNS_HEADER_DTYPE)[0], raw[16:].view(RUN_DTYPE)
    compare(hdr, recs, m, max_runs, what + (m.shape, str(m.dtype), "offset", off, "max_runs", max_runs))
    return hdr, recs[:stored + 1], raw


def check_map(lib, mem, m, offsets=(0, 1, 2, 3), what=()):
    """A map at every offset with max_runs = H W, count, count - 1 and 1; returns count."""
    H, W = m.shape
    count = int(runs_of(m)[0]["count"])
    for off in offsets:
        for max_runs in sorted({H * W, count, max(count - 1, 1), 1}):
            hdr, recs, _ = run_op(lib, mem, m, max_runs, off, what)
            if max_runs >= count:
                assert not int(hdr["status"]) and int(recs["start"][-1]) == H * W
            else:
                assert int(hdr["status"]) == RUNS_OVERFLOW and int(hdr["count"]) == count and int(hdr["stored"]) == max_runs
    return count


def run_decode(lib, mem, raw, max_runs, fill, H, W, i32, off=0):
    """One call of tdnet_op_runs_decode on table bytes `raw` (16 + 8 (max_runs + 1)) between guard bands: the map written, uint8 at byte offset off or
    int32 at byte offset 4 * off"""
    assert raw.size == 16 + 8 * (max_runs + 1)
    tab_t, tab_p = put_at(mem, raw, 0)
    boff, size = (4 * off, 4) if i32 else (off, 1)
    keep = np.zeros(words(H * W * size + boff), bool)
    keep[:boff // 4] = True                                            # whole words in front of an int32 map: not the kernel's
    out_t = mem.empty((keep.size, 1), unwritten_rows=keep)
    out_p = mem.ptr(out_t) + boff
    lib.check(lib.tdnet_op_runs_decode(tab_p, max_runs, fill, H, W, None if i32 else out_p, out_p if i32 else None, mem.stream))
    got = get_bytes(mem, out_t, H * W * size, boff)
    if boff:                                                           # the bytes in front of the map and behind it are not the kernel's
        assert np.array_equal(get_bytes(mem, out_t, boff), np.full(4, mem.FILL, np.float32).view(np.uint8)[:boff])
    mem.verify(finite=False)
    return got.view(np.int32 if i32 else np.uint8).reshape(H, W)


def check_round_trip(lib, mem, m, offsets=(0, 1, 2, 3)):
    """encode on the device, decode on the device: the map again; an overflowed table: the map below its closing start, fill beyond"""
    H, W = m.shape
    i32 = m.dtype == np.int32
    count = int(runs_of(m)[0]["count"])
    fill = -3 if i32 else 0xC8
    for max_runs in sorted({H * W, count, max(count // 2, 1), 1}):
        hdr, recs, raw = run_op(lib, mem, m, max_runs)
        want = runs_decode(hdr, recs, H, W, fill, m.dtype)
        end = int(recs["start"][-1])
        assert np.array_equal(want.reshape(-1)[:end], m.reshape(-1)[:end]) and (want.reshape(-1)[end:] == (fill if i32 else fill & 255)).all()
        assert (end == H * W) == (max_runs >= count)
        for off in offsets if max_runs in (H * W, max(count // 2, 1)) else offsets[:1]:
            got = run_decode(lib, mem, raw, max_runs, fill, H, W, i32, off)
            assert np.array_equal(got, want), (m.shape, str(m.dtype), max_runs, off, int((got != want).sum()))


def check_from_logits(lib, mem, x, C, h, w, H, W, want_labels):
    """The fused order of launches: the labels written are the label kernel's, the table the oracle's of those labels."""
    x_t = mem.put(x)
    lab_t = mem.empty((words(H * W),))
    count = int(runs_of(want_labels)[0]["count"])
    for max_runs in (H * W, max(count - 1, 1)):
        tab_t = table_holder(mem, max_runs, min(count, max_runs))
        lib.check(lib.tdnet_op_runs(mem.ptr(x_t), C, h, w, H, W, mem.ptr(lab_t), None, None, max_runs, mem.ptr(tab_t), mem.stream))
        raw = get_bytes(mem, tab_t, 16 + 8 * (max_runs + 1))
        assert np.array_equal(get_bytes(mem, lab_t, H * W).reshape(H, W), want_labels), ("labels", C, H, W)
        compare(raw[:16].view(RUNS_HEADER_DTYPE)[0], raw[16:].view(RUN_DTYPE), want_labels, max_runs, ("from logits", C, H, W, max_runs))
    mem.verify(finite=False)


def check_frame_table(table, labels, max_runs, what=()):
    """a frame entry's table (any array of 16 + 8 (max_runs + 1) bytes) against the oracle on that frame's labels; returns count"""
    raw = np.ascontiguousarray(table).view(np.uint8).reshape(-1)
    assert raw.size == 16 + 8 * (max_runs + 1)
    return compare(raw[:16].view(RUNS_HEADER_DTYPE)[0], raw[16:].view(RUN_DTYPE), labels, max_runs, what)
