"""Sequences and checks of tracks out (include/tdnet.h "tracks out"), shared by tests/test_emu_tracks.py (CPU, through the emulator) and
tests/test_gpu_tracks.py (device memory).  The expected id map, regions table, track map, header and records of every frame come from
tdnet_amd.dataloader.TrackOracle, which tests/test_tracks_host.py holds to hand-written answers.  Every comparison is exact: everything is an integer.

An operator sequence runs frame by frame through tdnet_op_tracks on ONE state blob; the label maps, the id map, the track map, both tables AND the
state blob sit between opcheck's guard bands (bytes and int32 words inside float32 holders, as in regions_cases.py), verified once the sequence ends."""
import functools

import numpy as np

import regions_cases
from regions_cases import get_bytes, put_bytes, words
from tdnet_amd.dataloader import REGION_DTYPE, REGIONS_HEADER_DTYPE, TRACK_DTYPE, TRACKS_HEADER_DTYPE, TrackOracle

C = regions_cases.C
FAMILIES = ("still", "moving", "split", "merge", "tie", "class_change", "vanish", "renumber", "beyond_table", "min_area", "overlap_1", "overlap_2", "overlap_large",
            "checker_worst", "noise_to_noise", "reset")


def shapes(th, tw):
    """The map sizes at which the quad tail, the wave rounds, the probe wrap-around and the cross-workgroup pair table can go wrong, from the real tile of
    the regions kernels; (128, 256) spans the XCDs on the device."""
    return ((1, 1), (1, tw + 3), (th + 1, 1), (th, tw), (th + 1, tw + 1), (2 * th + 3, 3 * tw + 5), (128, 256))


def big(H, W):
    """large enough for the hand-written expectations of a family (below that the sequence is still held to the oracle)"""
    return H >= 8 and W >= 16


def _blank(H, W):
    return np.full((H, W), 1, np.uint8)                                # 1: a class outside every set used here


def _blob(H, W, x0, label=3, y0=None, bw=None, bh=None):
    lab = _blank(H, W)
    bw, bh = bw or max(1, W // 4), bh or max(1, H // 2)
    y0 = H // 4 if y0 is None else y0
    lab[y0:y0 + bh, max(0, x0):max(0, x0 + bw)] = label
    return lab


@functools.lru_cache(maxsize=None)
def sequence(name, H, W):
    """(frames, keyword arguments of run_sequence) of one family at one size"""
    kw = dict(classes=(3, 7, 11), conn=8, max_regions=256, min_area=1, min_overlap=1, reset_before=())
    yy, xx = np.mgrid[0:H, 0:W]
    bw = max(1, W // 4)
    if name == "still":
        frames = [regions_cases.noise(H, W)] * 4
        kw.update(max_regions=4096)
    elif name in ("moving", "overlap_1", "overlap_2", "overlap_large"):
        frames = [_blob(H, W, 0), _blob(H, W, 1), _blob(H, W, 2), _blob(H, W, 2 + bw + 1), _blob(H, W, 2 + bw + 1 + max(1, bw - 1))]
        kw.update(min_overlap={"moving": 1, "overlap_1": 1, "overlap_2": 2, "overlap_large": H * W + 1}[name])
        if name != "moving":                                           # a one-row blob: the overlaps are bw - 1, bw - 1, 0 and min(1, bw - 1) pixels
            frames = [np.where(yy == H // 4, f, 1).astype(np.uint8) for f in frames]
    elif name in ("split", "merge"):
        bar, two = _blank(H, W), _blank(H, W)
        bar[0, :] = 3
        two[0, :] = 3
        two[0, W // 3] = 1                                             # the left piece is the smaller
        frames = [bar, two, two] if name == "split" else [two, bar, bar]
    elif name == "tie":
        two, one = _blank(H, W), _blank(H, W)
        two[0, 0:2] = 3
        two[0, 3:5] = 3
        one[0, 1:4] = 3
        frames = [two, one, two, one]
    elif name == "class_change":
        frames = [_blob(H, W, 1, 3), _blob(H, W, 1, 7), _blob(H, W, 1, 7), _blob(H, W, 1, 3)]
    elif name == "vanish":
        frames = [_blob(H, W, 1), _blank(H, W), _blob(H, W, 1), _blob(H, W, 1)]
    elif name == "renumber":
        a = _blank(H, W)
        a[H // 2:, 0:bw] = 3
        a[H // 2:, W - bw:] = 7
        b = a.copy()
        b[0, W // 2] = 11
        frames = [a, b, a, b]
    elif name == "beyond_table":                                       # a region per pixel, 5 records: everything from region 6 on is background to the match
        frames = [np.where((yy + xx) % 2 == 0, 3, 7).astype(np.uint8), np.where((yy + xx) % 2 == 0, 7, 3).astype(np.uint8),
                  np.where((yy + xx) % 2 == 0, 7, 3).astype(np.uint8), _blob(H, W, 0, bw=W, bh=1, y0=0)]
        kw.update(conn=4, max_regions=5)
    elif name == "min_area":
        frames = [regions_cases.noise(H, W), regions_cases.noise(H, W, seed=1), regions_cases.noise(H, W)]
        kw.update(min_area=3, max_regions=4096)
    elif name == "checker_worst":                                      # 4 neighbours, every region stored: H W regions, H W distinct pairs
        frames = [np.where((yy + xx) % 2 == 0, 3, 7).astype(np.uint8)] * 3
        kw.update(conn=4, max_regions=65536, classes=(3, 7))
        assert H * W <= 65536
    elif name == "noise_to_noise":
        frames = [regions_cases.noise(H, W), regions_cases.noise(H, W, seed=1), regions_cases.noise(H, W), regions_cases.noise(H, W, seed=1)]
        kw.update(max_regions=4096)
    elif name == "reset":
        frames = [regions_cases.noise(H, W)] * 2 + [regions_cases.noise(H, W, seed=1)] * 2
        kw.update(max_regions=4096, reset_before=(2,))
    else:
        raise KeyError(name)
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    for f in frames:
        f.setflags(write=False)
    assert 3 <= len(frames) <= 5
    return tuple(frames), kw


_oracle = {}


def oracle(frames, classes, conn, min_area, max_regions, min_overlap, reset_before=()):
    """TrackOracle stepped once per distinct question: a list of (ids, region table, track map, header, records), read-only"""
    key = (frames[0].shape, tuple(f.tobytes() for f in frames), tuple(classes), conn, min_area, max_regions, min_overlap, tuple(reset_before))
    if key not in _oracle:
        o, out = TrackOracle(classes, conn, min_area, max_regions, min_overlap), []
        for t, f in enumerate(frames):
            if t in reset_before:
                o.reset()
            step = o.step(f)
            for a in step[:3] + step[4:]:
                a.setflags(write=False)
            out.append(step)
        _oracle[key] = out
    return _oracle[key]


def compare(got, want, max_regions, what=()):
    """got = (ids or None, regions header, regions records [max_regions], track map or None, tracks header, track records [max_regions]) of one frame
    against the oracle's step"""
    ids, rhdr, rrecs, tmap, hdr, recs = got
    want_ids, table, want_map, want_hdr, want_recs = want
    stored = len(table)
    assert int(rhdr["stored"]) == stored, what + ("regions header", rhdr, stored)
    for f in REGION_DTYPE.names:
        assert np.array_equal(rrecs[f][:stored], table[f]), what + ("region field " + f,)
    if ids is not None:
        assert np.array_equal(ids, want_ids), what + ("id map",)
    for f in TRACKS_HEADER_DTYPE.names:
        assert int(hdr[f]) == int(want_hdr[f]), what + ("tracks header " + f, hdr, want_hdr)
    assert recs.shape == (max_regions,)
    for f in TRACK_DTYPE.names:
        bad = recs[f][:stored] != want_recs[f]
        assert not bad.any(), what + ("track field " + f, int(np.argmax(bad)), recs[:stored][bad][:1], want_recs[bad][:1])
    assert not recs[stored:].view(np.uint8).any(), what + ("track records beyond stored are not zero",)
    if tmap is not None:
        bad = tmap != want_map
        assert not bad.any(), what + ("track map", int(bad.sum()), tuple(int(i) for i in np.argwhere(bad)[0]))


def new_state(lib, mem, H, W):
    """a zeroed state blob between guard bands (an input to the guards: it is read and written)"""
    n = int(lib.tdnet_op_tracks_state_bytes(H, W))
    assert n > 0 and n % 16 == 0
    return mem.put(np.zeros(n // 4, np.float32))


def run_sequence(lib, mem, frames, classes, conn, max_regions, min_area, min_overlap, reset_before=(), lab_off=0, want_ids=True, want_map=True, what=()):
    """The frames through tdnet_op_tracks on one state blob, every frame compared with the oracle; returns the oracle's steps.  A reset is a zeroed blob."""
    H, W = frames[0].shape
    state = new_state(lib, mem, H, W)
    want = oracle(frames, classes, conn, min_area, max_regions, min_overlap, reset_before)
    cls = np.ascontiguousarray(classes, np.uint8)
    for t, labels in enumerate(frames):
        if t in reset_before:
            state[...] = 0
        ids_t = mem.empty((H, W)) if want_ids else None
        map_t = mem.empty((H, W)) if want_map else None
        rtab_t, ttab_t = mem.empty((words(16 + 48 * max_regions),)), mem.empty((words(16 + 24 * max_regions),))
        lab_t, lab_p = put_bytes(mem, labels, lab_off)
        lib.check(lib.tdnet_op_tracks(lab_p, C, H, W, cls.ctypes.data if cls.size else None, int(cls.size), conn, max_regions, min_area, min_overlap, mem.ptr(state),
                                      mem.ptr(ids_t), mem.ptr(rtab_t), mem.ptr(map_t), mem.ptr(ttab_t), mem.stream))
        i32 = lambda h: None if h is None else np.ascontiguousarray(np.asarray(mem.get(h))).view(np.int32).reshape(H, W).copy()
        rraw, traw = get_bytes(mem, rtab_t, 16 + 48 * max_regions), get_bytes(mem, ttab_t, 16 + 24 * max_regions)
        assert np.array_equal(get_bytes(mem, lab_t, H * W, lab_off).reshape(H, W), labels)   # the label map is only read
        got = (i32(ids_t), rraw[:16].view(REGIONS_HEADER_DTYPE)[0], rraw[16:].view(REGION_DTYPE), i32(map_t), traw[:16].view(TRACKS_HEADER_DTYPE)[0],
               traw[16:].view(TRACK_DTYPE))
        compare(got, want[t], max_regions, what + ("frame", t))
    mem.verify()
    return want


def check_family(lib, mem, name, H, W):
    """One family at one size against the oracle; at sizes where the pattern has room, the oracle's answer against what the family is about."""
    frames, kw = sequence(name, H, W)
    if name == "checker_worst":
        assert int(lib.tdnet_op_tracks_capacity(H, W)) >= 2 * H * W   # every pixel a pair of its own, and the table at most half full
    steps = run_sequence(lib, mem, frames, what=(name, H, W), **kw)
    hdr = [s[3] for s in steps]
    rec = [s[4] for s in steps]
    bw = max(1, W // 4)
    if name == "checker_worst" and H * W > 1:
        assert all(int(h["count"]) == H * W for h in hdr) and int(hdr[1]["matched"]) == H * W and (rec[2]["age"] == 3).all() and (rec[2]["overlap"] == 1).all()
    if name == "still":
        for t in range(1, len(steps)):
            assert int(hdr[t]["matched"]) == int(hdr[t]["count"]) and int(hdr[t]["ended"]) == 0 and (int(hdr[t]["count"]) > 0 or not big(H, W))
            assert np.array_equal(rec[t]["track"], rec[0]["track"]) and (rec[t]["age"] == t + 1).all()
    if not big(H, W):
        return steps
    if name == "moving":
        assert [int(r["track"][0]) for r in rec] == [1, 1, 1, 2, 2 if bw > 1 else 3] and [int(r["age"][0]) for r in rec[:4]] == [1, 2, 3, 1]
        assert int(hdr[3]["ended"]) == 1 and int(hdr[3]["matched"]) == 0
    if name == "overlap_2":
        assert [int(h["matched"]) for h in hdr] == [0, int(bw - 1 >= 2), int(bw - 1 >= 2), 0, 0]
    if name == "overlap_large":
        assert all(int(h["matched"]) == 0 for h in hdr) and [int(r["track"][0]) for r in rec] == [1, 2, 3, 4, 5] and int(rec[1]["origin_track"][0]) == 1
    if name == "split":                                                # the larger (right) piece continues; the left is born out of the bar's track
        assert rec[1]["track"].tolist() == [2, 1] and rec[1]["origin_track"].tolist() == [1, 1] and rec[1]["age"].tolist() == [1, 2]
        assert rec[2]["track"].tolist() == [2, 1] and int(hdr[1]["ended"]) == 0
    if name == "merge":
        assert rec[0]["track"].tolist() == [1, 2] and rec[1]["track"].tolist() == [2] and int(hdr[1]["ended"]) == 1 and rec[1]["prev_region"].tolist() == [2]
    if name == "tie":                                                  # the smallest number wins on both sides
        assert rec[1]["track"].tolist() == [1] and rec[1]["prev_region"].tolist() == [1] and int(hdr[1]["ended"]) == 1
        assert rec[2]["track"].tolist() == [1, 3] and rec[2]["origin_track"].tolist() == [1, 1] and rec[2]["age"].tolist() == [3, 1]
    if name == "class_change":
        assert [int(h["matched"]) for h in hdr] == [0, 0, 1, 0] and [int(r["track"][0]) for r in rec] == [1, 2, 2, 3] and int(rec[1]["origin_track"][0]) == 0
    if name == "vanish":
        assert [int(h["count"]) for h in hdr] == [1, 0, 1, 1] and int(hdr[1]["ended"]) == 1 and [int(r["track"][0]) for r in rec if len(r)] == [1, 2, 2]
    if name == "renumber":                                             # the new object takes region number 1; the tracks keep their ids
        assert rec[0]["track"].tolist() == [1, 2] and rec[1]["track"].tolist() == [3, 1, 2] and rec[2]["track"].tolist() == [1, 2] and rec[3]["track"].tolist() == [4, 1, 2]
        assert rec[3]["age"].tolist() == [1, 4, 4]
    if name == "beyond_table":
        assert all(int(h["count"]) == 5 for h in hdr[:3]) and int(hdr[1]["matched"]) == 0 and int(hdr[2]["matched"]) == 5
        assert (steps[2][2] > 0).sum() == 5                            # the track map beyond the table is zero
    if name == "reset":
        assert int(hdr[2]["matched"]) == 0 and int(hdr[2]["ended"]) == 0 and rec[2]["track"].tolist() == list(range(1, len(rec[2]) + 1))
        assert int(hdr[3]["matched"]) == len(rec[3])
    return steps


def check_parameters(lib, mem, H, W):
    """the label map at byte offsets 1..3; the id map and the track map left out, each and both"""
    frames, kw = sequence("noise_to_noise", H, W)
    for off in (1, 2, 3):
        run_sequence(lib, mem, frames[:3], lab_off=off, what=("byte offset", off), **kw)
    for want_ids, want_map in ((False, True), (True, False), (False, False)):
        run_sequence(lib, mem, frames[:3], want_ids=want_ids, want_map=want_map, what=("left out", want_ids, want_map), **kw)


def check_frame(got, want, max_regions, what=()):
    """got = (ids or None, regions table bytes, track map or None, tracks table bytes) of a frame entry against an oracle step"""
    ids, rraw, tmap, traw = got
    rraw, traw = np.ascontiguousarray(rraw).view(np.uint8).reshape(-1), np.ascontiguousarray(traw).view(np.uint8).reshape(-1)
    compare((ids, rraw[:16].view(REGIONS_HEADER_DTYPE)[0], rraw[16:].view(REGION_DTYPE), tmap, traw[:16].view(TRACKS_HEADER_DTYPE)[0], traw[16:].view(TRACK_DTYPE)),
            want, max_regions, what)
