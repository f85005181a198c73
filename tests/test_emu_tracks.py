"""Tracks out (include/tdnet.h "tracks out"), on the CPU through the kernel emulator: the four launches of csrc/td_tracks.h behind the regions pipeline,
through tdnet_op_tracks against TrackOracle on every family and size of tests/tracks_cases.py, between guard bands (the state blob included); whole frames
at 33x65 against the oracle stepped on the same frames' labels; the launch count; the error paths.  Every comparison is exact."""
import numpy as np
import pytest

import emu_util
import opcheck
import regions_cases
import tracks_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine

REGIONS_LAUNCHES, LAUNCHES = 7, 4                                      # include/tdnet.h TDNET_REGIONS_LAUNCHES, TDNET_TRACKS_LAUNCHES
TH, TW = 16, 64                                                        # csrc/td_regions.h's tile: the shapes are sized from it at collection, and ...


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.emu_lib()
    assert regions_cases.tile(lib) == (TH, TW)                         # ... held to the library's own answer here
    return lib


@pytest.mark.parametrize("shape", cases.shapes(TH, TW), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.FAMILIES)
def test_families_against_the_oracle(lib, name, shape):
    steps = cases.check_family(lib, opcheck.GuardedNumpyMem(), name, *shape)
    assert all(int(s[3]["status"]) == 0 for s in steps)


def test_label_map_offsets_and_maps_left_out(lib):
    cases.check_parameters(lib, opcheck.GuardedNumpyMem(), 33, 65)


def test_the_capacity_is_a_power_of_two_of_at_least_two_slots_a_pixel(lib):
    for H, W in ((1, 1), (1, 3), (33, 65), (128, 256), (1024, 2048)):
        cap = int(lib.tdnet_op_tracks_capacity(H, W))
        assert cap >= 2 * H * W and cap & (cap - 1) == 0 and cap < 4 * H * W + 2, (H, W, cap)
        assert int(lib.tdnet_op_tracks_state_bytes(H, W)) >= 8 * cap + 8 * H * W


def test_operator_entry_checks_its_arguments(lib):
    H, W = 9, 21
    labels = np.full((H, W), 3, np.uint8)
    ids, tmap = np.full((H, W), -7, np.int32), np.full((H, W), -7, np.int32)
    rtab, ttab = np.full(16 + 48 * 4 + 8, 0xEE, np.uint8), np.full(16 + 24 * 4 + 8, 0xEE, np.uint8)
    rbase, tbase = rtab.ctypes.data + (-rtab.ctypes.data) % 8, ttab.ctypes.data + (-ttab.ctypes.data) % 8
    n = int(lib.tdnet_op_tracks_state_bytes(H, W))
    raw = np.zeros(n + 16, np.uint8)
    sbase = raw.ctypes.data + (-raw.ctypes.data) % 16
    cls = np.array([3], np.uint8)
    ok = (labels.ctypes.data, 19, H, W, cls.ctypes.data, 1, 8, 4, 1, 1, sbase, ids.ctypes.data, rbase, tmap.ctypes.data, tbase, None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.tdnet_op_tracks(*a)

    for kw, word in (({"a14": tbase + 1}, "tracks_dev"), ({"a14": tbase + 4}, "tracks_dev = 0x"), ({"a14": None}, "tracks_dev is NULL"), ({"a12": rbase + 4}, "regions_dev"),
                     ({"a12": None}, "regions_dev"), ({"a9": 0}, "min_overlap"), ({"a10": None}, "state_dev"), ({"a10": sbase + 8}, "state_dev"), ({"a6": 6}, "connectivity"),
                     ({"a7": 0}, "max_regions"), ({"a8": 0}, "min_area"), ({"a0": None}, "tdnet_op_tracks"), ({"a1": 257}, "tdnet_op_tracks"),
                     ({"a4": np.array([19], np.uint8).ctypes.data}, "not a class id")):
        assert call(**kw) != 0 and word.encode() in lib.tdnet_last_error(), (kw, lib.tdnet_last_error())
    assert (ids == -7).all() and (tmap == -7).all() and (rtab == 0xEE).all() and (ttab == 0xEE).all() and not raw.any()   # nothing was written
    lib.check(call())                                                  # and the same arguments as they should be
    assert (ids == 1).all() and (tmap == 1).all()


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
H, W, HS, WS, T = 33, 65, 41, 83, 6
CLASSES, CONN, MAXR, MIN_AREA, MIN_OVERLAP = (0, 2, 5, 8, 11, 13, 17), 8, 64, 2, 2


def _engine(lib, model):
    name = {4: "td4", 2: "td2"}[model]
    spec = arch.model_spec(name, 19, "resnet18")
    e = Engine(model, 18, 19, H, W, 0, lib=lib, arch={})
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


@pytest.fixture(scope="module", params=[2, 4], ids=["td2", "td4"])
def clip(lib, request):
    """six frames of random bytes at 41x83 with the labels forward_u8_labels gives for them on a handle of its own, that handle's launch counts, and the
    oracle stepped on those labels"""
    P = request.param
    owner = _engine(lib, P)
    owner.set_input_u8(HS, WS)
    rng = np.random.default_rng(31)
    frames = [rng.integers(0, 256, (HS, WS, 3), dtype=np.uint8) for _ in range(T)]
    labels, launches = [], []
    for t, src in enumerate(frames):
        l8 = np.full((H, W), 0xEE, np.uint8)
        owner.forward_u8_labels(src, t % P, l8)
        labels.append(l8)
        launches.append(owner.last_launch_count())
    for a in frames + labels:
        a.setflags(write=False)
    want = cases.oracle(labels, CLASSES, CONN, MIN_AREA, MAXR, MIN_OVERLAP)
    yield P, owner, frames, labels, launches, want
    owner.close()


def _buffers(e):
    return (np.full((H, W), 0xEE, np.uint8), np.full((H, W), -7, np.int32), np.full(e.regions_bytes() // 8, 0xEEEEEEEEEEEEEEEE, np.uint64),
            np.full((H, W), -7, np.int32), np.full(e.tracks_bytes() // 8, 0xEEEEEEEEEEEEEEEE, np.uint64))


def _tracked(owner):
    e = owner.share()
    e.set_input_u8(HS, WS)
    e.set_tracks(MIN_OVERLAP)                                          # in either order
    assert e.tracks_bytes() == 0
    e.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
    assert e.tracks_bytes() == 16 + 24 * MAXR
    return e


def test_tracked_frames_equal_the_oracle_and_the_regions_entry(clip):
    P, owner, frames, labels, launches, want = clip
    a, r = _tracked(owner), owner.share()
    r.set_input_u8(HS, WS)
    r.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
    for t, src in enumerate(frames):
        l8, ids, rtab, tmap, ttab = _buffers(a)
        a.forward_u8_tracks(src, t % P, l8 if t % 2 == 0 else None, ids if t % 3 else None, rtab, tmap if t % 4 != 1 else None, ttab)
        assert a.last_launch_count() == launches[t] - 1 + REGIONS_LAUNCHES + LAUNCHES, t
        l8r, idsr, rtabr = np.full((H, W), 0xEE, np.uint8), np.full((H, W), -7, np.int32), np.full(rtab.size, 7, np.uint64)
        r.forward_u8_regions(src, t % P, l8r, idsr, rtabr)
        assert a.last_launch_count() == r.last_launch_count() + LAUNCHES
        assert np.array_equal(rtab, rtabr) and (np.array_equal(ids, idsr) if t % 3 else (ids == -7).all())     # byte for byte the regions entry's
        assert np.array_equal(l8, labels[t]) if t % 2 == 0 else (l8 == 0xEE).all()
        assert (tmap == -7).all() or t % 4 != 1
        cases.check_frame((ids if t % 3 else None, rtab, tmap if t % 4 != 1 else None, ttab), want[t], MAXR, ("frame", t))
        a.set_tracks(MIN_OVERLAP)                                      # idempotent: the tracks go on
    assert a.fifo_len() == owner.fifo_len() and sum(int(s[3]["matched"]) for s in want) > 0
    a.close()
    r.close()


def test_split_frames_and_other_entries_between_tracked_frames(clip):
    """encode_u8 + propagate_tracks and forward_u8_tracks in turn; a regions entry between two tracked frames leaves the track state alone"""
    P, owner, frames, labels, launches, want = clip
    c = _tracked(owner)
    for t, src in enumerate(frames):
        l8, ids, rtab, tmap, ttab = _buffers(c)
        if t % 2 == 0:
            c.encode_u8(src, t % P)
            c.propagate_tracks(l8, ids, rtab, tmap, ttab)
        else:
            c.forward_u8_tracks(src, t % P, l8, ids, rtab, tmap, ttab)
        assert np.array_equal(l8, labels[t]), t
        cases.check_frame((ids, rtab, tmap, ttab), want[t], MAXR, ("split frame", t))
        junk_ids, junk_tab = np.zeros((H, W), np.int32), np.zeros(rtab.size, np.uint64)
        c.labels_regions(labels[(t + 3) % T], junk_ids, junk_tab)      # the unfused regions entry runs on THIS handle's regions workspace
    c.close()


def test_the_unfused_entry_and_the_reset(clip):
    P, owner, frames, labels, launches, want = clip
    e = _tracked(owner)
    reset_before = (3,)
    want_r = cases.oracle(labels, CLASSES, CONN, MIN_AREA, MAXR, MIN_OVERLAP, reset_before)
    for t in range(T):
        if t in reset_before:
            e.tracks_reset()
            e.reset()                                                  # the FIFO's reset does not touch the tracks (and here there is nothing in it)
        _, ids, rtab, tmap, ttab = _buffers(e)
        e.labels_tracks(labels[t], ids, rtab, tmap, ttab)
        cases.check_frame((ids, rtab, tmap, ttab), want_r[t], MAXR, ("unfused", t))
    assert want_r[3][4]["track"].tolist() == list(range(1, len(want_r[3][4]) + 1))   # ids restart at 1
    e.reset()
    _, ids, rtab, tmap, ttab = _buffers(e)
    e.labels_tracks(labels[T - 1], ids, rtab, tmap, ttab)              # tdnet_reset left the tracks: the same map again continues every one
    hdr = ttab.view(np.uint8)[:16].view(cases.TRACKS_HEADER_DTYPE)[0]
    assert int(hdr["matched"]) == int(hdr["count"]) == len(want_r[T - 1][4]) and int(hdr["ended"]) == 0
    e.close()


def test_errors_name_the_missing_call_and_leave_a_pending_frame_alone(lib, clip):
    P, owner, frames, labels, launches, want = clip
    e = owner.share()
    x = np.zeros((1, 3, H, W), np.float32)
    e.set_input_u8(HS, WS)
    e.encode_u8(frames[0], 0)                                          # a pending frame: every failure below must leave it pending
    l8, ids, tmap = np.full((H, W), 0xEE, np.uint8), np.full((H, W), -7, np.int32), np.full((H, W), -7, np.int32)
    rtab, ttab = np.full(2 + 6 * 4, 0xEEEEEEEEEEEEEEEE, np.uint64), np.full(2 + 3 * 4 + 1, 0xEEEEEEEEEEEEEEEE, np.uint64)
    calls = (lambda tt=ttab, rt=rtab: e.forward_tracks(x, 1, l8, ids, rt, tmap, tt), lambda tt=ttab, rt=rtab: e.forward_u8_tracks(frames[1], 1, l8, ids, rt, tmap, tt),
             lambda tt=ttab, rt=rtab: e.propagate_tracks(l8, ids, rt, tmap, tt), lambda tt=ttab, rt=rtab: e.labels_tracks(labels[0], ids, rt, tmap, tt))
    for call in calls:
        with pytest.raises(_capi.TdnetError, match="tdnet_set_regions"):
            call()
    with pytest.raises(_capi.TdnetError, match="tdnet_set_tracks"):
        e.tracks_reset()
    _, before, _ = e.memory_bytes()
    with pytest.raises(_capi.TdnetError, match="min_overlap"):
        e.set_tracks(0)
    assert e.tracks_bytes() == 0 and e.memory_bytes()[1] == before
    e.set_regions(CLASSES, 4, 4, 2)
    for call in calls:
        with pytest.raises(_capi.TdnetError, match="tdnet_set_tracks"):
            call()
    _, before, _ = e.memory_bytes()
    e.set_tracks(1)
    state = int(lib.tdnet_op_tracks_state_bytes(H, W))
    assert e.tracks_bytes() == 16 + 24 * 4 and e.memory_bytes()[1] == before + state   # the state is counted ...
    e.set_tracks(3)
    e.set_regions(CLASSES, 8, 9, 1)                                    # ... once, and other regions arguments need no reallocation
    assert e.tracks_bytes() == 16 + 24 * 9 and e.memory_bytes()[1] == before + state
    e.set_regions(CLASSES, 4, 4, 2)
    e.set_tracks(1)
    odd_t, odd_r = ttab.view(np.uint8)[4:], rtab.view(np.uint8)[4:]
    for call in calls:
        with pytest.raises(_capi.TdnetError, match="tracks_dev = 0x[0-9a-f]+ is not 8-byte aligned"):
            call(tt=odd_t)
        with pytest.raises(_capi.TdnetError, match="regions_dev = 0x[0-9a-f]+ is not 8-byte aligned"):
            call(rt=odd_r)
        with pytest.raises(_capi.TdnetError, match="tracks_dev is NULL"):
            call(tt=None)
    with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):
        e.forward_u8_tracks(frames[1], 1, l8, ids, rtab, tmap, ttab)
    assert e.fifo_len() == 0 and (l8 == 0xEE).all() and (ids == -7).all() and (tmap == -7).all() and (rtab == 0xEEEEEEEEEEEEEEEE).all() and (ttab == 0xEEEEEEEEEEEEEEEE).all()
    e.propagate_tracks(l8, ids, rtab, tmap, ttab[:-1])                 # ... which is still there, and is the frame it was
    assert e.fifo_len() == 1 and np.array_equal(l8, labels[0]) and ttab[-1] == 0xEEEEEEEEEEEEEEEE
    cases.check_frame((ids, rtab, tmap, ttab[:-1]), cases.oracle(labels[:1], CLASSES, 4, 2, 4, 1)[0], 4)
    with pytest.raises(_capi.TdnetError, match="no encoded frame"):
        e.propagate_tracks(l8, ids, rtab, tmap, ttab[:-1])
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_tracks(1)
    fresh.close()
    e.close()
