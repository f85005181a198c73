"""Runs out (include/tdnet.h "runs out"), on the CPU through the kernel emulator: the launches of csrc/td_runs.h through tdnet_op_runs / tdnet_op_runs_decode
against the oracle tdnet_amd.dataloader.runs_of on every pattern and size of tests/runs_cases.py, between guard bands -- the table's bytes behind the closing
record included; the fused order of launches against the labels of tdnet_op_upsample_argmax; whole frames at 33x65 against the same frames asked for as
labels; a table of random bytes through the decoder; the error paths.  Every comparison is exact."""
import numpy as np
import pytest

import emu_util
import opcheck
import out_cases
import runs_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import RUNS_HEADER_DTYPE, RUNS_OVERFLOW, run_table, runs_decode, runs_of
from tdnet_amd.engine import Engine

LAUNCHES, DECODE_LAUNCHES = 4, 1                                       # include/tdnet.h TDNET_RUNS_LAUNCHES, TDNET_RUNS_DECODE_LAUNCHES
B = 1024                                                               # csrc/td_runs.h's block: the shapes are sized from it at collection, and ...


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


@pytest.fixture(scope="module")
def blk(lib):
    assert cases.block(lib) == B                                       # ... held to the library's own answer here
    return B


@pytest.mark.parametrize("shape", cases.shapes(B), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.U8_PATTERNS)
def test_uint8_patterns_against_the_oracle(lib, blk, name, shape):
    H, W = shape
    count = cases.check_map(lib, opcheck.GuardedNumpyMem(), cases.pattern(name, H, W, blk), what=(name,))
    if name == "constant":
        assert count == H
    if name in ("alternating", "stripes1"):
        assert count == H * W


@pytest.mark.parametrize("shape", cases.shapes(B), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.I32_PATTERNS)
def test_int32_patterns_against_the_oracle(lib, blk, name, shape):
    H, W = shape
    count = cases.check_map(lib, opcheck.GuardedNumpyMem(), cases.pattern(name, H, W, blk, True), what=(name,))
    if name == "alternating":
        assert count == H * W


@pytest.mark.parametrize("field", out_cases.FIELDS)
@pytest.mark.parametrize("case", out_cases.CASES, ids=out_cases.case_id)
def test_from_logits_the_labels_are_the_label_kernels(lib, case, field):
    C, (h, w), (H, W) = case
    x = out_cases.logits(field, C, h, w)
    l32 = np.full((H, W), -1, np.int32)
    lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
    cases.check_from_logits(lib, opcheck.GuardedNumpyMem(), x, C, h, w, H, W, l32.astype(np.uint8))


@pytest.mark.parametrize("i32", [False, True], ids=["uint8", "int32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, B + 1), (5, 7), (33, 65), (128, 256)], ids=lambda s: "%dx%d" % s)
def test_the_device_round_trip_is_the_map(lib, blk, shape, i32):
    for name in ("constant", "alternating", "noise3", "extremes" if i32 else "bytes_0_255", "stripes5"):
        cases.check_round_trip(lib, opcheck.GuardedNumpyMem(), cases.pattern(name, shape[0], shape[1], blk, i32))


@pytest.mark.parametrize("i32", [False, True], ids=["uint8", "int32"])
def test_a_table_of_random_bytes_stays_inside_its_buffers(lib, i32):
    """unspecified values, but every guard band intact: nothing is written outside the map"""
    H, W = 33, 65
    rng = np.random.default_rng(11)
    for max_runs in (1, 7, H * W):
        for trial in range(4):
            raw = rng.integers(0, 256, 16 + 8 * (max_runs + 1), dtype=np.uint8)
            if trial == 1:                                             # a header that claims more than the table holds
                raw[:16] = np.array([(2 ** 32 - 1, 2 ** 32 - 1, 0, 0)], RUNS_HEADER_DTYPE).view(np.uint8)
            if trial == 2:                                             # stored = max_runs: every record is searched, the closing start is anywhere
                raw[4:8] = np.array([max_runs], "<u4").view(np.uint8)
            got = cases.run_decode(lib, opcheck.GuardedNumpyMem(), raw, max_runs, 5, H, W, i32, off=trial % 4)
            assert got.shape == (H, W)


def test_operator_entries_check_their_arguments(lib):
    H, W = 9, 21
    m8, m32 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.int32)
    table = np.full(16 + 8 * 5 + 8, 0xEE, np.uint8)
    base = table.ctypes.data + (-table.ctypes.data) % 8

    def enc(map8=m8.ctypes.data, map32=None, max_runs=4, tab=base, H=H, W=W):
        return lib.tdnet_op_runs(None, 0, 0, 0, H, W, None, map8, map32, max_runs, tab, None)

    for kw, word in (({"tab": base + 1}, "runs_dev"), ({"tab": base + 4}, "8-byte aligned"), ({"tab": None}, "runs_dev is NULL"), ({"max_runs": 0}, "max_runs"),
                     ({"max_runs": H * W + 1}, "max_runs"), ({"map8": None}, "exactly one"), ({"map32": m32.ctypes.data}, "exactly one"),
                     ({"map8": None, "map32": m32.ctypes.data + 2}, "4-byte aligned"), ({"H": 0}, "size"), ({"H": 65536}, "65535")):
        assert enc(**kw) != 0 and word.encode() in lib.tdnet_last_error(), (kw, lib.tdnet_last_error())
    assert (table == 0xEE).all()
    assert lib.tdnet_op_runs_decode(base + 2, 4, 0, H, W, m8.ctypes.data, None, None) != 0 and b"runs_dev" in lib.tdnet_last_error()
    assert lib.tdnet_op_runs_decode(base, 4, 0, H, W, None, m32.ctypes.data + 1, None) != 0 and b"4-byte aligned" in lib.tdnet_last_error()
    assert lib.tdnet_op_runs_decode(base, 4, 0, H, W, None, None, None) != 0 and b"exactly one" in lib.tdnet_last_error()
    lib.check(enc())                                                   # and the same arguments as they should be: 9 runs against 4 records
    hdr, recs = run_table(table[base - table.ctypes.data:][:16 + 8 * 5])
    assert (int(hdr["count"]), int(hdr["stored"]), int(hdr["status"])) == (H, 4, RUNS_OVERFLOW) and list(recs["start"]) == [0, W, 2 * W, 3 * W, 4 * W]
    assert (table[base - table.ctypes.data + 16 + 8 * 5:] == 0xEE).all()


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
H, W, HS, WS, T = 33, 65, 41, 83, 4
MAXR = H * W


def _engine(lib, model):
    name = {4: "td4", 2: "td2"}[model]
    spec = arch.model_spec(name, 19, "resnet18")
    e = Engine(model, 18, 19, H, W, 0, lib=lib, arch={})
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


@pytest.fixture(scope="module", params=[2, 4], ids=["td2", "td4"])
def clip(lib, request):
    """four frames of random bytes at 41x83 with the labels forward_u8_labels gives for them on a handle of its own, and that handle's launch counts"""
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
    yield P, owner, frames, labels, launches
    owner.close()


def _table(max_runs):
    return np.full(2 + max_runs + 1, 0xEEEEEEEEEEEEEEEE, np.uint64)


def test_frames_coded_on_the_device_equal_the_oracle_on_their_labels(clip):
    P, owner, frames, labels, launches = clip
    a = owner.share()
    a.set_input_u8(HS, WS)
    assert a.runs_bytes() == 0
    a.set_runs(MAXR)
    assert a.runs_bytes() == 16 + 8 * (MAXR + 1)
    for t, src in enumerate(frames):
        l8, table = np.full((H, W), 0xEE, np.uint8), _table(MAXR)
        a.forward_u8_runs(src, t % P, l8 if t % 2 == 0 else None, table)
        assert a.last_launch_count() == launches[t] - 1 + LAUNCHES, t
        assert np.array_equal(l8, labels[t]) if t % 2 == 0 else (l8 == 0xEE).all()
        count = cases.check_frame_table(table, labels[t], MAXR, ("frame", t))
        assert (table[2 + count + 1:] == 0xEEEEEEEEEEEEEEEE).all()     # nothing behind the closing record
        a.set_runs(MAXR)                                               # idempotent
        table2 = _table(MAXR)
        a.labels_runs(labels[t], table2)                               # the unfused form on those labels: the same table
        assert a.last_launch_count() == launches[t] - 1 + LAUNCHES     # ... outside the frame's count
        assert np.array_equal(table2, table)
        back = np.full((H, W), 0xEE, np.uint8)
        a.runs_labels(table, 0, back)
        assert np.array_equal(back, labels[t])
    assert a.fifo_len() == owner.fifo_len()
    a.close()


def test_split_frames_the_fp32_entry_and_max_runs_read_at_enqueue(clip):
    P, owner, frames, labels, launches = clip
    c, ref = owner.share(), owner.share()
    c.set_input_u8(HS, WS)
    ref.set_input_u8(HS, WS)
    x = weights.synth_video(H, W, T, seed=5)
    for t, src in enumerate(frames):
        maxr = (MAXR, 40)[t % 2]
        c.set_runs(maxr)
        l8, table = np.full((H, W), 0xEE, np.uint8), _table(maxr)
        if t % 3 == 2:
            l32 = np.full((H, W), -1, np.int32)
            ref.forward_labels(x[t], t % P, l32)
            want = l32.astype(np.uint8)
        else:
            want = np.full((H, W), 0xEE, np.uint8)
            ref.forward_u8_labels(src, t % P, want)
        if t % 3 == 0:
            c.encode_u8(src, t % P)
            c.propagate_runs(l8, table)
        elif t % 3 == 1:
            c.forward_u8_runs(src, t % P, l8, table)
        else:
            c.forward_runs(x[t], t % P, l8, table)
        if t % 3:
            assert c.last_launch_count() == ref.last_launch_count() - 1 + LAUNCHES, t
        assert np.array_equal(l8, want), t
        count = cases.check_frame_table(table, want, maxr, ("mixed frame", t))
        back = np.full((H, W), 0xEE, np.uint8)
        c.runs_labels(table, 0xAB, back)
        hdr, recs = run_table(table)
        assert np.array_equal(back, runs_decode(hdr, recs, H, W, 0xAB, np.uint8)) and (count <= maxr) == np.array_equal(back, want)
        assert c.fifo_len() == ref.fifo_len(), t
    c.close()
    ref.close()


def test_an_id_map_coded_and_decoded(clip):
    """regions, then ids_runs on the id map, decoded back to it; a map of arbitrary int32 values the same way"""
    P, owner, frames, labels, launches = clip
    e = owner.share()
    e.set_regions(tuple(range(19)), 8, 4096, 1)
    e.set_runs(MAXR)
    ids, rtable = np.full((H, W), -7, np.int32), np.zeros(e.regions_bytes() // 8, np.uint64)
    e.labels_regions(labels[0], ids, rtable)
    assert ids.max() > 1
    for m in (ids, cases.pattern("extremes", H, W, B, True)):
        table, back = _table(MAXR), np.full((H, W), -7, np.int32)
        e.ids_runs(m, table)
        hdr, recs = run_table(table)
        whdr, wrecs = runs_of(m)
        assert np.array_equal(recs, wrecs) and int(hdr["count"]) == int(whdr["count"])
        e.runs_ids(table, 0, back)
        assert np.array_equal(back, m)
    e.close()


def test_errors_leave_the_fifo_and_a_pending_frame_alone(lib, clip):
    P, owner, frames, labels, launches = clip
    e = owner.share()
    x = np.zeros((1, 3, H, W), np.float32)
    e.set_input_u8(HS, WS)
    e.encode_u8(frames[0], 0)                                          # a pending frame: every failure below must leave it pending
    l8, ids = np.full((H, W), 0xEE, np.uint8), np.full((H, W), -7, np.int32)
    table = _table(4)
    for call in (lambda: e.forward_runs(x, 1, l8, table), lambda: e.forward_u8_runs(frames[1], 1, l8, table), lambda: e.propagate_runs(l8, table),
                 lambda: e.labels_runs(labels[0], table), lambda: e.ids_runs(ids, table), lambda: e.runs_labels(table, 0, l8), lambda: e.runs_ids(table, 0, ids)):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_runs"):  # a shared handle is unconfigured until it is configured itself
            call()
    _, before, _ = e.memory_bytes()
    for bad in (0, -1, H * W + 1):
        with pytest.raises(_capi.TdnetError, match="max_runs"):
            e.set_runs(bad)
    assert e.runs_bytes() == 0 and e.memory_bytes()[1] == before        # nothing changed
    e.set_runs(4)
    nblk = (H * W // 4 + 2 + 255) // 256
    assert e.runs_bytes() == 16 + 8 * 5 and e.memory_bytes()[1] == before + H * W + 4 * nblk   # the workspace is counted
    e.set_runs(H * W)
    e.set_runs(4)
    assert e.memory_bytes()[1] == before + H * W + 4 * nblk             # ... once
    odd = table.view(np.uint8)[4:]
    for call in (lambda: e.forward_u8_runs(frames[1], 1, l8, odd), lambda: e.propagate_runs(l8, odd), lambda: e.labels_runs(labels[0], odd),
                 lambda: e.forward_runs(x, 1, l8, odd), lambda: e.ids_runs(ids, odd), lambda: e.runs_labels(odd, 0, l8), lambda: e.runs_ids(odd, 0, ids)):
        with pytest.raises(_capi.TdnetError, match="runs_dev = 0x[0-9a-f]+ is not 8-byte aligned"):
            call()
    for call in (lambda: e.propagate_runs(l8, None), lambda: e.labels_runs(labels[0], None), lambda: e.runs_ids(None, 0, ids)):
        with pytest.raises(_capi.TdnetError, match="runs_dev is NULL"):
            call()
    with pytest.raises(_capi.TdnetError, match="ids_dev = 0x[0-9a-f]+ is not 4-byte aligned"):
        e.ids_runs(ids.view(np.uint8).reshape(-1)[2:].ctypes.data, table)
    for call in (lambda: e.labels_runs(None, table), lambda: e.ids_runs(None, table), lambda: e.runs_labels(table, 0, None)):
        with pytest.raises(_capi.TdnetError, match="null"):
            call()
    with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):   # the forward forms respect the pending frame like their siblings
        e.forward_u8_runs(frames[1], 1, l8, table)
    assert e.fifo_len() == 0 and (l8 == 0xEE).all() and (table == 0xEEEEEEEEEEEEEEEE).all()
    e.propagate_runs(l8, table)                                        # ... which is still there, and is the frame it was
    assert e.fifo_len() == 1 and np.array_equal(l8, labels[0])
    cases.check_frame_table(table, labels[0], 4)
    with pytest.raises(_capi.TdnetError, match="no encoded frame"):
        e.propagate_runs(l8, table)
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_runs(4)
    fresh.close()
    e.close()
