"""Regions out (include/tdnet.h "regions out"), on the CPU through the kernel emulator: the seven launches of csrc/td_regions.h through
tdnet_op_regions against the flood-fill oracle on every pattern and size of tests/regions_cases.py, between guard bands; the fused form against the
labels of tdnet_op_upsample_argmax; whole frames at 33x65 against the same frames asked for as labels; the error paths.  Every comparison is exact."""
import numpy as np
import pytest

import emu_util
import opcheck
import out_cases
import regions_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import REGIONS_BOUND
from tdnet_amd.engine import Engine

LAUNCHES = 7                                                           # include/tdnet.h TDNET_REGIONS_LAUNCHES


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


TH, TW = 16, 64                                                        # csrc/td_regions.h's tile: the shapes are sized from it at collection, and ...


@pytest.fixture(scope="module")
def tile(lib):
    assert cases.tile(lib) == (TH, TW)                                 # ... held to the library's own answer here
    return TH, TW


@pytest.mark.parametrize("shape", cases.shapes(TH, TW), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.PATTERNS)
def test_patterns_against_the_flood_fill(lib, tile, name, shape):
    counts = cases.check_pattern(lib, opcheck.GuardedNumpyMem(), name, shape[0], shape[1], *tile)
    H, W = shape
    if name == "one":
        assert counts == [1, 1]
    if name == "checker" and H * W > 1:
        assert counts[0] == H * W and counts[1] == (2 if min(H, W) > 1 else H * W)
    if name == "two_classes" and W > 1:
        assert counts == [2, 2]
    if name in ("diag_back", "diag_fwd") and min(H, W) > 1:
        assert counts[0] > counts[1] >= 1                             # 4 neighbours: a region per pixel; 8: a region per line
    if name == "spiral":
        assert counts[1] == 1 or min(H, W) < 3
    if name == "comb":
        assert counts == [1, 1]


def test_overflow_sets_the_status_bit_and_ids_run_on(lib, tile):
    """the checkerboard of two member classes at 4 neighbours: H W regions against 64 records"""
    H, W = 33, 65
    labels, classes = cases.pattern("checker", H, W, *tile)
    ids, hdr, recs, _ = cases.run_op(lib, opcheck.GuardedNumpyMem(), H, W, classes, 4, 64, 1, labels=labels)
    assert cases.compare((ids, hdr, recs), labels, classes, 4, 1, 64) == H * W
    assert int(hdr["status"]) == 1 and int(hdr["stored"]) == 64 and np.array_equal(ids.reshape(-1), np.arange(1, H * W + 1))


def test_parameters_on_the_noise_map(lib):
    cases.check_parameters(lib, opcheck.GuardedNumpyMem(), 33, 65)


@pytest.mark.parametrize("field", out_cases.FIELDS)
@pytest.mark.parametrize("case", out_cases.CASES, ids=out_cases.case_id)
def test_from_logits_the_labels_are_the_label_kernels(lib, case, field):
    C, (h, w), (H, W) = case
    x = out_cases.logits(field, C, h, w)
    l32 = np.full((H, W), -1, np.int32)
    lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
    cases.check_from_logits(lib, opcheck.GuardedNumpyMem(), x, C, h, w, H, W, l32.astype(np.uint8))


def test_operator_entry_checks_its_arguments(lib):
    H, W = 9, 21
    labels = np.zeros((H, W), np.uint8)
    ids = np.full((H, W), -7, np.int32)
    table = np.full(16 + 48 * 4 + 8, 0xEE, np.uint8)
    base = table.ctypes.data + (-table.ctypes.data) % 8
    cls = np.array([3], np.uint8)
    ok = (None, 19, 0, 0, H, W, labels.ctypes.data, None, cls.ctypes.data, 1, 8, 4, 1, ids.ctypes.data, base, None)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.tdnet_op_regions(*a)

    for kw, word in (({"a14": base + 1}, "regions_dev"), ({"a14": base + 4}, "8-byte aligned"), ({"a14": None}, "regions_dev"), ({"a10": 6}, "connectivity"),
                     ({"a11": 0}, "max_regions"), ({"a11": 65537}, "max_regions"), ({"a12": 0}, "min_area"), ({"a1": 257}, "tdnet_op_regions"),
                     ({"a6": None}, "tdnet_op_regions"), ({"a8": np.array([19], np.uint8).ctypes.data}, "not a class id")):
        assert call(**kw) != 0 and word.encode() in lib.tdnet_last_error(), (kw, lib.tdnet_last_error())
    assert (ids == -7).all() and (table == 0xEE).all()
    lib.check(call())                                                  # and the same arguments as they should be
    assert not ids.any() and not table[base - table.ctypes.data:][:16 + 48 * 4].any()


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
H, W, HS, WS, T = 33, 65, 41, 83, 4
CLASSES, CONN, MAXR, MIN_AREA = (0, 2, 5, 8, 11, 13, 17), 8, 64, 2


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
    rng = np.random.default_rng(29)
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


def _buffers(e):
    n = e.regions_bytes()
    return np.full((H, W), 0xEE, np.uint8), np.full((H, W), -7, np.int32), np.full(n // 8, 0xEEEEEEEEEEEEEEEE, np.uint64)


def test_frames_labelled_on_the_device_equal_the_oracle_on_their_labels(clip):
    P, owner, frames, labels, launches = clip
    a = owner.share()
    a.set_input_u8(HS, WS)
    a.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
    assert a.regions_bytes() == 16 + 48 * MAXR
    total = 0
    for t, src in enumerate(frames):
        l8, ids, table = _buffers(a)
        a.forward_u8_regions(src, t % P, l8 if t % 2 == 0 else None, ids if t % 3 else None, table)
        assert a.last_launch_count() == launches[t] - 1 + LAUNCHES, t
        assert np.array_equal(l8, labels[t]) if t % 2 == 0 else (l8 == 0xEE).all()
        total += cases.check_frame_regions((ids if t % 3 else None, table), labels[t], CLASSES, CONN, MIN_AREA, MAXR, ("frame", t))
        if not t % 3:
            assert (ids == -7).all()
        a.set_regions(CLASSES, CONN, MAXR, MIN_AREA)                   # idempotent
        ids2, table2 = np.full((H, W), -7, np.int32), np.full(table.size, 7, np.uint64)
        a.labels_regions(labels[t], ids2, table2)                      # the unfused form on those labels: the same table
        assert a.last_launch_count() == launches[t] - 1 + LAUNCHES     # ... outside the frame's count
        assert np.array_equal(table2, table) and (t % 3 == 0 or np.array_equal(ids2, ids))
    assert a.fifo_len() == owner.fifo_len() and total > 0
    a.close()


def test_split_frames_the_fp32_entry_and_the_configuration_read_at_enqueue(clip, lib):
    """encode_u8 + propagate_regions, forward_u8_regions and the fp32 entry in turn on ONE handle; the set and the limits are those in force at the call"""
    P, owner, frames, labels, launches = clip
    c, ref = owner.share(), owner.share()                              # ref: the same sequence of frames through the label entries
    c.set_input_u8(HS, WS)
    ref.set_input_u8(HS, WS)
    x = weights.synth_video(H, W, T, seed=5)
    for t, src in enumerate(frames):
        conn, maxr, mina = (4, 8)[t % 2], (MAXR, 3)[t % 2], (1, MIN_AREA)[t % 2]
        c.set_regions(CLASSES, conn, maxr, mina)
        l8, ids, table = _buffers(c)
        if t % 3 == 2:
            l32 = np.full((H, W), -1, np.int32)
            ref.forward_labels(x[t], t % P, l32)
            want = l32.astype(np.uint8)
        else:
            want = np.full((H, W), 0xEE, np.uint8)
            ref.forward_u8_labels(src, t % P, want)
        if t % 3 == 0:
            c.encode_u8(src, t % P)
            c.propagate_regions(l8, ids, table)
        elif t % 3 == 1:
            c.forward_u8_regions(src, t % P, l8, ids, table)
        else:
            c.forward_regions(x[t], t % P, l8, ids, table)
        if t % 3:
            assert c.last_launch_count() == ref.last_launch_count() - 1 + LAUNCHES, t
        assert np.array_equal(l8, want), t
        cases.check_frame_regions((ids, table), want, CLASSES, conn, mina, maxr, ("mixed frame", t))
        assert c.fifo_len() == ref.fifo_len(), t
    c.close()
    ref.close()


def test_rejected_pixels_are_in_no_region(clip):
    """the confidence entry's labels (rejected pixels are 255) handed to the unfused entry: 255 is background"""
    P, owner, frames, labels, launches = clip
    e, probe = owner.share(), owner.share()
    l8, conf = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    probe.set_input_u8(HS, WS)
    probe.forward_u8_labels_conf(frames[0], 0, l8, conf)               # nothing rejected: the frame's confidence bytes, for a threshold that splits them
    probe.close()
    e.set_input_u8(HS, WS)
    e.set_confidence(int(np.median(conf)) + 1, 255)
    e.set_regions(tuple(range(19)), 8, 256, 1)
    e.forward_u8_labels_conf(frames[0], 0, l8, conf)
    assert 0 < (l8 == 255).sum() < H * W
    _, ids, table = _buffers(e)
    e.labels_regions(l8, ids, table)
    cases.check_frame_regions((ids, table), l8, tuple(range(19)), 8, 1, 256)
    assert not ids[l8 == 255].any() and (ids[l8 != 255] > 0).all()
    e.close()


def test_errors_leave_the_fifo_and_a_pending_frame_alone(lib, clip):
    P, owner, frames, labels, launches = clip
    e = owner.share()
    x = np.zeros((1, 3, H, W), np.float32)
    e.set_input_u8(HS, WS)
    e.encode_u8(frames[0], 0)                                          # a pending frame: every failure below must leave it pending
    l8, ids = np.full((H, W), 0xEE, np.uint8), np.full((H, W), -7, np.int32)
    table = np.full(2 + 6 * 4 + 1, 0xEEEEEEEEEEEEEEEE, np.uint64)
    assert e.regions_bytes() == 0
    for call in (lambda: e.forward_regions(x, 1, l8, ids, table), lambda: e.forward_u8_regions(frames[1], 1, l8, ids, table),
                 lambda: e.propagate_regions(l8, ids, table), lambda: e.labels_regions(labels[0], ids, table)):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_regions"):   # a shared handle is unconfigured until it is configured itself
            call()
    _, before, _ = e.memory_bytes()
    for args, word in ((((3, 19), 8, 4, 1), "not a class id"), (((3,), 6, 4, 1), "connectivity"), (((3,), 8, 0, 1), "max_regions"), (((3,), 8, 65537, 1), "max_regions"),
                       (((3,), 8, 4, 0), "min_area")):
        with pytest.raises(_capi.TdnetError, match=word):
            e.set_regions(*args)
    assert lib.tdnet_set_regions(e.h, None, 2, 8, 4, 1) != 0 and b"classes is NULL" in lib.tdnet_last_error()
    assert lib.tdnet_set_regions(e.h, None, 257, 8, 4, 1) != 0 and b"0..256" in lib.tdnet_last_error()
    assert e.regions_bytes() == 0 and e.memory_bytes()[1] == before     # nothing changed
    e.set_regions(CLASSES, 8, 4, 1)
    nblk = (H * W + 1023) // 1024
    assert e.regions_bytes() == 16 + 48 * 4 and e.memory_bytes()[1] == before + 3 * 4 * H * W + H * W + 4 * nblk + 4   # the workspace is counted
    e.set_regions(CLASSES, 4, 4, 2)
    assert e.memory_bytes()[1] == before + 3 * 4 * H * W + H * W + 4 * nblk + 4                                       # ... once
    odd = table.view(np.uint8)[4:]
    for call in (lambda: e.forward_u8_regions(frames[1], 1, l8, ids, odd), lambda: e.propagate_regions(l8, ids, odd), lambda: e.labels_regions(labels[0], ids, odd),
                 lambda: e.forward_regions(x, 1, l8, ids, odd)):
        with pytest.raises(_capi.TdnetError, match="regions_dev = 0x[0-9a-f]+ is not 8-byte aligned"):
            call()
    with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):   # the forward forms respect the pending frame like their siblings
        e.forward_u8_regions(frames[1], 1, l8, ids, table)
    assert e.fifo_len() == 0 and (l8 == 0xEE).all() and (ids == -7).all() and (table == 0xEEEEEEEEEEEEEEEE).all()
    e.propagate_regions(l8, ids, table[:-1])                           # ... which is still there, and is the frame it was
    assert e.fifo_len() == 1 and np.array_equal(l8, labels[0]) and table[-1] == 0xEEEEEEEEEEEEEEEE
    cases.check_frame_regions((ids, table[:-1]), labels[0], CLASSES, 4, 2, 4)
    with pytest.raises(_capi.TdnetError, match="no encoded frame"):
        e.propagate_regions(l8, ids, table)
    assert lib.tdnet_labels_regions(e.h, None, ids.ctypes.data, table.ctypes.data, None) < 0 and b"null" in lib.tdnet_last_error()
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_regions((3,))
    fresh.close()
    e.close()


def test_the_bound_bit_is_never_set(lib, tile):
    """the deepest chains (the spiral) and the most contended unions (one class) at the largest test size: status bit 1 stays 0"""
    for name in ("spiral", "one", "noise"):
        labels, classes = cases.pattern(name, 128, 256, *tile)
        _, hdr, _, _ = cases.run_op(lib, opcheck.GuardedNumpyMem(), 128, 256, classes, 8, 16, 1, labels=labels, want_ids=False)
        assert not int(hdr["status"]) & REGIONS_BOUND, name
