"""Matte out (include/tdnet.h "matte out"), on the CPU through the kernel emulator: the fused upsample + argmax + matte kernel and the unfused
kernel on full-resolution logits against the labels of tdnet_op_upsample_argmax and the float64 softmax of tdnet_op_upsample's logits
(tests/matte_cases.py has the gate); what the contract makes exact -- every class 255, the empty set 0, the labels, one byte per pixel whatever
the byte offsets -- compared exactly; whole frames against the label entries and tdnet_forward_u8; the set per handle; the error paths."""
import numpy as np
import pytest

import emu_util
import matte_cases as cases
import opcheck
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


_ref = {}


def reference(lib, case):
    """(x, full, labels, {set name: (ids, want, near)}) of a case, through entries that predate the matte entries; computed once, read-only."""
    key = cases.case_id(case)
    if key not in _ref:
        name, C, (h, w), (H, W), scale = case
        x = cases.logits(name, C, h, w, scale)
        full = np.full((C, H, W), np.nan, np.float32)
        lib.check(lib.tdnet_op_upsample(x.ctypes.data, C, h, w, H, W, full.ctypes.data, None))
        l32 = np.full((H, W), -1, np.int32)
        lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
        assert l32.min() >= 0 and l32.max() < C
        sets = {}
        for sname, ids in cases.class_sets(C).items():
            want, near = cases.expected(full, ids, (key, sname))
            want.setflags(write=False)
            near.setflags(write=False)
            sets[sname] = (ids, want, near)
        for a in (full, l32):
            a.setflags(write=False)
        _ref[key] = (x, full, l32, sets)
    return _ref[key]


def holder(n, off):
    """(holder, view): room for n bytes `off` bytes into a holder of 0xEE with 16 guard bytes"""
    hold = np.full(n + 16, 0xEE, np.uint8)
    return hold, hold[off:off + n]


@opcheck.guarded_arg("x", False)
@opcheck.guarded_arg("full", False)
def matte_op(lib, C, H, W, ids, x=None, h=0, w=0, full=None, lab_off=0, mat_off=0, want_labels=True):
    """One call of the operator entry: (labels written or None, matte written).  Either map sits at its byte offset inside a 0xEE holder whose
    guard bytes must survive.  The logits go in between guard bands, once per band fill (opcheck.guarded_arg): the same bytes both times."""
    mh, mv = holder(H * W, mat_off)
    lh = lv = None
    if want_labels:
        lh, lv = holder(H * W, lab_off)
    cls = cases.ids_array(ids)
    lib.check(lib.tdnet_op_upsample_argmax_matte(None if x is None else x.ctypes.data, C, h, w, H, W, None if lv is None else lv.ctypes.data, mv.ctypes.data,
                                                 cls.ctypes.data if len(ids) else None, len(ids), None if full is None else full.ctypes.data, None))
    assert (mh[:mat_off] == 0xEE).all() and (mh[mat_off + H * W:] == 0xEE).all(), (lab_off, mat_off)
    if lh is not None:
        assert (lh[:lab_off] == 0xEE).all() and (lh[lab_off + H * W:] == 0xEE).all(), (lab_off, mat_off)
    return None if lv is None else lv.reshape(H, W), mv.reshape(H, W)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_fused_kernel_every_set_through_the_gate_and_the_exact_properties(lib, case):
    name, C, (h, w), (H, W), scale = case
    x, full, labels, sets = reference(lib, case)
    got = {}
    for i, (sname, (ids, want, near)) in enumerate(sets.items()):
        lab, mat = matte_op(lib, C, H, W, ids, x, h, w, lab_off=i & 3, mat_off=(i + 1) & 3)
        assert np.array_equal(lab, labels), sname                      # whatever the set: the label entries' labels
        cases.gate(mat, want, near, (cases.case_id(case), sname))
        got[sname] = mat.copy()
    assert (got["every"] == 255).all() and (got["empty"] == 0).all()   # exact: num and den share their operations
    if C == 1:
        assert (matte_op(lib, C, H, W, (0,), x, h, w)[1] == 255).all()
    for sname, (ids, want, near) in sets.items():                      # a set and its complement share den: their bytes add up to 255 within the two roundings
        _, comp = matte_op(lib, C, H, W, cases.complement(C, ids), x, h, w, mat_off=2)
        assert np.abs(got[sname].astype(np.int64) + comp - 255).max() <= 1, sname
    if scale >= 6 and C > 1:
        seen = np.concatenate([got[s].ravel() for s in got if s not in ("every", "empty")])
        assert seen.min() == 0 and seen.max() == 255                   # the proper subsets reach both ends of the byte range


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_labels_and_one_byte_per_pixel_at_every_pair_of_alignments(lib, case):
    name, C, (h, w), (H, W), scale = case
    x, full, labels, sets = reference(lib, case)
    sname = "moving" if "moving" in sets else "every"
    ids = sets[sname][0]
    first = None
    for lab_off, mat_off in cases.offsets_of(name):
        lab, mat = matte_op(lib, C, H, W, ids, x, h, w, lab_off=lab_off, mat_off=mat_off)
        assert np.array_equal(lab, labels), (lab_off, mat_off)
        first = mat.copy() if first is None else first
        assert np.array_equal(mat, first), (lab_off, mat_off)          # a pixel's byte does not depend on which lane computed it
    _, mat = matte_op(lib, C, H, W, ids, x, h, w, mat_off=3, want_labels=False)   # labels = NULL: the same matte
    assert np.array_equal(mat, first)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_unfused_kernel_on_full_resolution_logits(lib, case):
    name, C, (h, w), (H, W), scale = case
    x, full, labels, sets = reference(lib, case)
    for sname, (ids, want, near) in sets.items():
        _, fused = matte_op(lib, C, H, W, ids, x, h, w)
        mat = None
        for lab_off, mat_off in cases.FEW_OFFSETS:
            lab, mat = matte_op(lib, C, H, W, ids, full=full, lab_off=lab_off, mat_off=mat_off)
            assert np.array_equal(lab, labels), (sname, lab_off, mat_off)
            cases.gate(mat, want, near, (cases.case_id(case), sname, lab_off, mat_off))
            d = np.abs(mat.astype(np.int64) - fused)
            assert d.max() <= 1 and not (d != 0)[~near].any(), sname
        _, only = matte_op(lib, C, H, W, ids, full=full, mat_off=1, want_labels=False)
        assert np.array_equal(only, mat), sname
        if sname == "every":
            assert (mat == 255).all()
        if sname == "empty":
            assert (mat == 0).all()
    # logits that are not 16-byte aligned (the scalar loads): one float into a holder
    ids, want, near = sets["last"] if "last" in sets else sets["every"]
    hold = np.zeros(full.size + 1, np.float32)
    hold[1:] = full.reshape(-1)
    lab, m1 = matte_op(lib, C, H, W, ids, full=hold[1:])
    lab0, m0 = matte_op(lib, C, H, W, ids, full=full)
    assert np.array_equal(lab, labels) and np.array_equal(lab0, labels) and np.array_equal(m1, m0)


def test_the_last_membership_word_at_256_classes(lib):
    """c256 with a set that contains class 255 and one of classes >= 224 only: a kernel that drops or misplaces word 7 gives 0 where the
    reference does not."""
    for case in [c for c in cases.CASES if c[0] == "c256"]:
        name, C, (h, w), (H, W), scale = case
        x, full, labels, sets = reference(lib, case)
        for sname in ("high", "with_255", "last"):
            ids, want, near = sets[sname]
            assert min(ids) >= 224 or 255 in ids
            _, mat = matte_op(lib, C, H, W, ids, x, h, w, mat_off=1)
            cases.gate(mat, want, near, (cases.case_id(case), sname))
            _, umat = matte_op(lib, C, H, W, ids, full=full, mat_off=2)
            cases.gate(umat, want, near, (cases.case_id(case), sname, "unfused"))
        assert sets["high"][1].max() > 0 and sets["with_255"][1].max() > 0


def test_non_finite_logits_leave_the_labels_alone(lib):
    """The matte byte of such a pixel is unspecified; the labels are still the label entries'."""
    name, C, (h, w), (H, W), scale = cases.CASES[0]
    x = cases.logits(name, C, h, w, scale).copy()
    x[3, 1, 2], x[7, 2, 5], x[0, 4, 8], x[5, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    l32 = np.full((H, W), -1, np.int32)
    lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
    full = np.zeros((C, H, W), np.float32)
    lib.check(lib.tdnet_op_upsample(x.ctypes.data, C, h, w, H, W, full.ctypes.data, None))
    assert not np.isfinite(full).all()
    lab, _ = matte_op(lib, C, H, W, cases.MOVING, x, h, w, lab_off=1, mat_off=3)
    assert np.array_equal(lab, l32)
    lab, _ = matte_op(lib, C, H, W, cases.MOVING, full=full, lab_off=2, mat_off=1)
    assert np.array_equal(lab, l32)


def test_operator_entry_checks_its_arguments(lib):
    x = cases.logits("odd_w", 19, 5, 9, 1)
    lab, mat = np.full((33, 65), 0xEE, np.uint8), np.full((33, 65), 0xEE, np.uint8)
    ok, bad = cases.ids_array((11, 12)), cases.ids_array((11, 19))
    for args in ((x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, None, ok.ctypes.data, 2, None, None),
                 (x.ctypes.data, 257, 5, 9, 33, 65, lab.ctypes.data, mat.ctypes.data, ok.ctypes.data, 2, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, mat.ctypes.data, bad.ctypes.data, 2, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, mat.ctypes.data, ok.ctypes.data, 257, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, mat.ctypes.data, ok.ctypes.data, -1, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, mat.ctypes.data, None, 2, None, None),
                 (None, 19, 5, 9, 33, 65, lab.ctypes.data, mat.ctypes.data, ok.ctypes.data, 2, None, None)):
        with pytest.raises(_capi.TdnetError, match="tdnet_op_upsample_argmax_matte"):
            lib.check(lib.tdnet_op_upsample_argmax_matte(*args))
    assert (lab == 0xEE).all() and (mat == 0xEE).all()


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
H, W, HS, WS = 33, 65, 41, 83


def _engine(lib, model, opts=None):
    name = {4: "td4", 2: "td2"}[model]
    spec = arch.model_spec(name, 19, "resnet18")
    e = Engine(model, 18, 19, H, W, 0, lib=lib, opts=opts, arch={})
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


def _frames(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (HS, WS, 3), dtype=np.uint8) for _ in range(n)]


ODD = tuple(range(1, 19, 2))


@pytest.fixture(scope="module", params=[4, 2], ids=["td4-psp18", "td2-psp18"])
def clip(lib, request):
    """A clip of 2 P + 1 frames of random bytes at 41x83 on synthetic weights at 33x65, with -- from entries that predate the matte entries, each
    on a handle of its own, computed once -- the labels of forward_u8_labels, its launch counts and, from the logits of tdnet_forward_u8, the
    float64 reference of the sets `moving` and `odd`."""
    model = request.param
    P = model
    owner = _engine(lib, model)
    owner.set_input_u8(HS, WS)
    logit_h = owner.share()
    logit_h.set_input_u8(HS, WS)
    frames = _frames(2 * P + 1, 41 + model)
    labels, launches, refs = [], [], []
    for t, src in enumerate(frames):
        l8 = np.full((H, W), 0xEE, np.uint8)
        owner.forward_u8_labels(src, t % P, l8)
        labels.append(l8)
        launches.append(owner.last_launch_count())
        full = np.zeros((19, H, W), np.float32)
        logit_h.forward_u8(src, t % P, full)
        assert np.array_equal(full.argmax(0), l8)
        refs.append({"moving": cases.expected(full, cases.MOVING, ("frame", model, t)), "odd": cases.expected(full, ODD, ("frame odd", model, t))})
    for a in frames + labels:
        a.setflags(write=False)
    yield owner, P, frames, labels, launches, refs
    logit_h.close()
    owner.close()


def test_frames_with_a_matte_equal_the_label_entries_frames(clip):
    owner, P, frames, labels, launches, refs = clip
    a, b = owner.share(), owner.share()
    for e in (a, b):
        e.set_input_u8(HS, WS)
        e.set_matte(cases.MOVING)
    for t, src in enumerate(frames):
        l8, m8 = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
        a.forward_u8_matte(src, t % P, l8, m8)
        assert np.array_equal(l8, labels[t]), t
        cases.gate(m8, refs[t]["moving"][0], refs[t]["moving"][1], ("fused frame", t))
        assert a.last_launch_count() == launches[t] > 0, t
        # b mixes in turn: the matte entry, the label entry, encode + propagate_matte (= the one-call form), matte only
        l2, m2 = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
        if t % 4 == 0:
            b.forward_u8_matte(src, t % P, l2, m2)
        elif t % 4 == 1:
            b.forward_u8_labels(src, t % P, l2)
            m2 = m8
        elif t % 4 == 2:
            b.encode_u8(src, t % P)
            b.propagate_matte(l2, m2)
        else:
            b.forward_u8_matte(src, t % P, None, m2)
            l2 = l8
        assert np.array_equal(l2, l8) and np.array_equal(m2, m8), t    # bit-identical: the FIFO does not care what left the frame
        if t % 4 != 2:
            assert b.last_launch_count() == launches[t], t
    assert a.fifo_len() == b.fifo_len() == owner.fifo_len()
    a.close()
    b.close()


def test_fp32_frames_the_unfused_entry_and_a_set_per_handle(clip):
    owner, P, frames, labels, launches, refs = clip
    a, b = owner.share(), owner.share()
    x = weights.synth_video(H, W, 1, seed=5)[0]
    full = np.zeros((19, H, W), np.float32)
    b.forward(x, 0, full)
    l32 = full.argmax(0)
    want_m, near_m = cases.expected(full, cases.MOVING, "fp32 frame")
    want_o, near_o = cases.expected(full, ODD, "fp32 frame odd")
    a.set_matte(cases.MOVING)
    b.set_matte(ODD + ODD)                                             # per handle; duplicates are legal
    l8, m8 = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    a.forward_matte(x, 0, l8, m8)
    assert np.array_equal(l8, l32)
    cases.gate(m8, want_m, near_m, "fp32 frame")
    ul, um = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    a.logits_matte(full, ul, um)
    cases.gate(um, want_m, near_m, "tdnet_logits_matte")
    assert np.array_equal(ul, l32)
    bl, bm = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    b.logits_matte(full, bl, bm)
    cases.gate(bm, want_o, near_o, "tdnet_logits_matte, the other handle's set")
    assert np.array_equal(bl, l32) and not np.array_equal(bm, um)
    b.logits_matte(full, None, bl)                                     # matte only
    assert np.array_equal(bl, bm)
    a.set_matte(range(19))
    a.logits_matte(full, None, um)
    assert (um == 255).all()
    a.set_matte(())
    a.logits_matte(full, None, um)
    assert (um == 0).all()
    a.close()
    b.close()


@pytest.mark.parametrize("precision", [1, 3])
def test_one_frame_at_other_precisions(lib, precision):
    """one frame each (the emulator is slow at precision 3): labels and matte against tdnet_forward_u8's logits"""
    e = _engine(lib, 2, opts={"precision": precision})
    e.set_input_u8(HS, WS)
    e.set_matte(cases.MOVING)
    r = e.share()
    r.set_input_u8(HS, WS)
    src = _frames(1, 78)[0]
    full, lab, mat = np.zeros((19, H, W), np.float32), np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    r.forward_u8(src, 0, full)
    e.forward_u8_matte(src, 0, lab, mat)
    assert np.array_equal(lab, full.argmax(0)) and e.last_launch_count() == r.last_launch_count() > 0
    want, near = cases.expected(full, cases.MOVING, ("precision", precision))
    cases.gate(mat, want, near, ("precision", precision))
    r.close()
    e.close()


def test_errors_name_their_entry_and_leave_a_pending_frame_alone(lib, clip):
    owner, P, frames, labels, launches, refs = clip
    e = owner.share()
    e.set_input_u8(HS, WS)
    x = np.zeros((1, 3, H, W), np.float32)
    full = np.zeros((19, H, W), np.float32)
    lab, mat = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    e.encode_u8(frames[0], 0)                                          # a pending frame: every failure below must leave it pending
    for name, call in (("tdnet_forward_matte", lambda: e.forward_matte(x, 1, lab, mat)),      # a shared handle's set is unset at creation
                       ("tdnet_forward_u8_matte", lambda: e.forward_u8_matte(frames[1], 1, lab, mat)),
                       ("tdnet_propagate_matte", lambda: e.propagate_matte(lab, mat)),
                       ("tdnet_logits_matte", lambda: e.logits_matte(full, lab, mat))):
        with pytest.raises(_capi.TdnetError, match=name + ".*tdnet_set_matte"):
            call()
    assert e.fifo_len() == 0 and (lab == 0xEE).all() and (mat == 0xEE).all()
    e.set_matte(cases.MOVING)
    for bad in ((11, 19), (255,), range(257)):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_matte|set_matte"):
            e.set_matte(bad)
    for name, call in (("tdnet_forward_matte", lambda: e.forward_matte(x, 1, lab, None)),
                       ("tdnet_forward_u8_matte", lambda: e.forward_u8_matte(frames[1], 1, lab, None)),
                       ("tdnet_propagate_matte", lambda: e.propagate_matte(lab, None)),
                       ("tdnet_logits_matte", lambda: e.logits_matte(full, lab, None)),
                       ("tdnet_logits_matte", lambda: e.logits_matte(None, lab, mat))):
        with pytest.raises(_capi.TdnetError, match=name + ": null"):
            call()
    with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_matte.*waiting for tdnet_propagate"):   # the forward forms respect the pending frame
        e.forward_u8_matte(frames[1], 1, lab, mat)
    with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_matte"):
        e.forward_u8_matte(frames[1], P, lab, mat)                     # pos_id out of range
    assert e.fifo_len() == 0 and (lab == 0xEE).all() and (mat == 0xEE).all()
    e.propagate_matte(lab, mat)                                        # ... which is still there, is the frame it was, under the set the failed calls left alone
    assert e.fifo_len() == 1 and np.array_equal(lab, labels[0])
    cases.gate(mat, refs[0]["moving"][0], refs[0]["moving"][1], "pending frame")
    with pytest.raises(_capi.TdnetError, match="tdnet_propagate.*no encoded frame"):
        e.propagate_matte(lab, mat)
    assert e.fifo_len() == 1
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    fresh.set_matte(cases.MOVING)                                      # plain host state: no device, no weights needed
    for name, call in (("tdnet_forward_matte", lambda: fresh.forward_matte(x, 0, lab, mat)),
                       ("tdnet_propagate_matte", lambda: fresh.propagate_matte(lab, mat)),
                       ("tdnet_logits_matte", lambda: fresh.logits_matte(full, lab, mat))):
        with pytest.raises(_capi.TdnetError, match=name + ".*not finalized"):
            call()
    fresh.close()
    e.close()


# ---- the composite, operator level ---------------------------------------------------------------------------------------------------------
class HostMem:
    """The shared scenarios' memory (tests/matte_cases.py): numpy arrays stand in for HBM."""
    stream = None

    def up(self, a, off=0):
        flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        holder = np.full(flat.size + 64, 0xA5, np.uint8)
        holder[off:off + flat.size] = flat
        return holder, holder.ctypes.data + off

    def get(self, buf):
        return buf


MEM = HostMem()
_mattes = {}


def comp_inputs(lib):
    """(keepalive, address of the logits [19, 5, 9], {set name: (ids, the matte operator's bytes [33, 65])}), computed once"""
    if not _mattes:
        x = cases.logits("odd_w", 19, 5, 9, 6)
        keep, px = MEM.up(x)
        sets = {}
        for sname, ids in (("moving", cases.MOVING), ("every", tuple(range(19))), ("empty", ())):
            _, m = cases.matte_op(lib, MEM, 19, 33, 65, ids, px, 5, 9, want_labels=False)
            m.setflags(write=False)
            sets[sname] = (ids, m)
        assert (sets["every"][1] == 255).all() and (sets["empty"][1] == 0).all() and len(np.unique(sets["moving"][1])) > 100
        _mattes["v"] = (keep, x, sets)                                # the ARRAY: op_composite puts it between guard bands, once per band fill
    return _mattes["v"]


@pytest.mark.parametrize("kind", cases.SOURCE_KINDS)
@pytest.mark.parametrize("size", list(cases.SIZES), ids=list(cases.SIZES))
def test_composite_into_the_block_over_every_source_form(lib, size, kind):
    keep, px, sets = comp_inputs(lib)
    src = cases.comp_source(kind, cases.SIZES[size])
    ids, m = sets["moving"]
    cases.check_composite(lib, MEM, src, None, m, cases.BG, px, ids, what=(size, kind))
    if size == "up_41x83":                                             # M = 255 reproduces the source, M = 0 the background, exactly
        for sname in ("every", "empty"):
            ids, m = sets[sname]
            cases.check_composite(lib, MEM, src, None, m, cases.BG, px, ids, offsets=(1,), fills=(0xA5,), what=(size, kind, sname))
        out, host, base = cases.op_composite(lib, MEM, src, 0, None, np.zeros(3 * 41 * 83, np.uint8), 0, cases.BG, x=px, ids=tuple(range(19)))
        want = src[2][..., ::-1] if src[3] else src[2]
        assert np.array_equal(out[base:base + want.size].reshape(want.shape), want)
        out, host, base = cases.op_composite(lib, MEM, src, 0, None, np.zeros(3 * 41 * 83, np.uint8), 0, cases.BG, x=px, ids=())
        bg = cases.BG[::-1] if src[3] else cases.BG
        assert (out[base:base + want.size].reshape(-1, 3) == np.array(bg, np.uint8)).all()


@pytest.mark.parametrize("kind", ("rgb24", "bgra32", "nv12", "p010"))
@pytest.mark.parametrize("dst", list(cases.PACKED))
def test_composite_into_every_packed_view_and_the_alpha_mode(lib, dst, kind):
    keep, px, sets = comp_inputs(lib)
    size = cases.SIZES["up_41x83"]
    src = cases.comp_source(kind, size)
    dview = cases.comp_dest(cases.PACKED[dst], size)
    for sname in ("moving", "every", "empty"):
        ids, m = sets[sname]
        offs = range(4) if sname == "moving" else (2,)
        cases.check_composite(lib, MEM, src, dview, m, cases.BG, px, ids, offsets=offs, what=(dst, kind, sname))
        if dst in ("rgba32", "bgra32"):
            cases.check_composite(lib, MEM, src, dview, m, None, px, ids, offsets=offs, what=(dst, kind, sname, "alpha"))


def test_composite_operator_checks_its_arguments(lib):
    keep, px, sets = comp_inputs(lib)
    size = cases.SIZES["up_41x83"]
    src = cases.comp_source("rgb24", size)
    block = np.full(3 * 41 * 83, 0xEE, np.uint8)
    for dview, bg, match in ((None, None, "TDNET_COMPOSITE_ALPHA.*contiguous"), (cases.comp_dest(cases.PACKED["rgb24"], size), None, "TDNET_COMPOSITE_ALPHA.*RGB24"),
                             (cases.comp_dest(cases.PACKED["rgba32"], (40, 83)), cases.BG, "41 x 83.*40 x 83")):
        n = block.size if dview is None else cases.view_extent(dview)
        with pytest.raises(_capi.TdnetError, match="tdnet_op_composite.*" + match):
            cases.op_composite(lib, MEM, src, 0, dview, np.full(n, 0xEE, np.uint8), 0, bg, x=px, ids=cases.MOVING)
    from tdnet_amd.dataloader import SourceView
    nv = SourceView(cases.PIX_NV12, 60, 100, pitch=100, crop=(2, 4, 41, 83))
    with pytest.raises(_capi.TdnetError, match="tdnet_op_composite.*4:2:0 is not built"):
        cases.op_composite(lib, MEM, src, 0, nv, np.full(cases.view_extent(nv), 0xEE, np.uint8), 0, cases.BG, x=px, ids=cases.MOVING)
    with pytest.raises(_capi.TdnetError, match="tdnet_op_composite.*class id"):
        cases.op_composite(lib, MEM, src, 0, None, block, 0, cases.BG, x=px, ids=(19,))
    with pytest.raises(_capi.TdnetError, match="tdnet_op_composite.*logits"):
        cases.op_composite(lib, MEM, src, 0, None, block, 0, cases.BG, x=None, ids=cases.MOVING)


# ---- the composite, whole frames -----------------------------------------------------------------------------------------------------------
def test_frames_composited_equal_the_oracle_over_the_same_frames_matte(clip):
    from tdnet_amd.dataloader import PIX_BGRA32, composite_u8, view_extent
    owner, P, frames, labels, launches, refs = clip
    a, b, c = owner.share(), owner.share(), owner.share()
    dview = cases.comp_dest(PIX_BGRA32, (HS, WS))
    n = view_extent(dview)
    for e in (a, b, c):
        e.set_matte(cases.MOVING)
    a.set_input_u8(HS, WS)
    b.set_output_composite(cases.BG)                                   # before the byte input: the tables follow it
    b.set_input_u8(HS, WS)
    mem0 = b.memory_bytes()[1]
    b.set_output_composite(cases.BG)                                   # idempotent
    b.set_output_overlay(np.array([[1, 2, 3, 4]], np.uint8))           # independent of the overlay; the tables are counted once
    assert b.memory_bytes()[1] == mem0 + 256 * 4
    c.set_input_u8(HS, WS)
    c.set_output_composite(None)                                       # the alpha mode into a BGRA32 view
    c.set_output_view(dview)
    for t, src in enumerate(frames):
        l8, m8 = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
        a.forward_u8_matte(src, t % P, l8, m8)
        hold = np.full(3 * HS * WS + 32, 0xEE, np.uint8)
        out = hold[16 + (t & 3):16 + (t & 3) + 3 * HS * WS]
        if t % 2 == 0:
            b.forward_u8_composite(src, t % P, out)
            assert b.last_launch_count() == launches[t], t
        else:
            b.encode_u8(src, t % P)
            b.propagate_composite(src, out)
        want = composite_u8(src, m8, H, W, cases.BG)
        assert np.array_equal(out.reshape(HS, WS, 3), want), t
        assert (hold[:16 + (t & 3)] == 0xEE).all() and (hold[16 + (t & 3) + 3 * HS * WS:] == 0xEE).all()
        un = np.full((HS, WS, 3), 0xEE, np.uint8)
        b.matte_composite(m8, src, un)                                 # the unfused entry on the matte entry's bytes
        assert np.array_equal(un, want), t
        prefill = np.full(n, 0xA5, np.uint8)
        dst = prefill.copy()
        c.forward_u8_composite(src, t % P, dst)
        assert c.last_launch_count() == launches[t], t
        rgba = composite_u8(src, m8, H, W, None)
        assert np.array_equal(dst, cases.expected_dest(prefill, dview, np.ascontiguousarray(rgba[..., :3]), rgba[..., 3])), t
    assert a.fifo_len() == b.fifo_len() == c.fifo_len() == owner.fifo_len()
    for e in (a, b, c):
        e.close()


def test_composite_errors_name_the_missing_call_or_field_and_leave_a_pending_frame_alone(lib, clip):
    from tdnet_amd.dataloader import PIX_NV12, PIX_RGB24, PIX_RGBA32, SURF_NV12, SourceView, view_extent
    import surface_cases as sc
    owner, P, frames, labels, launches, refs = clip
    e = owner.share()
    out = np.full((HS, WS, 3), 0xEE, np.uint8)
    big = np.full(200 * 400 * 4, 0xEE, np.uint8)
    src = frames[0]
    with pytest.raises(_capi.TdnetError, match="tdnet_set_output_composite.*bg_rgb"):
        e.lib.check(e.lib.tdnet_set_output_composite(e.h, 0, None))
    with pytest.raises(_capi.TdnetError, match="tdnet_set_output_composite.*bg_rgb"):
        e.lib.check(e.lib.tdnet_set_output_composite(e.h, 1, out.ctypes.data))
    with pytest.raises(_capi.TdnetError, match="tdnet_set_output_composite.*mode"):
        e.lib.check(e.lib.tdnet_set_output_composite(e.h, 2, None))
    e.set_input_u8(HS, WS)
    e.encode_u8(src, 0)                                                # a pending frame: every failure below must leave it pending

    def refused(match, unfused=True):
        calls = [lambda: e.forward_u8_composite(frames[1], 1, big), lambda: e.propagate_composite(src, big)]
        if unfused:
            calls.append(lambda: e.matte_composite(labels[0], src, big))
        for call in calls:
            with pytest.raises(_capi.TdnetError, match=match):
                call()
        assert e.fifo_len() == 0 and (big == 0xEE).all()

    refused("tdnet_set_matte", unfused=False)
    e.set_matte(cases.MOVING)
    refused("tdnet_set_output_composite")
    e.set_output_composite(None)
    refused("TDNET_COMPOSITE_ALPHA.*contiguous")                        # the alpha mode without a view
    e.set_output_view(SourceView(PIX_RGB24, 60, 100, pitch=333, crop=(2, 4, HS, WS)))
    refused("TDNET_COMPOSITE_ALPHA.*RGB24")                             # ... and with a 24-bit one
    e.set_output_composite(cases.BG)
    e.set_output_view(SourceView(PIX_NV12, 60, 100, pitch=100, crop=(2, 4, HS, WS)))
    refused("NV12 view.*4:2:0 is not built")
    e.set_output_surface(sc.surface(SURF_NV12, (2, 4, HS, WS), "padded", frame=(60, 100)))
    refused("surface.*4:2:0 is not built")
    e.set_output_view(SourceView(PIX_RGBA32, 60, 100, pitch=405, crop=(2, 4, HS - 1, WS)))
    refused("41 x 83.*40 x 83")
    e.set_output_view(None)
    hold = np.zeros(2 * 3 * HS * WS, np.uint8)
    hold[:src.size] = src.reshape(-1)
    for call in (lambda: e.propagate_composite(hold, hold[src.size - 1:]), lambda: e.matte_composite(labels[0], hold, hold[5:]),
                 lambda: e.forward_u8_composite(hold, 1, hold[src.size - 1:])):
        with pytest.raises(_capi.TdnetError, match="overlaps"):
            call()
    assert e.fifo_len() == 0
    l8, m8 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    e.propagate_composite(src, out)                                    # ... which is still there, and is the frame it was
    from tdnet_amd.dataloader import composite_u8
    r = owner.share()
    r.set_input_u8(HS, WS)
    r.set_matte(cases.MOVING)
    r.forward_u8_matte(src, 0, l8, m8)
    assert e.fifo_len() == 1 and np.array_equal(out, composite_u8(src, m8, H, W, cases.BG))
    with pytest.raises(_capi.TdnetError, match="tdnet_propagate.*no encoded frame"):
        e.propagate_composite(src, out)
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="tdnet_set_output_composite.*not finalized"):
        fresh.set_output_composite(cases.BG)
    for name, call in (("tdnet_forward_u8_composite", lambda: e.forward_u8_composite(None, 0, out)), ("tdnet_propagate_composite", lambda: e.propagate_composite(src, None)),
                       ("tdnet_matte_composite", lambda: e.matte_composite(None, src, out))):
        with pytest.raises(_capi.TdnetError, match=name + ": null"):
            call()
    fresh.close()
    r.close()
    e.close()
