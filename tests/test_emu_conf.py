"""Confidence out (include/tdnet.h "confidence out"), on the CPU through the kernel emulator: the fused upsample + argmax + confidence kernel and
the unfused kernel on full-resolution logits against the labels of tdnet_op_upsample_argmax and the float64 softmax of tdnet_op_upsample's logits
(tests/conf_cases.py has the gate and where its margin comes from); rejection, which is defined on the byte and therefore compared exactly; whole
frames against the label entries and tdnet_forward; the composition with the score entries; the error paths."""
import numpy as np
import pytest

import opcheck
import conf_cases as cases
import emu_util
import score_cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


_ref = {}


def reference(lib, case):
    """(x, full, labels, want, near) of a case, through entries that predate the confidence entries; computed once, read-only."""
    key = cases.case_id(case)
    if key not in _ref:
        name, C, (h, w), (H, W), scale = case
        x = cases.logits(name, C, h, w, scale)
        full = np.full((C, H, W), np.nan, np.float32)
        lib.check(lib.tdnet_op_upsample(x.ctypes.data, C, h, w, H, W, full.ctypes.data, None))
        l32 = np.full((H, W), -1, np.int32)
        lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
        assert l32.min() >= 0 and l32.max() < C
        want, near = cases.expected(full, key)
        for a in (full, l32, want, near):
            a.setflags(write=False)
        _ref[key] = (x, full, l32, want, near)
    return _ref[key]


def holder(n, off):
    """(holder, view): room for n bytes `off` bytes into a holder of 0xEE with 16 guard bytes"""
    hold = np.full(n + 16, 0xEE, np.uint8)
    return hold, hold[off:off + n]


@opcheck.guarded_arg("x", False)
@opcheck.guarded_arg("full", False)
def conf_op(lib, C, H, W, x=None, h=0, w=0, full=None, lab_off=0, conf_off=0, min_conf=0, reject=255, want_labels=True):
    """One call of the operator entry: (labels written or None, confidence written).  Either map sits at its byte offset inside a 0xEE holder
    whose guard bytes must survive."""
    ch, cv = holder(H * W, conf_off)
    lh = lv = None
    if want_labels:
        lh, lv = holder(H * W, lab_off)
    lib.check(lib.tdnet_op_upsample_argmax_conf(None if x is None else x.ctypes.data, C, h, w, H, W, None if lv is None else lv.ctypes.data, cv.ctypes.data,
                                                min_conf, reject, None if full is None else full.ctypes.data, None))
    assert (ch[:conf_off] == 0xEE).all() and (ch[conf_off + H * W:] == 0xEE).all(), (lab_off, conf_off)
    if lh is not None:
        assert (lh[:lab_off] == 0xEE).all() and (lh[lab_off + H * W:] == 0xEE).all(), (lab_off, conf_off)
    return None if lv is None else lv.reshape(H, W), cv.reshape(H, W)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_fused_kernel_labels_and_confidence_at_every_pair_of_alignments(lib, case):
    name, C, (h, w), (H, W), scale = case
    x, full, labels, want, near = reference(lib, case)
    first = None
    for lab_off, conf_off in cases.offsets_of(name):
        lab, conf = conf_op(lib, C, H, W, x, h, w, lab_off=lab_off, conf_off=conf_off)
        assert np.array_equal(lab, labels), (lab_off, conf_off)        # min_conf = 0: the label entries' labels
        cases.gate(conf, want, near, (cases.case_id(case), lab_off, conf_off))
        first = conf.copy() if first is None else first
        assert np.array_equal(conf, first), (lab_off, conf_off)        # a pixel's byte does not depend on which lane computed it
    _, conf = conf_op(lib, C, H, W, x, h, w, conf_off=3, want_labels=False)   # labels = NULL: the same confidence
    assert np.array_equal(conf, first)
    if C == 1:
        assert (first == 255).all()
    if scale == 6:
        assert first.max() >= 254


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_rejection_is_exact_on_the_bytes_the_kernel_wrote(lib, case):
    name, C, (h, w), (H, W), scale = case
    x, full, labels, want, near = reference(lib, case)
    _, conf0 = conf_op(lib, C, H, W, x, h, w)
    _, uconf0 = conf_op(lib, C, H, W, full=full)
    some = 0
    for i, min_conf in enumerate(cases.thresholds(conf0)):
        for reject in cases.REJECT_LABELS:
            lab, conf = conf_op(lib, C, H, W, x, h, w, lab_off=(i + 1) & 3, conf_off=i & 3, min_conf=min_conf, reject=reject)
            assert np.array_equal(conf, conf0), (min_conf, reject)     # the confidence map is never altered by rejection
            assert np.array_equal(lab, cases.rejected(labels, conf, min_conf, reject)), (min_conf, reject)
            some += int((conf < min_conf).sum())
            lab, conf = conf_op(lib, C, H, W, full=full, lab_off=i & 3, conf_off=(i + 2) & 3, min_conf=min_conf, reject=reject)
            assert np.array_equal(conf, uconf0) and np.array_equal(lab, cases.rejected(labels, conf, min_conf, reject)), (min_conf, reject)
    assert some > 0 or C == 1


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_unfused_kernel_on_full_resolution_logits(lib, case):
    name, C, (h, w), (H, W), scale = case
    x, full, labels, want, near = reference(lib, case)
    _, fused = conf_op(lib, C, H, W, x, h, w)
    for lab_off, conf_off in cases.FEW_OFFSETS:
        lab, conf = conf_op(lib, C, H, W, full=full, lab_off=lab_off, conf_off=conf_off)
        assert np.array_equal(lab, labels), (lab_off, conf_off)
        cases.gate(conf, want, near, (cases.case_id(case), lab_off, conf_off))
        d = np.abs(conf.astype(np.int64) - fused)
        assert d.max() <= 1 and not (d != 0)[~near].any()
    _, only = conf_op(lib, C, H, W, full=full, conf_off=1, want_labels=False)
    assert np.array_equal(only, conf)
    # logits that are not 16-byte aligned (the scalar loads): one float into a holder
    hold = np.zeros(full.size + 1, np.float32)
    hold[1:] = full.reshape(-1)
    lab, conf2 = conf_op(lib, C, H, W, full=hold[1:])
    assert np.array_equal(lab, labels) and np.array_equal(conf2, conf)
    assert (H * W) % 4 != 0 or name in ("w_mult_of_4",)                # the cases cover an H W that is no multiple of 4, and one that is


@pytest.mark.parametrize("passes", ["1", "2"])
@pytest.mark.parametrize("name", ["odd_w", "c256", "ties"])
def test_one_pass_and_two_pass_forms_pass_the_same_gates(lib, name, passes, monkeypatch):
    """TDNET_CONF_PASSES=1 / 2 (read by the operator entry only; tools/conf_probe.py measures with it) picks the kernels' instantiation."""
    monkeypatch.setenv("TDNET_CONF_PASSES", passes)
    for case in [c for c in cases.CASES if c[0] == name]:
        _, C, (h, w), (H, W), scale = case
        x, full, labels, want, near = reference(lib, case)
        for kw in (dict(x=x, h=h, w=w), dict(full=full)):
            lab, conf = conf_op(lib, C, H, W, lab_off=1, conf_off=2, **kw)
            assert np.array_equal(lab, labels)
            cases.gate(conf, want, near, (cases.case_id(case), passes))
            lab, conf1 = conf_op(lib, C, H, W, lab_off=3, conf_off=0, min_conf=128, reject=19, **kw)
            assert np.array_equal(conf1, conf) and np.array_equal(lab, cases.rejected(labels, conf, 128, 19))


def test_non_finite_logits_leave_the_labels_alone(lib):
    """The confidence byte of such a pixel is unspecified; with min_conf = 0 the labels are still the label entries'."""
    name, C, (h, w), (H, W), scale = cases.CASES[0]
    x = cases.logits(name, C, h, w, scale).copy()
    x[3, 1, 2], x[7, 2, 5], x[0, 4, 8], x[5, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    l32 = np.full((H, W), -1, np.int32)
    lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
    full = np.zeros((C, H, W), np.float32)
    lib.check(lib.tdnet_op_upsample(x.ctypes.data, C, h, w, H, W, full.ctypes.data, None))
    assert not np.isfinite(full).all()
    lab, _ = conf_op(lib, C, H, W, x, h, w, lab_off=1, conf_off=3)
    assert np.array_equal(lab, l32)
    lab, _ = conf_op(lib, C, H, W, full=full, lab_off=2, conf_off=1)
    assert np.array_equal(lab, l32)


def test_operator_entry_checks_its_arguments(lib):
    x = cases.logits("odd_w", 19, 5, 9, 1)
    lab, conf = np.full((33, 65), 0xEE, np.uint8), np.full((33, 65), 0xEE, np.uint8)
    for args in ((x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, None, 0, 255, None, None),
                 (x.ctypes.data, 257, 5, 9, 33, 65, lab.ctypes.data, conf.ctypes.data, 0, 255, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, conf.ctypes.data, 256, 255, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, conf.ctypes.data, -1, 255, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, lab.ctypes.data, conf.ctypes.data, 0, 256, None, None),
                 (None, 19, 5, 9, 33, 65, lab.ctypes.data, conf.ctypes.data, 0, 255, None, None)):
        with pytest.raises(_capi.TdnetError, match="tdnet_op_upsample_argmax_conf"):
            lib.check(lib.tdnet_op_upsample_argmax_conf(*args))
    assert (lab == 0xEE).all() and (conf == 0xEE).all()


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


@pytest.fixture(scope="module", params=[4, 2], ids=["td4-psp18", "td2-psp18"])
def clip(lib, request):
    """A clip of 2 P + 1 frames of random bytes at 41x83 on synthetic weights at 33x65, with -- from entries that predate the confidence entries,
    each on a handle of its own, computed once -- the labels of forward_u8_labels, its launch counts and the logits of tdnet_forward_u8."""
    model = request.param
    P = model
    owner = _engine(lib, model)
    owner.set_input_u8(HS, WS)
    logit_h = owner.share()
    logit_h.set_input_u8(HS, WS)
    frames = _frames(2 * P + 1, 31 + model)
    labels, launches, refs = [], [], []
    for t, src in enumerate(frames):
        l8 = np.full((H, W), 0xEE, np.uint8)
        owner.forward_u8_labels(src, t % P, l8)
        labels.append(l8)
        launches.append(owner.last_launch_count())
        full = np.zeros((19, H, W), np.float32)
        logit_h.forward_u8(src, t % P, full)
        assert np.array_equal(full.argmax(0), l8)
        refs.append(cases.expected(full, ("frame", model, t)))
    for a in frames + labels:
        a.setflags(write=False)
    yield owner, P, frames, labels, launches, refs
    logit_h.close()
    owner.close()


def test_frames_with_confidence_equal_the_label_entries_frames(clip):
    owner, P, frames, labels, launches, refs = clip
    a, b = owner.share(), owner.share()
    for e in (a, b):
        e.set_input_u8(HS, WS)
    for t, src in enumerate(frames):
        l8, c8 = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
        a.forward_u8_labels_conf(src, t % P, l8, c8)                    # without tdnet_set_confidence: min_conf = 0
        assert np.array_equal(l8, labels[t]), t
        cases.gate(c8, refs[t][0], refs[t][1], ("fused frame", t))
        assert a.last_launch_count() == launches[t] > 0, t
        # b mixes in turn: the conf entry, the label entry, encode + propagate_labels_conf (= the one-call form), confidence only
        l2, c2 = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
        if t % 4 == 0:
            b.forward_u8_labels_conf(src, t % P, l2, c2)
        elif t % 4 == 1:
            b.forward_u8_labels(src, t % P, l2)
            c2 = c8
        elif t % 4 == 2:
            b.encode_u8(src, t % P)
            b.propagate_labels_conf(l2, c2)
        else:
            b.forward_u8_labels_conf(src, t % P, None, c2)
            l2 = l8
        assert np.array_equal(l2, l8) and np.array_equal(c2, c8), t    # bit-identical: the FIFO does not care what left the frame
        if t % 4 != 2:
            assert b.last_launch_count() == launches[t], t
    assert a.fifo_len() == b.fifo_len() == owner.fifo_len()
    a.close()
    b.close()


def test_fp32_frames_the_unfused_entry_and_a_threshold_per_handle(clip):
    owner, P, frames, labels, launches, refs = clip
    a, b = owner.share(), owner.share()
    x = weights.synth_video(H, W, 1, seed=5)[0]
    full = np.zeros((19, H, W), np.float32)
    b.forward(x, 0, full)
    want, near = cases.expected(full, "fp32 frame")
    l32 = full.argmax(0)
    a.set_confidence(0, 255)
    l8, c8 = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    a.forward_labels_conf(x, 0, l8, c8)
    assert np.array_equal(l8, l32)
    cases.gate(c8, want, near, "fp32 frame")
    mid = cases.thresholds(c8)[-1]
    a.set_confidence(mid, 200)                                         # per handle: b keeps min_conf = 0
    ul, uc = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    a.logits_conf(full, ul, uc)
    cases.gate(uc, want, near, "tdnet_logits_conf")
    assert np.array_equal(ul, cases.rejected(l32, uc, mid, 200)) and (ul == 200).any() and (ul != 200).any()
    bl, bc = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    b.logits_conf(full, bl, bc)
    assert np.array_equal(bl, l32) and np.array_equal(bc, uc)
    b.logits_conf(full, None, bc)                                       # confidence only
    assert np.array_equal(bc, uc)
    a.close()
    b.close()


@pytest.mark.parametrize("precision", [1, 3])
def test_one_frame_at_other_precisions(lib, precision):
    """one frame each (the emulator is slow at precision 3): the labels against the first-maximum argmax of tdnet_forward_u8's logits"""
    e = _engine(lib, 2, opts={"precision": precision})
    e.set_input_u8(HS, WS)
    r = e.share()
    r.set_input_u8(HS, WS)
    src = _frames(1, 77)[0]
    full, lab, conf = np.zeros((19, H, W), np.float32), np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    r.forward_u8(src, 0, full)
    e.forward_u8_labels_conf(src, 0, lab, conf)
    assert np.array_equal(lab, full.argmax(0)) and e.last_launch_count() == r.last_launch_count() > 0
    want, near = cases.expected(full, ("precision", precision))
    cases.gate(conf, want, near, ("precision", precision))
    r.close()
    e.close()


def test_rejected_labels_compose_with_the_score_entry(clip):
    """labels_conf with a threshold and reject_label 255, then tdnet_labels_score: the confusion matrix over the pixels with conf >= min_conf."""
    owner, P, frames, labels, launches, refs = clip
    e = owner.share()
    e.set_input_u8(HS, WS)
    e.set_score()
    probe, c0 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    e.forward_u8_labels_conf(frames[0], 0, probe, c0)
    e.reset()
    min_conf = cases.thresholds(c0)[-1]
    e.set_confidence(min_conf, 255)
    total = np.zeros((19, 19), np.int64)
    for t, src in enumerate(frames[:P + 1]):
        l8, c8 = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        e.forward_u8_labels_conf(src, t % P, l8, c8)
        gt = score_cases.ground_truth("noise", 19, np.roll(labels[t], t))
        e.labels_score(l8, gt)
        keep = c8 >= min_conf
        assert 0 < keep.sum() < H * W and np.array_equal(l8, cases.rejected(labels[t], c8, min_conf, 255))
        total += score_cases.expected_matrix(np.where(keep, gt, 255), labels[t], 19)
        assert np.array_equal(e.score_read(), total), t
    assert 0 < total.sum()
    e.close()


def test_errors_name_their_entry_and_leave_a_pending_frame_alone(lib, clip):
    owner, P, frames, labels, launches, refs = clip
    e = owner.share()
    e.set_input_u8(HS, WS)
    x = np.zeros((1, 3, H, W), np.float32)
    full = np.zeros((19, H, W), np.float32)
    lab, conf = np.full((H, W), 0xEE, np.uint8), np.full((H, W), 0xEE, np.uint8)
    e.set_confidence(77, 19)
    for args in ((256, 0), (-1, 0), (0, 256), (0, -1)):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_confidence"):
            e.set_confidence(*args)
    e.set_confidence(0, 255)
    e.encode_u8(frames[0], 0)                                          # a pending frame: every failure below must leave it pending
    for name, call in (("tdnet_forward_labels_conf", lambda: e.forward_labels_conf(x, 1, lab, None)),
                       ("tdnet_forward_u8_labels_conf", lambda: e.forward_u8_labels_conf(frames[1], 1, lab, None)),
                       ("tdnet_propagate_labels_conf", lambda: e.propagate_labels_conf(lab, None)),
                       ("tdnet_logits_conf", lambda: e.logits_conf(full, lab, None)),
                       ("tdnet_logits_conf", lambda: e.logits_conf(None, lab, conf))):
        with pytest.raises(_capi.TdnetError, match=name + ": null"):
            call()
    with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_labels_conf.*waiting for tdnet_propagate"):   # the forward forms respect the pending frame
        e.forward_u8_labels_conf(frames[1], 1, lab, conf)
    with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_labels_conf"):
        e.forward_u8_labels_conf(frames[1], P, lab, conf)              # pos_id out of range
    assert e.fifo_len() == 0 and (lab == 0xEE).all() and (conf == 0xEE).all()
    e.propagate_labels_conf(lab, conf)                                 # ... which is still there, and is the frame it was
    assert e.fifo_len() == 1 and np.array_equal(lab, labels[0])
    cases.gate(conf, refs[0][0], refs[0][1], "pending frame")
    with pytest.raises(_capi.TdnetError, match="tdnet_propagate.*no encoded frame"):
        e.propagate_labels_conf(lab, conf)
    assert e.fifo_len() == 1
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    for name, call in (("tdnet_forward_labels_conf", lambda: fresh.forward_labels_conf(x, 0, lab, conf)),
                       ("tdnet_propagate_labels_conf", lambda: fresh.propagate_labels_conf(lab, conf)),
                       ("tdnet_logits_conf", lambda: fresh.logits_conf(full, lab, conf))):
        with pytest.raises(_capi.TdnetError, match=name + ".*not finalized"):
            call()
    fresh.set_confidence(3, 4)                                         # plain host state: no device, no weights needed
    fresh.close()
    e.close()


def test_model_classes_check_their_arguments():
    import torch
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    assert m.set_confidence() == (0, 255) and m.set_confidence(0.5) == (128, 255) and m.set_confidence(1.0, 19) == (255, 19)
    assert m.set_confidence(1e-9)[0] == 1 and m.set_confidence(7.0)[0] == 255 and m.set_confidence(-1.0)[0] == 0   # ceil, then clamped
    with pytest.raises(RuntimeError, match="reject_label"):
        m.set_confidence(0.5, 256)
    with pytest.raises(RuntimeError, match="uint8 image"):
        m.forward_labels_conf_u8(torch.zeros(1, 41, 83, 3), 0, (33, 65))
    with pytest.raises(_capi.TdnetError):                               # no CPU fallback
        m.forward_labels_conf(torch.zeros(1, 3, 33, 65), 0)
    with pytest.raises(_capi.TdnetError):
        m.forward_labels_conf_u8(torch.zeros(1, 41, 83, 3, dtype=torch.uint8), 0, (33, 65))
    with pytest.raises(RuntimeError, match="no encoded frame"):
        m.propagate(conf=True)
    with pytest.raises(RuntimeError, match="no handle"):
        m.logits_conf(torch.zeros(1, 19, 33, 65))
    assert m.engine is None
