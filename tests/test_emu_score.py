"""Score out (include/tdnet.h "score out"), on the CPU through the kernel emulator: the fused upsample + argmax + count kernel and the labels + count
kernel against np.bincount of the labels tdnet_op_upsample_argmax gives, on both sides of the LDS / global-atomics threshold; whole frames scored
on the device against the same frames asked for as labels and counted on the host; the error paths.  Every comparison is exact."""
import numpy as np
import pytest

import emu_util
import opcheck
import score_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


_labels = {}


def labels_of(lib, name, C, h, w, H, W):
    """The labels of a case through tdnet_op_upsample_argmax (an entry that predates the score entries), computed once."""
    if name not in _labels:
        x = cases.lowres_logits(name, C, h, w)
        l32 = np.full((H, W), -1, np.int32)
        lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, None, None))
        assert l32.min() >= 0 and l32.max() < C
        l32.setflags(write=False)
        _labels[name] = l32
    return _labels[name]


def held(a, off, fill):
    """(holder, view): the bytes of `a` (or room for a.size bytes if fill only) `off` bytes into a holder of 0xEE with 16 guard bytes."""
    holder = np.full(a.size + 16, 0xEE, np.uint8)
    if not fill:
        holder[off:off + a.size] = a.reshape(-1)
    return holder, holder[off:off + a.size].reshape(a.shape)


@opcheck.guarded_arg("x", False, accumulates="cm")
def score(lib, C, H, W, gt, x=None, h=0, w=0, gt_off=0, lab_off=None, gt_map=None, labels_in=None, cm=None):
    """One call of the operator entry: (cm, labels written or None).  gt sits gt_off bytes into a 0xEE holder, the label map (lab_off != None) lab_off
    bytes into another whose guard bytes must survive; cm is accumulated into (a fresh zero matrix by default)."""
    gh, gv = held(gt, gt_off, False)
    cm = np.zeros((C, C), np.uint64) if cm is None else cm
    lh = lv = None
    if lab_off is not None:
        lh, lv = held(np.zeros((H, W), np.uint8), lab_off, True)
    m = None if gt_map is None else np.ascontiguousarray(gt_map, np.uint8)
    lib.check(lib.tdnet_op_upsample_argmax_score(None if x is None else x.ctypes.data, C, h, w, H, W, gv.ctypes.data, None if m is None else m.ctypes.data,
                                                 None if lv is None else lv.ctypes.data, cm.ctypes.data, None if labels_in is None else labels_in.ctypes.data, None))
    assert np.array_equal(gv, gt)                                      # the ground truth is only read
    if lh is not None:
        assert (lh[:lab_off] == 0xEE).all() and (lh[lab_off + H * W:] == 0xEE).all(), lab_off
    return cm, lv


@pytest.mark.parametrize("kind", cases.GT_KINDS)
@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_both_kernels_count_what_bincount_counts(lib, name, C, lo, hi, kind):
    (h, w), (H, W) = lo, hi
    x = cases.lowres_logits(name, C, h, w)
    labels = labels_of(lib, name, C, h, w, H, W)
    gt = cases.ground_truth(kind, C, labels)
    want = cases.expected_matrix(gt, labels, C)
    assert want.sum() == (gt < C).sum()
    if kind == "labels":
        assert want.sum() == H * W and (want == np.diag(np.diag(want))).all()
    if kind == "all_ignored" and C < 256:
        assert not want.any()
    for gt_off, lab_off in cases.OFFSETS:
        cm, written = score(lib, C, H, W, gt, x, h, w, gt_off, lab_off)
        assert np.array_equal(cm, want), (name, kind, gt_off, lab_off)
        assert cm.sum() == (gt < C).sum()
        assert np.array_equal(written, labels), (name, kind, lab_off)   # the label map tdnet_op_upsample_argmax gives
    cm, _ = score(lib, C, H, W, gt, x, h, w, 1, None)                   # no label map asked for: the same matrix
    assert np.array_equal(cm, want), (name, kind)
    l8 = labels.astype(np.uint8)
    for gt_off, lab_off in cases.OFFSETS[:2] if kind != "noise" else cases.OFFSETS:   # k_labels_score: the label map the caller holds, at any address
        lh, lv = held(l8, lab_off, False)
        cm, _ = score(lib, C, H, W, gt, gt_off=gt_off, labels_in=lv)
        assert np.array_equal(cm, want), (name, kind, gt_off, lab_off)
        assert np.array_equal(lv, l8)


def test_ties_the_lower_index_still_wins(lib):
    name, C, (h, w), (H, W) = [c for c in cases.ARGMAX_CASES if c[0] == "ties"][0]
    x = cases.lowres_logits(name, C, h, w)
    cm, written = score(lib, C, H, W, np.zeros((H, W), np.uint8), x, h, w, 0, 0)
    assert (written[::8, ::16][[0, 1, 3, 4]] == 4).all() and (written[::8, ::16][2] == 3).all()
    assert cm[0, 4] > 0 and cm[0, 3] > 0 and cm[1:].sum() == 0 and cm.sum() == H * W
    assert np.array_equal(cm[0], np.bincount(written.reshape(-1), minlength=C))


@pytest.mark.parametrize("name", ["c256", "c64_lds", "c65_global", "odd_w"])
def test_a_map_that_folds_and_permutes(lib, name):
    """Raw ids through a non-identity map: a permutation of the class ids, every fourth id and every byte >= C folded to 255.  At C = 256 no
    byte can say "ignore" (255 < nclass): there the map permutes only."""
    _, C, (h, w), (H, W) = [c for c in cases.ARGMAX_CASES if c[0] == name][0]
    x = cases.lowres_logits(name, C, h, w)
    labels = labels_of(lib, name, C, h, w, H, W)
    gt = np.random.default_rng(77).integers(0, 256, (H, W)).astype(np.uint8)   # raw bytes, all 256 values
    m = cases.permuting_map(C)
    want = cases.expected_matrix(gt, labels, C, m)
    assert 0 < want.sum() and (C == 256 or want.sum() < H * W) and not np.array_equal(want, cases.expected_matrix(gt, labels, C))
    cm, _ = score(lib, C, H, W, gt, x, h, w, 3, 2, gt_map=m)
    assert np.array_equal(cm, want)
    cm, _ = score(lib, C, H, W, gt, gt_off=2, gt_map=m, labels_in=labels.astype(np.uint8))
    assert np.array_equal(cm, want)


def test_one_class(lib):
    _, C, (h, w), (H, W) = [c for c in cases.ARGMAX_CASES if c[0] == "c1"][0]
    gt = cases.ground_truth("noise", 2, np.zeros((H, W), np.int32))     # ids 0, 1 and 255: only 0 is a class
    cm, written = score(lib, 1, H, W, gt, cases.lowres_logits("c1", 1, h, w), h, w, 2, 1)
    assert cm.shape == (1, 1) and cm[0, 0] == (gt == 0).sum() > 0 and not written.any()


@pytest.mark.parametrize("name", ["odd_w", "c65_global"])
def test_calls_accumulate_into_a_matrix_that_really_is_64_bit(lib, name):
    _, C, (h, w), (H, W) = [c for c in cases.ARGMAX_CASES if c[0] == name][0]
    x = cases.lowres_logits(name, C, h, w)
    labels = labels_of(lib, name, C, h, w, H, W)
    gt = cases.ground_truth("blocky", C, labels)
    want = cases.expected_matrix(gt, labels, C).astype(np.uint64)
    cm = np.zeros((C, C), np.uint64)
    g, l = np.unravel_index(np.argmax(want), want.shape)
    cm[g, l] = 2 ** 32 - 3                                             # a bin about to pass 32 bits
    score(lib, C, H, W, gt, x, h, w, 0, 0, cm=cm)
    score(lib, C, H, W, gt, gt_off=1, labels_in=labels.astype(np.uint8), cm=cm)
    want2 = 2 * want
    want2[g, l] += np.uint64(2 ** 32 - 3)
    assert want[g, l] > 3 and np.array_equal(cm, want2) and int(cm[g, l]) == 2 ** 32 - 3 + 2 * int(want[g, l]) > 2 ** 32


@pytest.mark.parametrize("name", ["odd_w", "c65_global"])
@pytest.mark.parametrize("uniform", ["1", "0"])
def test_with_and_without_the_wave_uniform_path_the_counts_are_the_same(lib, name, uniform, monkeypatch):
    """TDNET_SCORE_WAVE_UNIFORM=1 / 0 (read by the operator entry only; tools/score_probe.py measures with it) picks the kernels' instantiation."""
    _, C, (h, w), (H, W) = [c for c in cases.ARGMAX_CASES if c[0] == name][0]
    x = cases.lowres_logits(name, C, h, w)
    labels = labels_of(lib, name, C, h, w, H, W)
    monkeypatch.setenv("TDNET_SCORE_WAVE_UNIFORM", uniform)
    for kind in ("blocky", "one_id", "all_ignored", "labels", "noise"):
        gt = cases.ground_truth(kind, C, labels)
        want = cases.expected_matrix(gt, labels, C)
        assert np.array_equal(score(lib, C, H, W, gt, x, h, w, 1, 3)[0], want), kind
        assert np.array_equal(score(lib, C, H, W, gt, gt_off=3, labels_in=labels.astype(np.uint8))[0], want), kind


def test_labels_outside_the_matrix_are_not_counted(lib):
    """k_labels_score on a label map with values >= C (not this library's labels): such pixels have no column and are left out."""
    C, H, W = 19, 9, 21
    rng = np.random.default_rng(5)
    l8 = rng.integers(0, 40, (H, W)).astype(np.uint8)
    gt = rng.integers(0, 19, (H, W)).astype(np.uint8)
    keep = l8 < C
    want = np.bincount(C * gt[keep].astype(np.int64) + l8[keep], minlength=C * C).reshape(C, C)
    cm, _ = score(lib, C, H, W, gt, labels_in=l8)
    assert np.array_equal(cm, want) and cm.sum() == keep.sum() < H * W


def test_operator_entry_checks_its_arguments(lib):
    cm, gt = np.zeros((19, 19), np.uint64), np.zeros((33, 65), np.uint8)
    x = cases.lowres_logits("odd_w", 19, 5, 9)
    for args in ((x.ctypes.data, 19, 5, 9, 33, 65, None, None, None, cm.ctypes.data, None, None),
                 (x.ctypes.data, 19, 5, 9, 33, 65, gt.ctypes.data, None, None, None, None, None),
                 (x.ctypes.data, 257, 5, 9, 33, 65, gt.ctypes.data, None, None, cm.ctypes.data, None, None),
                 (None, 19, 5, 9, 33, 65, gt.ctypes.data, None, None, cm.ctypes.data, None, None)):
        with pytest.raises(_capi.TdnetError, match="tdnet_op_upsample_argmax_score"):
            lib.check(lib.tdnet_op_upsample_argmax_score(*args))
    assert not cm.any()


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
H, W, HS, WS, T, P = 33, 65, 41, 83, 6, 2


def _engine(lib, model=2):
    name = {4: "td4", 2: "td2", 1: "psp"}[model]
    spec = arch.model_spec(name, 19, "resnet18")
    e = Engine(model, 18, 19, H, W, 0, lib=lib, arch={})
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


@pytest.fixture(scope="module")
def clip(lib):
    """td2-resnet18 at 33x65 and six frames of random bytes at 41x83, with the labels forward_u8_labels gives for them on a handle of its own
    (computed once), that handle's launch counts, a ground truth per frame and the host's confusion matrix per frame."""
    owner = _engine(lib, 2)
    owner.set_input_u8(HS, WS)
    rng = np.random.default_rng(23)
    frames = [rng.integers(0, 256, (HS, WS, 3), dtype=np.uint8) for _ in range(T)]
    labels, launches, gts, cms = [], [], [], []
    for t, src in enumerate(frames):
        l8 = np.full((H, W), 0xEE, np.uint8)
        owner.forward_u8_labels(src, t % P, l8)
        labels.append(l8)
        launches.append(owner.last_launch_count())
        gts.append(cases.ground_truth(("noise", "blocky", "labels")[t % 3], 19, l8 if t % 3 == 2 else np.roll(l8, t)))
        cms.append(cases.expected_matrix(gts[-1], l8, 19))
    for a in frames + labels + gts + cms:
        a.setflags(write=False)
    yield owner, frames, labels, launches, gts, cms
    owner.close()


def test_frames_scored_on_the_device_equal_labels_counted_on_the_host(clip):
    """forward_u8_score throughout on a second handle: after every frame the matrix is the host's running sum, in as many launches as the label
    entry takes; the label map is written on even frames and not asked for on odd ones."""
    owner, frames, labels, launches, gts, cms = clip
    a = owner.share()
    a.set_input_u8(HS, WS)
    a.set_score()
    total = np.zeros((19, 19), np.int64)
    for t, src in enumerate(frames):
        l8 = np.full((H, W), 0xEE, np.uint8)
        a.forward_u8_score(src, t % P, gts[t], l8 if t % 2 == 0 else None)
        total += cms[t]
        assert np.array_equal(a.score_read(), total), t
        assert a.last_launch_count() == launches[t] > 0, t
        assert np.array_equal(l8, labels[t]) if t % 2 == 0 else (l8 == 0xEE).all()
        a.set_score()                                                  # idempotent: the counts stay
    assert a.fifo_len() == owner.fifo_len() and total.sum() > 0
    out = np.full((19, 19), 7, np.uint64)
    a.score_export(out)
    assert np.array_equal(out, total)
    a.score_reset()
    assert not a.score_read().any()
    a.close()


def test_fused_unfused_and_split_frames_mixed_on_one_handle(clip):
    """In turn forward_u8_score, forward_u8_labels + tdnet_labels_score of that map, and encode_u8 + propagate_score on ONE handle: the labels and
    the running matrix of the unmixed handles.  The FIFO does not care what left the frame."""
    owner, frames, labels, launches, gts, cms = clip
    c = owner.share()
    c.set_input_u8(HS, WS)
    c.set_score()
    total = np.zeros((19, 19), np.int64)
    for t, src in enumerate(frames):
        l8 = np.full((H, W), 0xEE, np.uint8)
        if t % 3 == 0:
            c.forward_u8_score(src, t % P, gts[t], l8)
            assert c.last_launch_count() == launches[t]
        elif t % 3 == 1:
            c.forward_u8_labels(src, t % P, l8)
            assert c.last_launch_count() == launches[t]
            c.labels_score(l8, gts[t])                                 # the unfused form: one more launch, outside the frame
        else:
            c.encode_u8(src, t % P)
            c.propagate_score(gts[t], l8)
        total += cms[t]
        assert np.array_equal(l8, labels[t]), t
        assert np.array_equal(c.score_read(), total), t
    assert c.fifo_len() == owner.fifo_len()
    c.close()


def test_fp32_frames_pspnet_and_a_map(lib):
    e = _engine(lib, 1)
    m = cases.permuting_map(19)
    e.set_score(m)
    x = weights.synth_video(H, W, 1, seed=3)[0]
    l32 = np.full((H, W), -1, np.int32)
    e.forward_labels(x, 0, l32)
    n_labels = e.last_launch_count()
    gt = np.random.default_rng(9).integers(0, 256, (H, W)).astype(np.uint8)
    l8 = np.full((H, W), 0xEE, np.uint8)
    e.forward_score(x, 0, gt, l8)
    assert e.last_launch_count() == n_labels > 0 and np.array_equal(l8, l32)
    want = cases.expected_matrix(gt, l32, 19, m)
    assert np.array_equal(e.score_read(), want) and 0 < want.sum() < H * W
    e.set_score(m)                                                     # an equal map: nothing happens
    assert np.array_equal(e.score_read(), want)
    e.set_score(None)                                                  # another map: a new, zeroed matrix
    assert not e.score_read().any()
    e.close()


def test_errors_leave_the_fifo_and_a_pending_frame_alone(lib, clip):
    owner, frames, labels, launches, gts, cms = clip
    e = owner.share()
    x = np.zeros((1, 3, H, W), np.float32)
    lab, out = np.zeros((H, W), np.uint8), np.zeros((19, 19), np.uint64)
    e.set_input_u8(HS, WS)
    e.encode_u8(frames[0], 0)                                          # a pending frame: every failure below must leave it pending
    _, before, _ = e.memory_bytes()
    for call in (lambda: e.forward_score(x, 1, gts[0], lab), lambda: e.forward_u8_score(frames[1], 1, gts[0], lab), lambda: e.propagate_score(gts[0], lab),
                 lambda: e.labels_score(lab, gts[0]), lambda: e.score_reset(), lambda: e.score_export(out), lambda: e.score_read()):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_score"):  # a shared handle is unconfigured until it is configured itself
            call()
    assert not lab.any() and not out.any()
    e.set_score()
    assert e.memory_bytes()[1] == before + 19 * 19 * 8 + 256            # matrix and map are counted in tdnet_memory_bytes
    assert not e.score_read().any()                                    # ... and it has its own zero matrix
    with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):   # the forward forms respect the pending frame like their siblings
        e.forward_u8_score(frames[1], 1, gts[0], lab)
    assert e.fifo_len() == 0 and not e.score_read().any()
    e.propagate_score(gts[0], lab)                                     # ... which is still there, and is the frame it was
    assert e.fifo_len() == 1 and np.array_equal(lab, labels[0]) and np.array_equal(e.score_read(), cms[0])
    with pytest.raises(_capi.TdnetError, match="no encoded frame"):
        e.propagate_score(gts[0], lab)
    assert e.fifo_len() == 1 and np.array_equal(e.score_read(), cms[0])
    small = np.zeros(19 * 19 - 1, np.uint64)
    assert lib.tdnet_score_read(e.h, small.ctypes.data, small.size, None) < 0 and b"capacity" in lib.tdnet_last_error() and not small.any()
    assert lib.tdnet_forward_u8_score(e.h, frames[1].ctypes.data, 1, None, lab.ctypes.data, None) < 0 and b"null" in lib.tdnet_last_error()
    with pytest.raises(_capi.TdnetError, match="256 values"):
        e.set_score(np.zeros(255, np.uint8))
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_score()
    fresh.close()
    e.close()


def test_model_classes_check_their_arguments():
    import torch
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    gt = torch.zeros(1, 33, 65, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="uint8 image"):
        m.forward_score_u8(torch.zeros(1, 41, 83, 3), gt, 0, (33, 65))
    with pytest.raises(RuntimeError, match="gt"):
        m.forward_score_u8(torch.zeros(1, 41, 83, 3, dtype=torch.uint8), gt.float(), 0, (33, 65))
    with pytest.raises(RuntimeError, match="gt"):
        m.forward_score(torch.zeros(1, 3, 33, 65), gt[0], 0)
    with pytest.raises(_capi.TdnetError):                               # no CPU fallback
        m.forward_score(torch.zeros(1, 3, 33, 65), gt, 0)
    with pytest.raises(_capi.TdnetError):
        m.forward_score_u8(torch.zeros(1, 41, 83, 3, dtype=torch.uint8), gt, 0, (33, 65))
    with pytest.raises(RuntimeError, match="no encoded frame"):
        m.propagate(labels="score", gt=gt)
    with pytest.raises(RuntimeError, match="no handle"):
        m.confusion_matrix()
    assert m.engine is None
