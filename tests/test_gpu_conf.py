"""Confidence out on the MI355X: the operator tests of tests/test_emu_conf.py on device memory (plus rows wider than one workgroup's strip and the
real 769x1537 geometry), whole frames against the label entries and the float64 softmax of tdnet_forward's logits in fp32, fp16 mode and
precision 2, a batch of three through the model class, a captured pos_id cycle, and the command line with --conf / --min_conf.  Labels and
rejection are compared exactly; the confidence bytes through the gate of tests/conf_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opcheck
import conf_cases as cases
import score_cases
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


_ref = {}


def reference(lib, key, x, C, h, w, H, W):
    """(x on the device, full logits on the device, labels, want, near) through entries that predate the confidence entries; computed once."""
    if key not in _ref:
        xd = torch.from_numpy(np.array(x)).cuda()                      # a writable copy: the cases are read-only
        full = torch.full((C, H, W), float("nan"), dtype=torch.float32, device="cuda")
        lib.check(lib.tdnet_op_upsample(xd.data_ptr(), C, h, w, H, W, full.data_ptr(), _stream()))
        l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        lib.check(lib.tdnet_op_upsample_argmax(xd.data_ptr(), C, h, w, H, W, l32.data_ptr(), None, _stream()))
        labels = l32.cpu().numpy()
        assert labels.min() >= 0 and labels.max() < C
        want, near = cases.expected(full.cpu().numpy(), key)
        _ref[key] = (xd, full, labels, want, near)
    return _ref[key]


@opcheck.guarded_arg("x", True)
@opcheck.guarded_arg("full", True)
def conf_op(lib, C, H, W, x=None, h=0, w=0, full=None, lab_off=0, conf_off=0, min_conf=0, reject=255, want_labels=True):
    """One call of the operator entry on device memory: (labels written or None, confidence written) as numpy.  Either map sits at its byte
    offset inside a 0xEE holder whose 16 guard bytes must survive."""
    n = H * W
    ch = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    lh = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda") if want_labels else None
    lib.check(lib.tdnet_op_upsample_argmax_conf(None if x is None else x.data_ptr(), C, h, w, H, W, None if lh is None else lh.data_ptr() + lab_off,
                                                ch.data_ptr() + conf_off, min_conf, reject, None if full is None else full.data_ptr(), _stream()))
    chost = ch.cpu().numpy()
    assert (chost[:conf_off] == 0xEE).all() and (chost[conf_off + n:] == 0xEE).all(), (lab_off, conf_off)
    lab = None
    if lh is not None:
        lhost = lh.cpu().numpy()
        assert (lhost[:lab_off] == 0xEE).all() and (lhost[lab_off + n:] == 0xEE).all(), (lab_off, conf_off)
        lab = lhost[lab_off:lab_off + n].reshape(H, W)
    return lab, chost[conf_off:conf_off + n].reshape(H, W)


def check_case(lib, key, x, C, h, w, H, W, offsets, thresholds=True):
    xd, full, labels, want, near = reference(lib, key, x, C, h, w, H, W)
    first = None
    for lab_off, conf_off in offsets:                                  # the fused kernel
        lab, conf = conf_op(lib, C, H, W, xd, h, w, lab_off=lab_off, conf_off=conf_off)
        assert np.array_equal(lab, labels), (key, lab_off, conf_off)
        cases.gate(conf, want, near, (key, lab_off, conf_off))
        first = conf if first is None else first
        assert np.array_equal(conf, first), (key, lab_off, conf_off)
    _, only = conf_op(lib, C, H, W, xd, h, w, conf_off=3, want_labels=False)
    assert np.array_equal(only, first), key
    ufirst = None
    for lab_off, conf_off in cases.FEW_OFFSETS:                        # the unfused kernel on tdnet_op_upsample's output
        lab, conf = conf_op(lib, C, H, W, full=full, lab_off=lab_off, conf_off=conf_off)
        assert np.array_equal(lab, labels), (key, lab_off, conf_off)
        cases.gate(conf, want, near, (key, "unfused", lab_off, conf_off))
        d = np.abs(conf.astype(np.int64) - first)
        assert d.max() <= 1 and not (d != 0)[~near].any(), key
        ufirst = conf if ufirst is None else ufirst
        assert np.array_equal(conf, ufirst)
    _, only = conf_op(lib, C, H, W, full=full, conf_off=1, want_labels=False)
    assert np.array_equal(only, ufirst), key
    if not thresholds:
        return
    some = 0
    for i, min_conf in enumerate(cases.thresholds(first)):             # rejection: exact on the bytes the kernel itself wrote
        for reject in cases.REJECT_LABELS:
            lab, conf = conf_op(lib, C, H, W, xd, h, w, lab_off=(i + 1) & 3, conf_off=i & 3, min_conf=min_conf, reject=reject)
            assert np.array_equal(conf, first), (key, min_conf, reject)
            assert np.array_equal(lab, cases.rejected(labels, conf, min_conf, reject)), (key, min_conf, reject)
            some += int((conf < min_conf).sum())
            lab, conf = conf_op(lib, C, H, W, full=full, lab_off=i & 3, conf_off=(i + 2) & 3, min_conf=min_conf, reject=reject)
            assert np.array_equal(conf, ufirst) and np.array_equal(lab, cases.rejected(labels, conf, min_conf, reject)), (key, min_conf, reject)
    assert some > 0 or C == 1


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_both_kernels_labels_confidence_and_rejection(lib, case):
    name, C, (h, w), (H, W), scale = case
    check_case(lib, cases.case_id(case), cases.logits(name, C, h, w, scale), C, h, w, H, W, cases.offsets_of(name))
    if C == 1:
        assert (conf_op(lib, C, H, W, _ref[cases.case_id(case)][0], h, w)[1] == 255).all()


@pytest.mark.parametrize("scale", cases.SCALES)
@pytest.mark.parametrize("name,C,lo,hi", cases.WIDE_CASES, ids=[c[0] for c in cases.WIDE_CASES])
def test_wide_rows_and_the_real_geometry(lib, name, C, lo, hi, scale):
    (h, w), (H, W) = lo, hi
    x = (np.random.default_rng(H + W).standard_normal((C, h, w)) * scale).astype(np.float32)
    check_case(lib, "%s-x%d" % (name, scale), x, C, h, w, H, W, cases.FEW_OFFSETS, thresholds=scale == 1)
    _ref.pop("%s-x%d" % (name, scale))                                 # 90 MB of logits at 769x1537: not kept


@pytest.mark.parametrize("passes", ["1", "2"])
def test_one_pass_and_two_pass_forms_pass_the_same_gates(lib, passes, monkeypatch):
    """TDNET_CONF_PASSES (read by the operator entry only): both instantiations of both kernels ship"""
    monkeypatch.setenv("TDNET_CONF_PASSES", passes)
    for case in [c for c in cases.CASES if c[0] in ("odd_w", "c256", "ties")]:
        name, C, (h, w), (H, W), scale = case
        check_case(lib, cases.case_id(case), cases.logits(name, C, h, w, scale), C, h, w, H, W, cases.FEW_OFFSETS, thresholds=False)


def test_non_finite_logits_leave_the_labels_alone(lib):
    name, C, (h, w), (H, W), scale = cases.CASES[0]
    x = cases.logits(name, C, h, w, scale).copy()
    x[3, 1, 2], x[7, 2, 5], x[0, 4, 8], x[5, 0, 0] = np.nan, np.inf, -np.inf, np.nan
    xd = torch.from_numpy(x).cuda()
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    lib.check(lib.tdnet_op_upsample_argmax(xd.data_ptr(), C, h, w, H, W, l32.data_ptr(), None, _stream()))
    full = torch.zeros((C, H, W), dtype=torch.float32, device="cuda")
    lib.check(lib.tdnet_op_upsample(xd.data_ptr(), C, h, w, H, W, full.data_ptr(), _stream()))
    assert not torch.isfinite(full).all()
    assert np.array_equal(conf_op(lib, C, H, W, xd, h, w, lab_off=1, conf_off=3)[0], l32.cpu().numpy())
    assert np.array_equal(conf_op(lib, C, H, W, full=full, lab_off=2, conf_off=1)[0], l32.cpu().numpy())


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
def make_model(name, kernel_opts=None):
    from tdnet_amd.model import td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0, kernel_opts=kernel_opts)
    else:
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0, kernel_opts=kernel_opts)
    return m.eval().to("cuda")


def _clip(n, Hs, Ws, seed, batch=1):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.integers(0, 256, (batch, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(n)]


@pytest.mark.parametrize("name,opts", [("td4", None), ("td2", None), ("td4", {"precision": 1}), ("td4", {"precision": 2})],
                         ids=["td4-psp18-fp32", "td2-psp18-fp32", "td4-psp18-fp16-mode", "td4-psp18-precision2"])
def test_frames_with_confidence_equal_the_label_entries_frames(name, opts):
    """A clip of 2 P + 1 frames at 129x257.  Model B: forward_labels_u8; L: forward_u8 (the logits of the float64 reference); A: forward_labels_conf_u8
    throughout; C mixes in turn the conf entry, the label entry, encode_u8 + propagate(conf=True) and the unfused logits_conf of L's logits."""
    H, W, Hs, Ws = 129, 257, 160, 321
    b = make_model(name, opts)
    b.ensure_engine(H, W, "cuda")
    lg, a, c = (make_model(name, opts).share_weights_with(b) for _ in range(3))
    P = b.path_num
    with torch.no_grad():
        for t, u in enumerate(_clip(2 * P + 1, Hs, Ws, 51)):
            l8 = b.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            full = lg.forward_u8(u, pos_id=t % P, in_size=(H, W))
            want, near = cases.expected(full[0].cpu().numpy(), (name, opts, t))
            la, ca = a.forward_labels_conf_u8(u, t % P, (H, W))
            assert torch.equal(la, l8), t
            cases.gate(ca[0].cpu().numpy(), want, near, ("frame", t))
            assert a.engine.last_launch_count() == b.engine.last_launch_count() > 0, t
            if t % 4 == 0:
                lc, cc = c.forward_labels_conf_u8(u, t % P, (H, W))
                assert c.engine.last_launch_count() == b.engine.last_launch_count()
            elif t % 4 == 1:
                lc, cc = c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W)), ca
            elif t % 4 == 2:
                c.encode_u8(u, t % P, in_size=(H, W))
                lc, cc = c.propagate(conf=True)
            else:
                c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
                lc, cc = c.logits_conf(full)                           # the unfused form: within 1 at near-boundary pixels only
                d = (cc.int() - ca.int()).abs()[0].cpu().numpy()
                assert d.max() <= 1 and not (d != 0)[~near].any(), t
                cases.gate(cc[0].cpu().numpy(), want, near, ("unfused frame", t))
                cc = ca
            assert torch.equal(lc, l8) and torch.equal(cc, ca), t      # bit-identical: the FIFO does not care what left the frame
    assert a.engine.fifo_len() == b.engine.fifo_len() == c.engine.fifo_len()


def test_a_batch_of_three_a_threshold_and_the_score_of_the_accepted_pixels():
    H, W, Hs, Ws = 65, 129, 80, 161
    b = make_model("td2")
    b.ensure_engine(H, W, "cuda")
    a = make_model("td2").share_weights_with(b)
    probe = make_model("td2").share_weights_with(b)
    clip = _clip(3, Hs, Ws, 52, batch=3)
    with torch.no_grad():
        _, c0 = probe.forward_labels_conf_u8(clip[0], 0, (H, W))
        mid = cases.thresholds(c0.cpu().numpy())[-1]
        assert a.set_confidence(mid / 255.0, 255) == (mid, 255)        # before the batch's handles exist: applies to those created later
        for t, u in enumerate(clip):
            l8 = b.forward_labels_u8(u, pos_id=t % 2, in_size=(H, W)).cpu().numpy()
            la, ca = a.forward_labels_conf_u8(u, t % 2, (H, W))
            la, ca = la.cpu().numpy(), ca.cpu().numpy()
            assert la.shape == ca.shape == (3, H, W)
            assert np.array_equal(la, cases.rejected(l8, ca, mid, 255)), t
            if t == 0:
                assert np.array_equal(ca, c0.cpu().numpy())
                assert (la == 255).any() and (la != 255).any()
        assert len([a.engine] + list(a._extra_engines)) == 3
        # composition: the rejected label 255 >= nclass is not counted by the score entry
        gt_np = np.stack([score_cases.ground_truth("noise", 19, np.roll(l8[i], 2)) for i in range(3)])
        a.score_labels(torch.from_numpy(la).cuda(), torch.from_numpy(gt_np).cuda())
        want = sum(score_cases.expected_matrix(np.where(ca[i] >= mid, gt_np[i], 255), l8[i], 19) for i in range(3))
        assert np.array_equal(a.confusion_matrix(), want) and 0 < want.sum() < (gt_np < 19).sum()
        # ... and comes out grey from the colour-map entry
        rgb = a.labels_rgb(torch.from_numpy(la[:1]).cuda(), (H, W)).cpu().numpy()[0]
        assert (rgb[la[0] == 255] == 255).all()


def test_pspnet_and_fp32_frames():
    from tdnet_amd import weights
    from tdnet_amd.model import pspnet
    H, W = 33, 65
    m = pspnet.pspnet(nclass=19, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")
    x = torch.from_numpy(weights.synth_video(H, W, 1, seed=3)[0]).cuda()
    with torch.no_grad():
        l32 = m.forward_labels(x)
        n_labels = m.engine.last_launch_count()
        want, near = cases.expected(m(x)[0].cpu().numpy(), "pspnet")
        lab, conf = m.forward_labels_conf(x)
    assert m.engine.last_launch_count() == n_labels > 0
    assert np.array_equal(lab.cpu().numpy(), l32.cpu().numpy())
    cases.gate(conf[0].cpu().numpy(), want, near, "pspnet")


def test_errors_name_their_entry_and_leave_a_pending_frame_alone():
    H, W, Hs, Ws = 33, 65, 41, 83
    m, ref, old = make_model("td2"), make_model("td2"), make_model("td2")
    u = _clip(2, Hs, Ws, 53)
    with torch.no_grad():
        m.encode_u8(u[0], 0, in_size=(H, W))
        e = m.engine
        lab, conf = (torch.full((H, W), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
        for name, call in (("tdnet_forward_u8_labels_conf", lambda: e.forward_u8_labels_conf(u[1].data_ptr(), 1, lab.data_ptr(), None)),
                           ("tdnet_propagate_labels_conf", lambda: e.propagate_labels_conf(lab.data_ptr(), None)),
                           ("tdnet_logits_conf", lambda: e.logits_conf(None, lab.data_ptr(), conf.data_ptr()))):
            with pytest.raises(_capi.TdnetError, match=name + ": null"):
                call()
        for args in ((256, 0), (0, 256), (-1, 0)):
            with pytest.raises(_capi.TdnetError, match="tdnet_set_confidence"):
                e.set_confidence(*args)
        with pytest.raises(_capi.TdnetError, match="tdnet_forward_u8_labels_conf.*waiting for tdnet_propagate"):
            e.forward_u8_labels_conf(u[1].data_ptr(), 1, lab.data_ptr(), conf.data_ptr())
        torch.cuda.synchronize()
        assert (lab == 0xEE).all() and (conf == 0xEE).all()
        got, gconf = m.propagate(conf=True)                            # the pending frame is still there, and is the frame it was
        want, wconf = ref.forward_labels_conf_u8(u[0], 0, (H, W))
        assert torch.equal(got, want) and torch.equal(gconf, wconf)
        assert torch.equal(want, old.forward_labels_u8(u[0], pos_id=0, in_size=(H, W)))
        with pytest.raises(_capi.TdnetError, match="no encoded frame"):
            e.propagate_labels_conf(lab.data_ptr(), conf.data_ptr())


def test_a_captured_cycle_replays_bit_identically_with_the_threshold_of_capture_time():
    """One pos_id cycle of forward_labels_conf_u8 at 65x129 captured into a hipGraph (tdnet_warmup before the capture) and replayed twice: labels
    and confidence of the eager loop.  min_conf and reject_label are kernel arguments: the graph keeps the ones in force when it was captured."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    warm = 2 * P
    T = warm + cycles * P
    clip = _clip(T, Hs, Ws, 54)
    with torch.no_grad():
        m = make_model("td4")
        _, c0 = m.forward_labels_conf_u8(clip[0], 0, (H, W))
        mid = cases.thresholds(c0.cpu().numpy())[-1]
        m.reset()
        m.set_confidence(mid / 255.0, 77)
        eager = [tuple(o.clone() for o in m.forward_labels_conf_u8(clip[t], t % P, (H, W))) for t in range(T)]
        assert any((l == 77).any() for l, _ in eager) and any((l != 77).any() for l, _ in eager)
        m.reset()
        for t in range(warm):
            l, c = m.forward_labels_conf_u8(clip[t], t % P, (H, W))
            assert torch.equal(l, eager[t][0]) and torch.equal(c, eager[t][1])
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        m.engine.warmup(stream.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = [m.forward_labels_conf_u8(xin[j], j, (H, W)) for j in range(P)]
        m.set_confidence(0.0, 255)                                     # after the capture: the replays do not see it
        m.engine.set_confidence(0, 255)
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            graph.replay()
            torch.cuda.synchronize()
            for j in range(P):
                assert torch.equal(outs[j][0], eager[t0 + j][0]) and torch.equal(outs[j][1], eager[t0 + j][1]), (c, j)


def test_cli_writes_confidence_maps_and_greys_rejected_pixels(tmp_path):
    """Five random 80x161 frames, --in_size 65x129, with --u8 and without: `--conf DIR` saves the confidence map the model class gives for the same
    frames, and with `--min_conf T` the picture is decode_segmap of the nearest-sampled labels with the rejected pixels at 255 (grey)."""
    from PIL import Image
    from tdnet_amd.dataloader import cityscapesLoader, nearest_index
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(16)
    H, W, T = 65, 129, 5
    for t in range(T):
        Image.fromarray(rng.integers(0, 256, (80, 161, 3), dtype=np.uint8)).save(frames_dir / ("frame_%06d.png" % t))
    for u8 in (True, False):
        ld = cityscapesLoader(img_path=str(tmp_path / "data"), in_size=(H, W), as_uint8=u8)
        ld.load_frames()
        m = make_model("td4")
        host = []
        with torch.no_grad():
            m.ensure_engine(H, W, "cuda")
            probe = make_model("td4").share_weights_with(m)
            img0 = ld.data[0][0].cuda()
            c0 = (probe.forward_labels_conf_u8(img0, 0, (H, W)) if u8 else probe.forward_labels_conf(img0, 0))[1].cpu().numpy()
            thr = cases.thresholds(c0)[-1] / 255.0
            assert m.set_confidence(thr, 255)[0] == cases.thresholds(c0)[-1]
            for t, item in enumerate(ld.data):
                img = item[0].cuda()
                l, c = m.forward_labels_conf_u8(img, t % 4, (H, W)) if u8 else m.forward_labels_conf(img, t % 4)
                host.append((l[0].cpu().numpy(), c[0].cpu().numpy(), item[3]))
        out, cdir = tmp_path / ("out_%d" % u8), tmp_path / ("conf_%d" % u8)
        out.mkdir()
        r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0",
                            "--in_size", "65x129", "--conf", str(cdir), "--min_conf", repr(thr)] + (["--u8"] if u8 else []),
                           cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        rejected_some = False
        for t, (l, c, ori_size) in enumerate(host):
            name = "frame_%06d.png" % t
            assert np.array_equal(np.array(Image.open(cdir / "vid1" / name)), c), (u8, t)
            ys, xs = nearest_index(H, ori_size[1] // 4), nearest_index(W, ori_size[0] // 4)
            small = l.astype(np.int16)[ys][:, xs]
            pic = np.array(Image.open(out / "vid1" / name))
            assert np.array_equal(pic, ld.decode_segmap(small).astype(np.uint8)), (u8, t)
            assert (pic[small == 255] == 255).all()
            rejected_some |= bool((small == 255).any())
        assert rejected_some and len(os.listdir(out / "vid1")) == T
