"""Score out on the MI355X: the operator cases of tests/test_emu_score.py on device memory (plus rows wider than one workgroup's strip and the
real 769x1537 geometry), whole frames scored on the device against the same frames asked for as labels and counted on the host, a captured
pos_id cycle, and the command line with --gt_path.  Every comparison of counts is exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import opcheck
import score_cases as cases
from tdnet_amd import _capi
from tdnet_amd.metrics import SCORE_KEYS, runningScore

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


def labels_of(lib, x, C, h, w, H, W):
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    lib.check(lib.tdnet_op_upsample_argmax(x.data_ptr(), C, h, w, H, W, l32.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    l32 = l32.cpu().numpy()
    assert l32.min() >= 0 and l32.max() < C
    return l32


def held(a, off):
    """a device holder of 0xEE with the bytes of `a` (numpy uint8) `off` bytes in and 16 guard bytes: (holder, address of the bytes)"""
    holder = torch.full((a.size + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    holder[off:off + a.size] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    return holder, holder.data_ptr() + off


@opcheck.guarded_arg("x", True, accumulates="cm")
def score(lib, C, H, W, gt, x=None, h=0, w=0, gt_off=0, lab_off=None, gt_map=None, labels_in=None, lin_off=0, cm=None):
    """One call of the operator entry on device memory: (cm as numpy uint64, labels written or None)."""
    gh, gp = held(gt, gt_off)
    cm_d = torch.zeros((C, C), dtype=torch.int64, device="cuda") if cm is None else cm
    lh = lp = None
    if lab_off is not None:
        lh, lp = held(np.full((H, W), 0xEE, np.uint8), lab_off)
    lin = None if labels_in is None else held(labels_in, lin_off)
    m = None if gt_map is None else np.ascontiguousarray(gt_map, np.uint8)
    lib.check(lib.tdnet_op_upsample_argmax_score(None if x is None else x.data_ptr(), C, h, w, H, W, gp, None if m is None else m.ctypes.data, lp,
                                                 cm_d.data_ptr(), None if lin is None else lin[1], torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(gh.cpu().numpy()[gt_off:gt_off + H * W].reshape(H, W), gt)
    written = None
    if lh is not None:
        host = lh.cpu().numpy()
        assert (host[:lab_off] == 0xEE).all() and (host[lab_off + H * W:] == 0xEE).all(), lab_off
        written = host[lab_off:lab_off + H * W].reshape(H, W)
    return cm_d.cpu().numpy().view(np.uint64), written


def check_case(lib, name, C, h, w, H, W, x, kinds):
    labels = labels_of(lib, x, C, h, w, H, W)
    l8 = labels.astype(np.uint8)
    for kind in kinds:
        gt = cases.ground_truth(kind, C, labels)
        want = cases.expected_matrix(gt, labels, C)
        assert want.sum() == (gt < C).sum()
        for gt_off, lab_off in cases.OFFSETS:
            cm, written = score(lib, C, H, W, gt, x, h, w, gt_off, lab_off)
            assert np.array_equal(cm, want), (name, kind, gt_off, lab_off)
            assert np.array_equal(written, labels), (name, kind, lab_off)
            cm, _ = score(lib, C, H, W, gt, gt_off=gt_off, labels_in=l8, lin_off=lab_off)   # k_labels_score
            assert np.array_equal(cm, want), (name, kind, gt_off, lab_off)
        cm, _ = score(lib, C, H, W, gt, x, h, w, 1, None)              # no label map asked for: the same matrix
        assert np.array_equal(cm, want), (name, kind)
    return labels


@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_both_kernels_count_what_bincount_counts(lib, name, C, lo, hi):
    (h, w), (H, W) = lo, hi
    x = torch.from_numpy(cases.lowres_logits(name, C, h, w)).cuda()
    labels = check_case(lib, name, C, h, w, H, W, x, cases.GT_KINDS)
    if name == "ties":                                                 # the lower index still wins
        _, written = score(lib, C, H, W, np.zeros((H, W), np.uint8), x, h, w, 0, 0)
        assert (written[::8, ::16][[0, 1, 3, 4]] == 4).all() and (written[::8, ::16][2] == 3).all()
    if name in ("c256", "c64_lds", "c65_global", "odd_w"):             # raw ids through a map that permutes and (C < 256) folds to "ignore"
        gt = np.random.default_rng(77).integers(0, 256, (H, W)).astype(np.uint8)
        m = cases.permuting_map(C)
        want = cases.expected_matrix(gt, labels, C, m)
        assert 0 < want.sum() and (C == 256 or want.sum() < H * W)
        assert np.array_equal(score(lib, C, H, W, gt, x, h, w, 3, 2, gt_map=m)[0], want)
        assert np.array_equal(score(lib, C, H, W, gt, gt_off=2, gt_map=m, labels_in=labels.astype(np.uint8))[0], want)
    if name in ("odd_w", "c65_global"):                                # two calls accumulate, past 32 bits
        gt = cases.ground_truth("blocky", C, labels)
        want = cases.expected_matrix(gt, labels, C).astype(np.uint64)
        g, l = np.unravel_index(np.argmax(want), want.shape)
        cm = torch.zeros((C, C), dtype=torch.int64, device="cuda")
        cm[g, l] = 2 ** 32 - 3
        score(lib, C, H, W, gt, x, h, w, 0, 0, cm=cm)
        got, _ = score(lib, C, H, W, gt, gt_off=1, labels_in=labels.astype(np.uint8), cm=cm)
        want2 = 2 * want
        want2[g, l] += np.uint64(2 ** 32 - 3)
        assert np.array_equal(got, want2) and int(got[g, l]) > 2 ** 32


@pytest.mark.parametrize("uniform", ["1", "0"])
@pytest.mark.parametrize("name,C,lo,hi", cases.WIDE_CASES, ids=[c[0] for c in cases.WIDE_CASES])
def test_wide_rows_and_the_real_geometry(lib, name, C, lo, hi, uniform, monkeypatch):
    """with and without the kernels' wave-uniform path (TDNET_SCORE_WAVE_UNIFORM, read by the operator entry): both instantiations ship"""
    (h, w), (H, W) = lo, hi
    monkeypatch.setenv("TDNET_SCORE_WAVE_UNIFORM", uniform)
    x = torch.from_numpy(np.random.default_rng(H + W).standard_normal((C, h, w)).astype(np.float32)).cuda()
    check_case(lib, name, C, h, w, H, W, x, ("noise", "blocky", "labels"))


@pytest.mark.parametrize("uniform", ["1", "0"])
@pytest.mark.parametrize("name", ["odd_w", "c65_global"])
def test_with_and_without_the_wave_uniform_path_the_counts_are_the_same(lib, name, uniform, monkeypatch):
    _, C, (h, w), (H, W) = [c for c in cases.ARGMAX_CASES if c[0] == name][0]
    monkeypatch.setenv("TDNET_SCORE_WAVE_UNIFORM", uniform)
    x = torch.from_numpy(cases.lowres_logits(name, C, h, w)).cuda()
    check_case(lib, name, C, h, w, H, W, x, ("blocky", "one_id", "all_ignored", "labels", "noise"))


def make_model(name, bb="resnet18", kernel_opts=None):
    from tdnet_amd.model import pspnet, td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts)
    elif name == "td2":
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts)
    else:
        m = pspnet.pspnet(nclass=19, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts)
    return m.eval().to("cuda")


def frame_gt(rng, t, l8):
    """ground truth of frame t from its labels l8 (numpy [H, W]): noise, blocky or the (shifted) labels with holes, in turn"""
    if t % 3 == 2:
        gt = np.roll(l8, 3, axis=1).copy()
        gt[rng.random(l8.shape) < 0.1] = 255
        return gt
    return cases.ground_truth(("noise", "blocky")[t % 3], 19, l8 + t)


@pytest.mark.parametrize("name,H,W,Hs,Ws,opts", [("td4", 65, 129, 80, 161, None), ("td2", 33, 65, 41, 83, None), ("td4", 65, 129, 80, 161, {"precision": 1})],
                         ids=["td4-psp18-65x129", "td2-psp18-33x65", "td4-psp18-precision1"])
def test_frames_scored_on_the_device_equal_labels_counted_on_the_host(name, H, W, Hs, Ws, opts):
    """Six frames of random bytes.  Model B: forward_labels_u8 + host bincount; A: forward_score_u8 throughout (the label map asked for on even
    frames only); C in turn forward_score_u8, forward_labels_u8 + score_labels, and encode_u8 + propagate(labels="score").  Same running matrix,
    same labels, same launch counts."""
    b = make_model(name, kernel_opts=opts)
    b.ensure_engine(H, W, "cuda")
    a, c = (make_model(name, kernel_opts=opts).share_weights_with(b) for _ in range(2))
    P = b.path_num
    rng = np.random.default_rng(41)
    host = runningScore(19)
    with torch.no_grad():
        for t in range(6):
            u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
            l8 = b.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            gt_np = frame_gt(rng, t, l8[0].cpu().numpy())
            gt = torch.from_numpy(gt_np[None]).cuda()
            host.update([gt_np], [l8[0].cpu().numpy()])
            got = a.forward_score_u8(u, gt, t % P, (H, W), return_labels=t % 2 == 0)
            assert (got is None) if t % 2 else torch.equal(got, l8), t
            assert a.engine.last_launch_count() == b.engine.last_launch_count() > 0, t
            assert np.array_equal(a.confusion_matrix(), host.confusion_matrix), t
            if t % 3 == 0:
                lc = c.forward_score_u8(u, gt, t % P, (H, W), return_labels=True)
                assert c.engine.last_launch_count() == b.engine.last_launch_count()
            elif t % 3 == 1:
                lc = c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
                c.score_labels(lc, gt)
            else:
                c.encode_u8(u, t % P, in_size=(H, W))
                lc = c.propagate(labels="score", gt=gt)
            assert torch.equal(lc, l8), t
            assert np.array_equal(c.confusion_matrix(), host.confusion_matrix), t
    assert a.engine.fifo_len() == b.engine.fifo_len() == c.engine.fifo_len() and host.confusion_matrix.sum() > 0
    want, want_iou = host.get_scores()
    got, got_iou = a.get_scores()
    assert tuple(got) == SCORE_KEYS and all(got[k] == want[k] for k in SCORE_KEYS)
    assert all(got_iou[i] == want_iou[i] or (np.isnan(got_iou[i]) and np.isnan(want_iou[i])) for i in range(19))
    # score_export into a device buffer equals score_read; reset_score
    buf = torch.full((19, 19), -1, dtype=torch.int64, device="cuda")
    a.engine.score_export(buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(buf.cpu().numpy(), a.engine.score_read(torch.cuda.current_stream().cuda_stream).astype(np.int64))
    assert np.array_equal(buf.cpu().numpy(), host.confusion_matrix)
    from tdnet_amd import parallel
    assert np.array_equal(parallel.allreduce_score(a).cpu().numpy(), host.confusion_matrix)   # one rank: the sum over this model's handles
    a.reset_score()
    assert not a.confusion_matrix().any() and c.confusion_matrix().any()


def test_a_batch_of_two_sums_its_handles_and_a_map_folds():
    H, W, Hs, Ws = 33, 65, 41, 83
    b = make_model("td2")
    b.ensure_engine(H, W, "cuda")
    a = make_model("td2").share_weights_with(b)
    rng = np.random.default_rng(42)
    m = cases.permuting_map(19)
    host = runningScore(19)
    per_sample = [np.zeros((19, 19), np.int64) for _ in range(2)]
    with torch.no_grad():
        for t in range(3):
            u = torch.from_numpy(rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)).cuda()
            gt_np = rng.integers(0, 256, (2, H, W)).astype(np.uint8)   # raw ids, folded by the map
            l8 = b.forward_labels_u8(u, pos_id=t % 2, in_size=(H, W)).cpu().numpy()
            got = a.forward_score_u8(u, torch.from_numpy(gt_np).cuda(), t % 2, (H, W), gt_map=m, return_labels=True)
            assert np.array_equal(got.cpu().numpy(), l8), t
            for i in range(2):
                per_sample[i] += cases.expected_matrix(gt_np[i], l8[i], 19, m)
            host.add_counts(cases.expected_matrix(gt_np[0], l8[0], 19, m) + cases.expected_matrix(gt_np[1], l8[1], 19, m))
            assert np.array_equal(a.confusion_matrix(), host.confusion_matrix), t
    engines = [a.engine] + list(a._extra_engines)
    assert len(engines) == 2
    for i in range(2):                                                 # each handle owns the matrix of its own stream
        assert np.array_equal(engines[i].score_read().astype(np.int64), per_sample[i])
    assert 0 < host.confusion_matrix.sum() < 6 * H * W


def test_pspnet_and_fp32_frames_through_forward_score():
    from tdnet_amd import weights
    H, W = 33, 65
    m = make_model("psp")
    x = torch.from_numpy(weights.synth_video(H, W, 1, seed=3)[0]).cuda()
    with torch.no_grad():
        l32 = m.forward_labels(x)
        n_labels = m.engine.last_launch_count()
        gt_np = cases.ground_truth("noise", 19, l32[0].cpu().numpy())
        got = m.forward_score(x, torch.from_numpy(gt_np[None]).cuda(), return_labels=True)
    assert m.engine.last_launch_count() == n_labels > 0
    assert np.array_equal(got[0].cpu().numpy(), l32[0].cpu().numpy())
    assert np.array_equal(m.confusion_matrix(), cases.expected_matrix(gt_np, l32[0].cpu().numpy(), 19))


def test_errors_leave_a_pending_frame_alone():
    H, W, Hs, Ws = 33, 65, 41, 83
    m = make_model("td2")
    ref = make_model("td2")
    rng = np.random.default_rng(43)
    u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
    gt_np = rng.integers(0, 19, (1, H, W)).astype(np.uint8)
    gt = torch.from_numpy(gt_np).cuda()
    with torch.no_grad():
        m.encode_u8(u, 0, in_size=(H, W))
        e = m.engine
        lab = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        for call in (lambda: e.forward_u8_score(u.data_ptr(), 1, gt.data_ptr(), lab.data_ptr()), lambda: e.propagate_score(gt.data_ptr(), lab.data_ptr()),
                     lambda: e.labels_score(lab.data_ptr(), gt.data_ptr()), lambda: e.score_read()):
            with pytest.raises(_capi.TdnetError, match="tdnet_set_score"):
                call()
        _, before, _ = e.memory_bytes()
        e.set_score()
        assert e.memory_bytes()[1] == before + 19 * 19 * 8 + 256
        with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):
            e.forward_u8_score(u.data_ptr(), 1, gt.data_ptr(), lab.data_ptr())
        assert not e.score_read().any()
        got = m.propagate(labels="score", gt=gt)                       # the pending frame is still there, and is the frame it was
        want = ref.forward_labels_u8(u, pos_id=0, in_size=(H, W))
        assert torch.equal(got, want)
        assert np.array_equal(m.confusion_matrix(), cases.expected_matrix(gt_np[0], want[0].cpu().numpy(), 19))
        with pytest.raises(_capi.TdnetError, match="no encoded frame"):
            e.propagate_score(gt.data_ptr(), lab.data_ptr())
        small = np.zeros(19 * 19 - 1, np.uint64)
        assert e.lib.tdnet_score_read(e.h, small.ctypes.data, small.size, None) < 0 and b"capacity" in e.lib.tdnet_last_error()
        with pytest.raises(RuntimeError, match="ground truth"):        # the ground truth is at the network size
            m.forward_score_u8(u, gt[:, :, :W - 1], 1, (H, W))
        shared = e.share()                                             # a shared handle is unconfigured until it is configured itself ...
        shared.set_input_u8(Hs, Ws)
        with pytest.raises(_capi.TdnetError, match="tdnet_set_score"):
            shared.forward_u8_score(u.data_ptr(), 0, gt.data_ptr(), lab.data_ptr())
        shared.set_score()
        assert not shared.score_read().any() and e.score_read().any()  # ... and then has its own zero matrix
        shared.close()


def test_a_captured_cycle_of_scored_frames_replays_to_the_eager_matrix():
    """One pos_id cycle of forward_score_u8 at 65x129 captured into a hipGraph (tdnet_warmup and tdnet_set_score before the capture) and
    replayed twice: every replay adds its frames, and the matrix is the eager one."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    warm = 2 * P
    T = warm + cycles * P
    rng = np.random.default_rng(44)
    clip = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(T)]
    gts = [torch.from_numpy(cases.ground_truth(("noise", "blocky")[t % 2], 19, np.zeros((H, W), np.int32) + t)[None]).cuda() for t in range(T)]
    with torch.no_grad():
        m = make_model("td4")
        eager = [m.forward_score_u8(clip[t], gts[t], t % P, (H, W), return_labels=True).clone() for t in range(T)]
        after_warm = None
        m.reset()
        m.reset_score()
        for t in range(warm):                                          # steady state; the handle is configured (input and score) by these frames
            assert torch.equal(m.forward_score_u8(clip[t], gts[t], t % P, (H, W), return_labels=True), eager[t])
        after_warm = m.confusion_matrix()
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        gin = torch.zeros((P, 1, H, W), dtype=torch.uint8, device="cuda")
        m.engine.warmup(stream.cuda_stream)
        m.engine.set_score()
        torch.cuda.synchronize()
        before = m.confusion_matrix()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = [m.forward_score_u8(xin[j], gin[j], j, (H, W), return_labels=True) for j in range(P)]
        assert np.array_equal(m.confusion_matrix(), before) and np.array_equal(before, after_warm)   # capturing counts nothing
        want = after_warm.copy()
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
                gin[j].copy_(gts[t0 + j])
            graph.replay()
            torch.cuda.synchronize()
            for j in range(P):
                assert torch.equal(outs[j], eager[t0 + j]), (c, j)
                want += cases.expected_matrix(gts[t0 + j][0].cpu().numpy(), eager[t0 + j][0].cpu().numpy(), 19)
            assert np.array_equal(m.confusion_matrix(), want), c
    total = sum(cases.expected_matrix(gts[t][0].cpu().numpy(), eager[t][0].cpu().numpy(), 19) for t in range(T))
    assert np.array_equal(want, total) and total.sum() > 0


def _printed_scores(stdout):
    """the lines print_scores writes: {key: text of the value}, [text of the IoU of class i]"""
    score = {}
    for k in SCORE_KEYS:
        m = re.search(re.escape(k) + r" (\S+)", stdout)
        assert m, (k, stdout)
        score[k] = m.group(1)
    ious = re.findall(r"^(\d+) (\S+)$", stdout, flags=re.M)
    assert [int(i) for i, _ in ious] == list(range(19)), stdout
    return score, [v for _, v in ious]


def test_cli_prints_the_scores_of_a_host_running_score(tmp_path):
    """Five random 80x161 frames with random train-id ground truth at 80x161, --in_size 65x129: the scores `--gt_path` prints with --u8 --prefetch
    and with neither equal, to the printed digits, a host runningScore over the labels the library gives for the same frames (the plain run
    saves pictures of them; the labels themselves come from the model classes here) and the ground truth sampled with the nearest rule."""
    from PIL import Image
    from tdnet_amd.dataloader import cityscapesLoader, nearest_index
    frames_dir, gt_dir = tmp_path / "data" / "vid1", tmp_path / "gt" / "vid1"
    frames_dir.mkdir(parents=True)
    gt_dir.mkdir(parents=True)
    rng = np.random.default_rng(15)
    H, W = 65, 129
    gts = []
    for t in range(5):
        Image.fromarray(rng.integers(0, 256, (80, 161, 3), dtype=np.uint8)).save(frames_dir / ("frame_%06d.png" % t))
        g = rng.integers(0, 19, (80, 161)).astype(np.uint8)
        g[rng.random((80, 161)) < 0.1] = 255
        Image.fromarray(g).save(gt_dir / ("frame_%06d.png" % t))
        gts.append(g[nearest_index(80, H)][:, nearest_index(161, W)])
    host = {}
    for u8 in (True, False):                                            # the labels of the two loops (bytes in / the loader's fp32 tensor in)
        ld = cityscapesLoader(img_path=str(tmp_path / "data"), in_size=(H, W), as_uint8=u8)
        ld.load_frames()
        m = make_model("td4")
        rs = runningScore(19)
        with torch.no_grad():
            for t, item in enumerate(ld.data):
                img = item[0].cuda()
                l = m.forward_labels_u8(img, pos_id=t % 4, in_size=(H, W)) if u8 else m.forward_labels(img, pos_id=t % 4)
                rs.update([gts[t]], [l[0].cpu().numpy()])
        host[u8] = rs.get_scores()
    for extra, u8 in ((["--u8", "--prefetch"], True), ([], False)):
        out = tmp_path / ("out" + "".join(extra).replace("--", "_"))
        out.mkdir()
        r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0",
                            "--in_size", "65x129", "--gt_path", str(tmp_path / "gt")] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        score, ious = _printed_scores(r.stdout)
        want, want_iou = host[u8]
        assert score == {k: str(want[k]) for k in SCORE_KEYS}, (extra, score, want)
        assert ious == [str(want_iou[i]) for i in range(19)], extra
        assert len(os.listdir(out / "vid1")) == 5
