"""Runs out on the MI355X: the operator cases of tests/test_emu_runs.py on device memory between guard bands (513x513 is 257 blocks: the scan's chunk carry),
whole frames through the model classes against runs_of of the labels a second handle's label entry gives, a captured pos_id cycle, regions coded and
decoded, RunsDownloader's short-prefix path, every refusal and the command line with --runs.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opcheck
import out_cases
import runs_cases as cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import RUN_DTYPE, RUNS_OVERFLOW, RunsDownloader, run_table, runs_decode, runs_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES, DECODE_LAUNCHES = 4, 1                                       # include/tdnet.h TDNET_RUNS_LAUNCHES, TDNET_RUNS_DECODE_LAUNCHES
B = 1024                                                               # csrc/td_runs.h's block; test_the_block_is_the_one_the_cases_are_sized_for holds it to the library's


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


def test_the_block_is_the_one_the_cases_are_sized_for(lib):
    assert cases.block(lib) == B


@pytest.mark.parametrize("shape", cases.shapes(B), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.U8_PATTERNS)
def test_uint8_patterns_against_the_oracle(lib, name, shape):
    H, W = shape
    count = cases.check_map(lib, opcheck.GuardedTorchMem(), cases.pattern(name, H, W, B), what=(name,))
    if name == "constant":
        assert count == H
    if name in ("alternating", "stripes1"):
        assert count == H * W


@pytest.mark.parametrize("shape", cases.shapes(B), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.I32_PATTERNS)
def test_int32_patterns_against_the_oracle(lib, name, shape):
    H, W = shape
    count = cases.check_map(lib, opcheck.GuardedTorchMem(), cases.pattern(name, H, W, B, True), what=(name,))
    if name == "alternating":
        assert count == H * W


@pytest.mark.parametrize("field", out_cases.FIELDS)
@pytest.mark.parametrize("case", out_cases.CASES, ids=out_cases.case_id)
def test_from_logits_the_labels_are_the_label_kernels(lib, case, field):
    C, (h, w), (H, W) = case
    x = out_cases.logits(field, C, h, w)
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    dx = torch.from_numpy(x.copy()).cuda()
    lib.check(lib.tdnet_op_upsample_argmax(dx.data_ptr(), C, h, w, H, W, l32.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    cases.check_from_logits(lib, opcheck.GuardedTorchMem(), x, C, h, w, H, W, l32.cpu().numpy().astype(np.uint8))


@pytest.mark.parametrize("i32", [False, True], ids=["uint8", "int32"])
@pytest.mark.parametrize("shape", [(1, 1), (1, B + 1), (5, 7), (33, 65), (128, 256), (513, 513)], ids=lambda s: "%dx%d" % s)
def test_the_device_round_trip_is_the_map(lib, shape, i32):
    names = ("noise3",) if shape == (513, 513) else ("constant", "alternating", "noise3", "extremes" if i32 else "bytes_0_255", "stripes5")
    for name in names:
        cases.check_round_trip(lib, opcheck.GuardedTorchMem(), cases.pattern(name, shape[0], shape[1], B, i32))


def test_refusals_of_the_operator_entries_launch_nothing(lib):
    H, W = 33, 65
    mem = opcheck.GuardedTorchMem()
    map_t, map_p = cases.put_at(mem, cases.pattern("noise3", H, W, B), 0)
    tab_t = mem.empty((4 + 3, 2))
    for off in (1, 2, 4, 7):
        rc = lib.tdnet_op_runs(None, 0, 0, 0, H, W, None, map_p, None, 4, mem.ptr(tab_t) + off, mem.stream)
        assert rc != 0 and b"runs_dev = 0x" in lib.tdnet_last_error() and b"not 8-byte aligned" in lib.tdnet_last_error()
    for max_runs in (0, H * W + 1):
        assert lib.tdnet_op_runs(None, 0, 0, 0, H, W, None, map_p, None, max_runs, mem.ptr(tab_t), mem.stream) != 0 and b"max_runs" in lib.tdnet_last_error()
    assert lib.tdnet_op_runs(None, 0, 0, 0, H, W, None, None, map_p + 2, 4, mem.ptr(tab_t), mem.stream) != 0 and b"4-byte aligned" in lib.tdnet_last_error()
    assert lib.tdnet_op_runs(None, 0, 0, 0, H, W, None, map_p, None, 4, None, mem.stream) != 0 and b"runs_dev is NULL" in lib.tdnet_last_error()
    mem.verify(untouched=True)


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
def make_model(name, kernel_opts=None):
    from tdnet_amd.model import pspnet, td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0, kernel_opts=kernel_opts)
    elif name == "td2":
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0, kernel_opts=kernel_opts)
    else:
        m = pspnet.pspnet(nclass=19, model_path=None, backbone="resnet18", synthetic_seed=0, kernel_opts=kernel_opts)
    return m.eval().to("cuda")


def check_tables(table, tables, labels, max_runs, what=()):
    """a model method's (device tables [N, words], [(header, records)]) against runs_of on labels [N, H, W] (tensors); returns the runs found"""
    total = 0
    host = table.cpu().numpy()
    for i, (hdr, recs) in enumerate(tables):
        m = np.ascontiguousarray(labels[i].cpu().numpy())
        whdr, wrecs = runs_of(m, max_runs)
        assert (int(hdr["count"]), int(hdr["stored"]), int(hdr["status"]), int(hdr["reserved"])) == \
            (int(whdr["count"]), int(whdr["stored"]), int(whdr["status"]), 0), what + (i, hdr, whdr)
        assert recs.tolist() == wrecs.tolist(), what + (i,)
        cases.check_frame_table(host[i], m, max_runs, what + (i,))
        total += int(hdr["count"])
    return total


@pytest.mark.parametrize("name,opts,H,W,Hs,Ws", [("td4", None, 65, 129, 80, 161), ("td4", {"precision": 1}, 33, 65, 41, 83), ("td4", {"precision": 2}, 33, 65, 41, 83),
                                                 ("td2", None, 33, 65, 41, 83)],
                         ids=["td4-psp18-fp32-65x129", "td4-psp18-fp16-mode", "td4-psp18-precision2", "td2-psp18-fp32"])
def test_frames_coded_on_the_device_equal_the_oracle_on_their_labels(name, opts, H, W, Hs, Ws):
    """Six frames of random bytes.  Model B: forward_labels_u8; A: forward_u8_runs throughout (max_runs = H W); C in turn forward_u8_runs with a table that
    overflows, forward_labels_u8 + labels_runs, and encode_u8 + propagate_runs.  Same labels, the oracle's tables, the launch-count relation, the same
    FIFO; every table decoded on the device is the labels again, an overflowed one up to its closing start."""
    b = make_model(name, opts)
    b.ensure_engine(H, W, "cuda")
    a, c = (make_model(name, opts).share_weights_with(b) for _ in range(2))
    a.set_runs()
    P = b.path_num
    rng = np.random.default_rng(51)
    total = 0
    with torch.no_grad():
        for t in range(6):
            u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
            l8 = b.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            n_labels = b.engine.last_launch_count()
            got, table, tables = a.forward_u8_runs(u, t % P, (H, W))
            assert torch.equal(got, l8) and a.engine.last_launch_count() == n_labels - 1 + LAUNCHES, t
            count = check_tables(table, tables, l8, H * W, ("A", t))
            total += count
            assert torch.equal(a.runs_labels(table, 0xEE), l8), t
            small = max(count // 3, 1)
            c.set_runs((small, None, H * W)[t % 3])
            if t % 3 == 0:
                lc, table, tables = c.forward_u8_runs(u, t % P, (H, W))
                assert c.engine.last_launch_count() == n_labels - 1 + LAUNCHES
                check_tables(table, tables, l8, small, ("C overflow", t))
                hdr, recs = tables[0]
                assert int(hdr["status"]) == RUNS_OVERFLOW
                assert np.array_equal(c.runs_labels(table, 0xEE)[0].cpu().numpy(), runs_decode(hdr, recs, H, W, 0xEE, np.uint8))
            elif t % 3 == 1:
                lc = c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
                table, tables = c.labels_runs(lc)
                check_tables(table, tables, l8, H * W, ("C unfused", t))
            else:
                c.encode_u8(u, t % P, in_size=(H, W))
                lc, table, tables = c.propagate_runs()
                check_tables(table, tables, l8, H * W, ("C split", t))
            assert torch.equal(lc, l8), t
    assert a.engine.fifo_len() == b.engine.fifo_len() == c.engine.fifo_len() and total > 0


def test_pspnet_fp32_frames_and_no_label_map():
    """the stateless model through forward_runs; then the engine's entry with labels_dev = NULL: the same table, no label map anywhere"""
    from tdnet_amd import weights
    H, W = 33, 65
    m = make_model("psp")
    x = torch.from_numpy(weights.synth_video(H, W, 1, seed=3)[0]).cuda()
    with torch.no_grad():
        l32 = m.forward_labels(x)
        n_labels = m.engine.last_launch_count()
        m.set_runs()
        got, table, tables = m.forward_runs(x)
        assert m.engine.last_launch_count() == n_labels - 1 + LAUNCHES > 0
        assert torch.equal(got, l32.to(torch.uint8))
        check_tables(table, tables, got, H * W, ("pspnet",))
        bare = torch.full_like(table[0], -1)
        m.engine.forward_runs(x.data_ptr(), 0, None, bare.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert m.engine.last_launch_count() == n_labels - 1 + LAUNCHES
        torch.cuda.synchronize()
        count = int(tables[0][0]["count"])
        assert torch.equal(bare[:2 + count + 1], table[0][:2 + count + 1]) and bool((bare[2 + count + 1:] == -1).all())   # and nothing behind the closing record


def test_label_and_runs_entries_mixed_on_one_handle_with_fp32_frames():
    from tdnet_amd import weights
    H, W, Hs, Ws = 33, 65, 41, 83
    b = make_model("td2")
    b.ensure_engine(H, W, "cuda")
    a = make_model("td2").share_weights_with(b)
    a.set_runs(50)
    rng = np.random.default_rng(55)
    x = weights.synth_video(H, W, 6, seed=6)
    with torch.no_grad():
        for t in range(6):
            if t % 3 == 0:
                f = torch.from_numpy(x[t]).cuda()
                want = b.forward_labels(f, pos_id=t % 2).to(torch.uint8)
                n_labels = b.engine.last_launch_count()
                got, table, tables = a.forward_runs(f, t % 2)
            else:
                u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
                want = b.forward_labels_u8(u, pos_id=t % 2, in_size=(H, W))
                n_labels = b.engine.last_launch_count()
                if t % 3 == 1:
                    got, table, tables = a.forward_u8_runs(u, t % 2, (H, W))
                else:                                                  # a plain label frame between two coded ones
                    got = a.forward_labels_u8(u, pos_id=t % 2, in_size=(H, W))
                    assert a.engine.last_launch_count() == n_labels
            assert torch.equal(got, want), t
            if t % 3 != 2:
                assert a.engine.last_launch_count() == n_labels - 1 + LAUNCHES, t
                assert check_tables(table, tables, want, 50, ("mixed", t)) > 50 and int(tables[0][0]["status"]) == RUNS_OVERFLOW
    assert a.engine.fifo_len() == b.engine.fifo_len()


def test_regions_then_the_id_map_coded_and_decoded_back():
    H, W, Hs, Ws = 65, 129, 80, 161
    m = make_model("td4")
    m.set_regions(range(19), 8, 4096, 1)
    m.set_runs()
    rng = np.random.default_rng(56)
    with torch.no_grad():
        u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
        l8, ids, _ = m.forward_regions_u8(u, 0, (H, W))
        assert int(ids.max()) > 1
        table, tables = m.ids_runs(ids)
        hdr, recs = tables[0]
        whdr, wrecs = runs_of(ids[0].cpu().numpy())
        assert int(hdr["count"]) == int(whdr["count"]) and recs.tolist() == wrecs.tolist()
        assert torch.equal(m.runs_ids(table, -1), ids)
        odd = torch.from_numpy(cases.pattern("extremes", H, W, B, True).copy())[None].cuda()   # any int32 values
        table, tables = m.ids_runs(odd)
        assert tables[0][1].tolist() == runs_of(odd[0].cpu().numpy())[1].tolist()
        assert torch.equal(m.runs_ids(table, 0), odd)
        with pytest.raises(RuntimeError, match="int32 maps"):
            m.ids_runs(l8)
        with pytest.raises(RuntimeError, match="uint8 maps"):
            m.labels_runs(ids)


def test_a_captured_cycle_of_runs_frames_replays_to_the_eager_tables():
    """One pos_id cycle of tdnet_forward_u8_runs at 65x129 captured into a hipGraph (tdnet_warmup and tdnet_set_runs before the capture) and replayed twice:
    labels and tables -- the untouched tail included -- bit-equal to the eager frames'."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    warm = 2 * P
    T = warm + cycles * P
    nwords = 2 + H * W + 1
    rng = np.random.default_rng(54)
    clip = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(T)]
    with torch.no_grad():
        m = make_model("td4")
        m.set_runs()
        eager = []
        for t in range(T):
            l8, table, tables = m.forward_u8_runs(clip[t], t % P, (H, W))
            eager.append((l8.clone(), tables[0]))
        m.reset()
        for t in range(warm):                                          # steady state; the handle is configured (input and runs) by these frames
            l8, table, tables = m.forward_u8_runs(clip[t], t % P, (H, W))
            assert torch.equal(l8, eager[t][0]) and tables[0][1].tolist() == eager[t][1][1].tolist()
        e = m.engine
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        lab = torch.zeros((P, H, W), dtype=torch.uint8, device="cuda")
        tab = torch.zeros((P, nwords), dtype=torch.int64, device="cuda")
        e.warmup(stream.cuda_stream)
        e.set_runs(H * W)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for j in range(P):
                e.forward_u8_runs(xin[j].data_ptr(), j, lab[j].data_ptr(), tab[j].data_ptr(), torch.cuda.current_stream().cuda_stream)
        found = 0
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            lab.fill_(0xEE); tab.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            host = tab.cpu().numpy()
            for j in range(P):
                want_l8, (want_hdr, want_recs) = eager[t0 + j]
                assert torch.equal(lab[j], want_l8[0]), (c, j)
                hdr, recs = run_table(host[j])
                assert hdr.tobytes() == want_hdr.tobytes() and recs.tobytes() == want_recs.tobytes(), (c, j)
                assert (host[j][2 + len(recs):] == -1).all(), (c, j)
                found += int(hdr["count"])
    assert found > 0


def test_the_downloader_fetches_a_short_prefix_with_a_second_copy():
    """a clip whose run count jumps: constant maps (H runs), then noise (about 2/3 H W): the prefix sized from the previous count is short"""
    H, W = 65, 129
    m = make_model("td2")
    m.ensure_engine(H, W, "cuda")
    m.set_runs()
    maps = [cases.pattern(n, H, W, B) for n in ("constant", "constant", "noise3", "noise3", "stripes64", "alternating", "constant")]
    down = RunsDownloader("cuda")
    got = []
    for t, mp in enumerate(maps):
        table, _ = m.labels_runs(torch.from_numpy(mp.copy())[None].cuda())
        for tag, hdr, recs in down.submit(table[0], t):
            got.append((tag, hdr.copy(), recs.copy()))
        if t in (1, 3, 4):                                             # let the count of this frame be known before the next is submitted
            for tag, hdr, recs in down.drain():
                got.append((tag, hdr.copy(), recs.copy()))
    for tag, hdr, recs in down.drain():
        got.append((tag, hdr.copy(), recs.copy()))
    assert [g[0] for g in got] == list(range(len(maps)))
    for tag, hdr, recs in got:
        whdr, wrecs = runs_of(maps[tag])
        assert hdr.tobytes() == whdr.tobytes() and recs.dtype == RUN_DTYPE and recs.tolist() == wrecs.tolist(), tag
    assert down.short >= 2                                             # constant -> noise3 and stripes64 -> alternating at the least


def test_errors_name_the_call_and_leave_a_pending_frame_alone():
    H, W, Hs, Ws = 33, 65, 41, 83
    m, ref = make_model("td2"), make_model("td2")
    rng = np.random.default_rng(53)
    u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="set_runs"):
            m.forward_u8_runs(u, 0, (H, W))
        for bad in (0, -3, 1.5, True):
            with pytest.raises(RuntimeError, match="set_runs"):
                m.set_runs(bad)
        m.set_runs(H * W + 1)
        with pytest.raises(RuntimeError, match="max_runs"):
            m.forward_u8_runs(u, 0, (H, W))
        m.encode_u8(u, 0, in_size=(H, W))
        e = m.engine
        s = torch.cuda.current_stream().cuda_stream
        lab = torch.full((H, W), 0xEE, dtype=torch.uint8, device="cuda")
        ids = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
        table = torch.full((2 + 8 + 1 + 1,), -1, dtype=torch.int64, device="cuda")
        calls = lambda tp: (lambda: e.forward_u8_runs(u.data_ptr(), 1, lab.data_ptr(), tp, s), lambda: e.propagate_runs(lab.data_ptr(), tp, s),
                            lambda: e.labels_runs(lab.data_ptr(), tp, s), lambda: e.ids_runs(ids.data_ptr(), tp, s),
                            lambda: e.runs_labels(tp, 0, lab.data_ptr(), s), lambda: e.runs_ids(tp, 0, ids.data_ptr(), s))
        for call in calls(table.data_ptr()):
            with pytest.raises(_capi.TdnetError, match="tdnet_set_runs"):
                call()
        assert e.runs_bytes() == 0
        _, before, _ = e.memory_bytes()
        for bad in (0, H * W + 1):
            with pytest.raises(_capi.TdnetError, match="max_runs"):
                e.set_runs(bad)
        assert e.runs_bytes() == 0 and e.memory_bytes()[1] == before
        e.set_runs(8)
        assert e.runs_bytes() == 16 + 8 * 9 and e.memory_bytes()[1] == before + H * W + 4 * ((H * W // 4 + 2 + 255) // 256)
        for off in (1, 4):
            for call in calls(table.data_ptr() + off):
                with pytest.raises(_capi.TdnetError, match="runs_dev = 0x[0-9a-f]+ is not 8-byte aligned"):
                    call()
        for call in calls(None):
            with pytest.raises(_capi.TdnetError, match="runs_dev is NULL"):
                call()
        with pytest.raises(_capi.TdnetError, match="ids_dev = 0x[0-9a-f]+ is not 4-byte aligned"):
            e.ids_runs(ids.data_ptr() + 2, table.data_ptr(), s)
        with pytest.raises(_capi.TdnetError, match="ids_dev = 0x[0-9a-f]+ is not 4-byte aligned"):
            e.runs_ids(table.data_ptr(), 0, ids.data_ptr() + 1, s)
        with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):
            e.forward_u8_runs(u.data_ptr(), 1, lab.data_ptr(), table.data_ptr(), s)
        torch.cuda.synchronize()
        assert bool((lab == 0xEE).all()) and bool((ids == -7).all()) and bool((table == -1).all()) and e.fifo_len() == 0
        m.set_runs(8)
        got, tab, tables = m.propagate_runs()                          # the pending frame is still there, and is the frame it was
        want = ref.forward_labels_u8(u, pos_id=0, in_size=(H, W))
        assert torch.equal(got, want)
        check_tables(tab, tables, want, 8)
        with pytest.raises(RuntimeError, match="no encoded frame"):
            m.propagate_runs()
        with pytest.raises(_capi.TdnetError, match="no encoded frame"):
            e.propagate_runs(lab.data_ptr(), table.data_ptr(), s)


def test_cli_writes_the_records_of_the_oracle_and_the_usual_pictures(tmp_path):
    """Five random 80x161 frames, --in_size 65x129 --u8 --runs --runs_out DIR: one .npy per frame, the oracle's records on the labels the library gives for
    the same frames; the PNGs are byte for byte those of the run without --runs."""
    from PIL import Image
    from tdnet_amd.dataloader import cityscapesLoader
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(17)
    H, W = 65, 129
    for t in range(5):
        Image.fromarray(rng.integers(0, 256, (80, 161, 3), dtype=np.uint8)).save(frames_dir / ("frame_%06d.png" % t))
    ld = cityscapesLoader(img_path=str(tmp_path / "data"), in_size=(H, W), as_uint8=True)
    ld.load_frames()
    m = make_model("td4")
    want = {}
    with torch.no_grad():
        for t, item in enumerate(ld.data):
            l8 = m.forward_labels_u8(item[0].cuda(), pos_id=t % 4, in_size=(H, W))
            want[os.path.splitext(item[1])[0] + ".npy"] = runs_of(l8[0].cpu().numpy())[1]
    base = [sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--synthetic_seed", "0", "--in_size", "65x129", "--u8"]
    out, plain, npys = tmp_path / "out", tmp_path / "plain", tmp_path / "npy"
    out.mkdir(); plain.mkdir()
    r = subprocess.run(base + ["--output_path", str(out), "--runs", "--runs_out", str(npys)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(npys / "vid1")) == sorted(want)
    for name, recs in want.items():
        got = np.load(npys / "vid1" / name)
        assert got.dtype == RUN_DTYPE and got.tolist() == recs.tolist() and len(got) > 2, name
    r = subprocess.run(base + ["--output_path", str(plain)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out / "vid1")) == sorted(os.listdir(plain / "vid1")) and len(os.listdir(out / "vid1")) == 5
    for name in os.listdir(out / "vid1"):
        assert open(out / "vid1" / name, "rb").read() == open(plain / "vid1" / name, "rb").read(), name
    r = subprocess.run(base + ["--output_path", str(out), "--runs_out", str(npys)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--runs [MAX_RUNS]" in r.stderr
