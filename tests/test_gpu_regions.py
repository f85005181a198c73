"""Regions out on the MI355X: the operator cases of tests/test_emu_regions.py on device memory between guard bands (128x256 is 32 tiles and more: the
border merge really spans the XCDs), whole frames through the model classes against the flood-fill oracle on the labels the label entries give, a
captured pos_id cycle, and the command line with --regions.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opcheck
import out_cases
import regions_cases as cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import REGIONS_BOUND, region_table, regions_u8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = 7                                                           # include/tdnet.h TDNET_REGIONS_LAUNCHES
TH, TW = 16, 64                                                        # csrc/td_regions.h's tile; test_the_tile_is_the_one_the_cases_are_sized_for holds it to the library's


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


def test_the_tile_is_the_one_the_cases_are_sized_for(lib):
    assert cases.tile(lib) == (TH, TW)


@pytest.mark.parametrize("shape", cases.shapes(TH, TW), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.PATTERNS)
def test_patterns_against_the_flood_fill(lib, name, shape):
    counts = cases.check_pattern(lib, opcheck.GuardedTorchMem(), name, shape[0], shape[1], TH, TW)
    H, W = shape
    if name in ("one", "comb"):
        assert counts == [1, 1]
    if name == "checker" and H * W > 1:
        assert counts[0] == H * W and counts[1] == (2 if min(H, W) > 1 else H * W)
    if name in ("diag_back", "diag_fwd") and min(H, W) > 1:
        assert counts[0] > counts[1] >= 1


def test_overflow_sets_the_status_bit_and_ids_run_on(lib):
    H, W = 128, 256
    labels, classes = cases.pattern("checker", H, W, TH, TW)
    ids, hdr, recs, _ = cases.run_op(lib, opcheck.GuardedTorchMem(), H, W, classes, 4, 64, 1, labels=labels)
    assert cases.compare((ids, hdr, recs), labels, classes, 4, 1, 64) == H * W
    assert int(hdr["status"]) == 1 and int(hdr["stored"]) == 64 and np.array_equal(ids.reshape(-1), np.arange(1, H * W + 1))


@pytest.mark.parametrize("shape", [(33, 65), (128, 256)], ids=lambda s: "%dx%d" % s)
def test_parameters_on_the_noise_map(lib, shape):
    cases.check_parameters(lib, opcheck.GuardedTorchMem(), *shape)


@pytest.mark.parametrize("field", out_cases.FIELDS)
@pytest.mark.parametrize("case", out_cases.CASES, ids=out_cases.case_id)
def test_from_logits_the_labels_are_the_label_kernels(lib, case, field):
    C, (h, w), (H, W) = case
    x = out_cases.logits(field, C, h, w)
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    dx = torch.from_numpy(x.copy()).cuda()
    lib.check(lib.tdnet_op_upsample_argmax(dx.data_ptr(), C, h, w, H, W, l32.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    cases.check_from_logits(lib, opcheck.GuardedTorchMem(), x, C, h, w, H, W, l32.cpu().numpy().astype(np.uint8))


def test_from_logits_across_many_tiles(lib):
    """19 classes, 17x33 -> 129x257: every tile position (first, inner, last partial row and column) computes its own labels"""
    C, h, w, H, W = 19, 17, 33, 129, 257
    x = np.random.default_rng(7).standard_normal((C, h, w)).astype(np.float32)
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    dx = torch.from_numpy(x).cuda()
    lib.check(lib.tdnet_op_upsample_argmax(dx.data_ptr(), C, h, w, H, W, l32.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    cases.check_from_logits(lib, opcheck.GuardedTorchMem(), x, C, h, w, H, W, l32.cpu().numpy().astype(np.uint8))


def test_an_odd_table_pointer_is_refused_and_the_bound_bit_stays_clear(lib):
    H, W = 128, 256
    mem = opcheck.GuardedTorchMem()
    labels, classes = cases.pattern("spiral", H, W, TH, TW)
    lab_t, lab_p = cases.put_bytes(mem, labels)
    ids_t, tab_t = mem.empty((H, W)), mem.empty((cases.words(16 + 48 * 4) + 2,))
    cls = np.ascontiguousarray(classes, np.uint8)
    for off in (1, 2, 4, 7):
        rc = lib.tdnet_op_regions(None, 19, 0, 0, H, W, lab_p, None, cls.ctypes.data, 1, 8, 4, 1, mem.ptr(ids_t), mem.ptr(tab_t) + off, mem.stream)
        assert rc != 0 and b"regions_dev = 0x" in lib.tdnet_last_error() and b"not 8-byte aligned" in lib.tdnet_last_error()
    mem.verify(untouched=True)
    for name in ("spiral", "one", "noise"):                            # the deepest chains, the most contended unions
        labels, classes = cases.pattern(name, H, W, TH, TW)
        _, hdr, _, _ = cases.run_op(lib, opcheck.GuardedTorchMem(), H, W, classes, 8, 16, 1, labels=labels, want_ids=False)
        assert not int(hdr["status"]) & REGIONS_BOUND, name


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
CLASSES, CONN, MAXR, MIN_AREA = (0, 2, 5, 8, 11, 13, 17), 8, 64, 2


def make_model(name):
    from tdnet_amd.model import td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0)
    else:
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0)
    return m.eval().to("cuda")


def check_tables(ids, tables, labels, conn=CONN, min_area=MIN_AREA, max_regions=MAXR, what=()):
    """a model method's (ids [N, H, W] or None, [RegionTable]) against the oracle on labels [N, H, W] (tensors); returns the regions found"""
    total = 0
    for i, t in enumerate(tables):
        want_ids, count, table = cases.oracle(np.ascontiguousarray(labels[i].cpu().numpy()), CLASSES, conn, min_area, max_regions)
        assert (t.count, len(t), t.status) == (count, min(count, max_regions), int(count > max_regions)), what + (i, t.count, count)
        assert t.tolist() == table.tolist(), what + (i,)
        if ids is not None:
            assert np.array_equal(ids[i].cpu().numpy(), want_ids), what + (i,)
        total += count
    return total


@pytest.mark.parametrize("name,H,W,Hs,Ws", [("td4", 65, 129, 80, 161), ("td2", 33, 65, 41, 83), ("td4", 33, 65, 41, 83), ("td2", 65, 129, 80, 161)],
                         ids=["td4-65x129", "td2-33x65", "td4-33x65", "td2-65x129"])
def test_frames_labelled_on_the_device_equal_the_oracle_on_their_labels(name, H, W, Hs, Ws):
    """Six frames of random bytes.  Model B: forward_labels_u8; A: forward_regions_u8 throughout; C in turn forward_regions_u8, forward_labels_u8 +
    regions_labels, and encode_u8 + propagate_regions.  Same labels, the oracle's ids and tables, the launch-count relation, the same FIFO."""
    b = make_model(name)
    b.ensure_engine(H, W, "cuda")
    a, c = (make_model(name).share_weights_with(b) for _ in range(2))
    for m in (a, c):
        m.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
    P = b.path_num
    rng = np.random.default_rng(41)
    total = 0
    with torch.no_grad():
        for t in range(6):
            u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
            l8 = b.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            n_labels = b.engine.last_launch_count()
            got, ids, tables = a.forward_regions_u8(u, t % P, (H, W), return_ids=t % 2 == 0)
            assert torch.equal(got, l8) and (ids is None) == bool(t % 2), t
            assert a.engine.last_launch_count() == n_labels - 1 + LAUNCHES, t
            total += check_tables(ids, tables, l8, what=("A", t))
            if t % 3 == 0:
                lc, ids, tables = c.forward_regions_u8(u, t % P, (H, W))
                assert c.engine.last_launch_count() == n_labels - 1 + LAUNCHES
            elif t % 3 == 1:
                lc = c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
                _, ids, tables = c.regions_labels(lc)
            else:
                c.encode_u8(u, t % P, in_size=(H, W))
                lc, ids, tables = c.propagate_regions()
            assert torch.equal(lc, l8), t
            check_tables(ids, tables, l8, what=("C", t))
    assert a.engine.fifo_len() == b.engine.fifo_len() == c.engine.fifo_len() and total > 0


def test_fp32_frames_mixed_with_byte_frames_and_rejected_pixels():
    H, W, Hs, Ws = 33, 65, 41, 83
    from tdnet_amd import weights
    b = make_model("td2")
    b.ensure_engine(H, W, "cuda")
    a = make_model("td2").share_weights_with(b)
    a.set_regions(CLASSES, 4, 3, 1)                                    # 3 records: the table overflows, the ids run on
    rng = np.random.default_rng(45)
    x = weights.synth_video(H, W, 4, seed=6)
    with torch.no_grad():
        for t in range(4):
            if t % 2:
                f = torch.from_numpy(x[t]).cuda()
                want = b.forward_labels(f, pos_id=t % 2).to(torch.uint8)
                n_labels = b.engine.last_launch_count()
                got, ids, tables = a.forward_regions(f, t % 2)
            else:
                u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
                want = b.forward_labels_u8(u, pos_id=t % 2, in_size=(H, W))
                n_labels = b.engine.last_launch_count()
                got, ids, tables = a.forward_regions_u8(u, t % 2, (H, W))
            assert torch.equal(got, want) and a.engine.last_launch_count() == n_labels - 1 + LAUNCHES, t
            assert check_tables(ids, tables, want, 4, 1, 3, ("mixed", t)) > 3 and tables[0].status == 1
        # the confidence entry's labels, rejected pixels 255, through the unfused entry: in no region
        u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
        b.reset()
        _, conf = b.forward_labels_conf_u8(u, 0, (H, W))               # nothing rejected: the frame's confidence bytes, for a threshold that splits them
        b.reset()
        b.set_confidence((int(np.median(conf.cpu().numpy())) + 1) / 255.0, 255)
        l8, _ = b.forward_labels_conf_u8(u, 0, (H, W))
        rejected = (l8 == 255)
        assert 0 < int(rejected.sum()) < H * W
        a.set_regions(range(19), 8, 256, 1)
        _, ids, tables = a.regions_labels(l8)
        want_ids, count, table = regions_u8(l8[0].cpu().numpy(), range(19), 8, 1, 256)
        assert np.array_equal(ids[0].cpu().numpy(), want_ids) and tables[0].tolist() == table.tolist() and tables[0].count == count
        assert not bool(ids[rejected].any()) and bool((ids[~rejected] > 0).all())


def test_errors_name_the_call_and_leave_a_pending_frame_alone():
    H, W, Hs, Ws = 33, 65, 41, 83
    m, ref = make_model("td2"), make_model("td2")
    rng = np.random.default_rng(43)
    u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="set_regions"):
            m.forward_regions_u8(u, 0, (H, W))
        for bad in (dict(classes=(19,)), dict(classes=(3,), connectivity=6), dict(classes=(3,), max_regions=0), dict(classes=(3,), min_area=0)):
            with pytest.raises(RuntimeError, match="set_regions"):
                m.set_regions(**bad)
        m.encode_u8(u, 0, in_size=(H, W))
        e = m.engine
        lab = torch.full((H, W), 0xEE, dtype=torch.uint8, device="cuda")
        ids = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
        table = torch.full((2 + 6 * 8 + 1,), -1, dtype=torch.int64, device="cuda")
        for call in (lambda: e.forward_u8_regions(u.data_ptr(), 1, lab.data_ptr(), ids.data_ptr(), table.data_ptr()),
                     lambda: e.propagate_regions(lab.data_ptr(), ids.data_ptr(), table.data_ptr()),
                     lambda: e.labels_regions(lab.data_ptr(), ids.data_ptr(), table.data_ptr())):
            with pytest.raises(_capi.TdnetError, match="tdnet_set_regions"):
                call()
        _, before, _ = e.memory_bytes()
        with pytest.raises(_capi.TdnetError, match="connectivity"):
            e.set_regions((3,), 5, 8, 1)
        assert e.regions_bytes() == 0 and e.memory_bytes()[1] == before
        e.set_regions(CLASSES, 8, 8, 1)
        assert e.regions_bytes() == 16 + 48 * 8 and e.memory_bytes()[1] == before + 13 * H * W + 4 * ((H * W + 1023) // 1024) + 4
        for call in (lambda: e.forward_u8_regions(u.data_ptr(), 1, lab.data_ptr(), ids.data_ptr(), table.data_ptr() + 4),
                     lambda: e.propagate_regions(lab.data_ptr(), ids.data_ptr(), table.data_ptr() + 1),
                     lambda: e.labels_regions(lab.data_ptr(), ids.data_ptr(), table.data_ptr() + 2)):
            with pytest.raises(_capi.TdnetError, match="regions_dev = 0x[0-9a-f]+ is not 8-byte aligned"):
                call()
        with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):
            e.forward_u8_regions(u.data_ptr(), 1, lab.data_ptr(), ids.data_ptr(), table.data_ptr())
        torch.cuda.synchronize()
        assert bool((lab == 0xEE).all()) and bool((ids == -7).all()) and bool((table == -1).all()) and e.fifo_len() == 0
        m.set_regions(CLASSES, 8, 8, 1)
        got, gids, tables = m.propagate_regions()                      # the pending frame is still there, and is the frame it was
        want = ref.forward_labels_u8(u, pos_id=0, in_size=(H, W))
        assert torch.equal(got, want)
        check_tables(gids, tables, want, 8, 1, 8)
        with pytest.raises(RuntimeError, match="no encoded frame"):
            m.propagate_regions()
        with pytest.raises(_capi.TdnetError, match="no encoded frame"):   # the engine's own message for the same state
            e.propagate_regions(lab.data_ptr(), ids.data_ptr(), table.data_ptr())
        with pytest.raises(RuntimeError, match="uint8 labels"):
            m.regions_labels(want.float())


def test_a_captured_cycle_of_region_frames_replays_to_the_eager_tables():
    """One pos_id cycle of tdnet_forward_u8_regions at 65x129 captured into a hipGraph (tdnet_warmup and tdnet_set_regions before the capture) and replayed
    twice: labels, ids and tables bit-equal to the eager frames'."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    warm = 2 * P
    T = warm + cycles * P
    nwords = 2 + 6 * MAXR
    rng = np.random.default_rng(44)
    clip = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(T)]
    with torch.no_grad():
        m = make_model("td4")
        m.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
        eager = []
        for t in range(T):
            l8, ids, tables = m.forward_regions_u8(clip[t], t % P, (H, W))
            eager.append((l8.clone(), ids.clone(), tables[0]))
        m.reset()
        for t in range(warm):                                          # steady state; the handle is configured (input and regions) by these frames
            l8, ids, tables = m.forward_regions_u8(clip[t], t % P, (H, W))
            assert torch.equal(l8, eager[t][0]) and torch.equal(ids, eager[t][1]) and tables[0].tolist() == eager[t][2].tolist()
        e = m.engine
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        lab = torch.zeros((P, H, W), dtype=torch.uint8, device="cuda")
        ids = torch.zeros((P, H, W), dtype=torch.int32, device="cuda")
        tab = torch.zeros((P, nwords), dtype=torch.int64, device="cuda")
        e.warmup(stream.cuda_stream)
        e.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for j in range(P):
                e.forward_u8_regions(xin[j].data_ptr(), j, lab[j].data_ptr(), ids[j].data_ptr(), tab[j].data_ptr(), torch.cuda.current_stream().cuda_stream)
        found = 0
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            lab.fill_(0xEE); ids.fill_(-7); tab.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            host = tab.cpu().numpy()
            for j in range(P):
                want_l8, want_ids, want_table = eager[t0 + j]
                assert torch.equal(lab[j], want_l8[0]) and torch.equal(ids[j], want_ids[0]), (c, j)
                got = region_table(host[j], MAXR)
                assert (got.count, got.status) == (want_table.count, want_table.status) and got.tobytes() == want_table.tobytes(), (c, j)
                assert not got.status & REGIONS_BOUND
                found += got.count
    assert found > 0


def test_cli_writes_the_csvs_of_the_oracle(tmp_path):
    """Five random 80x161 frames, --in_size 65x129 --u8 --regions ... --regions_out DIR: one CSV per frame, equal as text to the oracle's records on the labels
    the library gives for the same frames."""
    from PIL import Image
    from tdnet_amd.dataloader import cityscapesLoader
    from tdnet_amd.test import regions_csv
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(16)
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
            _, count, table = regions_u8(l8[0].cpu().numpy(), (0, 2, 5, 8, 11), 4, 3, 4096)
            want[os.path.splitext(item[1])[0] + ".csv"] = regions_csv(table)
    out, csvs = tmp_path / "out", tmp_path / "csv"
    out.mkdir()
    r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0",
                        "--in_size", "65x129", "--u8", "--regions", "0,2,5,8,11", "--regions_conn", "4", "--regions_min_area", "3", "--regions_out", str(csvs)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(csvs / "vid1")) == sorted(want)
    for name, text in want.items():
        assert open(csvs / "vid1" / name).read() == text, name
        assert text.count("\n") > 1
    assert len(os.listdir(out / "vid1")) == 5 and "regions" in r.stdout
    r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0",
                        "--in_size", "65x129", "--regions_conn", "4"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--regions IDS" in r.stderr
