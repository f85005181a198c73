"""Tracks out on the MI355X: the operator families of tests/test_emu_tracks.py on device memory between guard bands (128x256 is 32 workgroups a launch:
the pair table is really shared across the XCDs, and the checker at that size fills it with a pair per pixel), whole frames through the model classes
against TrackOracle on the labels the label entries give, a captured pos_id cycle replayed so that the tracks go on from replay to replay, and the command
line with --tracks.  Every comparison is exact; status == 0 everywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opcheck
import regions_cases
import tracks_cases as cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import TrackOracle, track_table

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIONS_LAUNCHES, LAUNCHES = 7, 4                                      # include/tdnet.h TDNET_REGIONS_LAUNCHES, TDNET_TRACKS_LAUNCHES
TH, TW = 16, 64                                                        # csrc/td_regions.h's tile; held to the library's answer in the lib fixture


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    lib = _capi.test_lib()
    assert regions_cases.tile(lib) == (TH, TW)
    return lib


@pytest.mark.parametrize("shape", cases.shapes(TH, TW), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", cases.FAMILIES)
def test_families_against_the_oracle(lib, name, shape):
    steps = cases.check_family(lib, opcheck.GuardedTorchMem(), name, *shape)
    assert all(int(s[3]["status"]) == 0 for s in steps)                # (compare() held the device's status word to this one)


@pytest.mark.parametrize("shape", [(33, 65), (128, 256)], ids=lambda s: "%dx%d" % s)
def test_label_map_offsets_and_maps_left_out(lib, shape):
    cases.check_parameters(lib, opcheck.GuardedTorchMem(), *shape)


def test_odd_table_pointers_are_refused_and_nothing_is_written(lib):
    H, W = 33, 65
    mem = opcheck.GuardedTorchMem()
    labels = regions_cases.noise(H, W)
    lab_t, lab_p = cases.put_bytes(mem, labels)
    state = cases.new_state(lib, mem, H, W)
    ids_t, map_t = mem.empty((H, W)), mem.empty((H, W))
    rtab_t, ttab_t = mem.empty((cases.words(16 + 48 * 4) + 2,)), mem.empty((cases.words(16 + 24 * 4) + 2,))
    cls = np.array([3, 7, 11], np.uint8)

    def call(state_p, rtab_p, ttab_p, min_overlap=1):
        return lib.tdnet_op_tracks(lab_p, 19, H, W, cls.ctypes.data, 3, 8, 4, 1, min_overlap, state_p, mem.ptr(ids_t), rtab_p, mem.ptr(map_t), ttab_p, mem.stream)

    for off in (1, 2, 4, 7):
        assert call(mem.ptr(state), mem.ptr(rtab_t), mem.ptr(ttab_t) + off) != 0 and b"tracks_dev = 0x" in lib.tdnet_last_error()
        assert call(mem.ptr(state), mem.ptr(rtab_t) + off, mem.ptr(ttab_t)) != 0 and b"regions_dev = 0x" in lib.tdnet_last_error()
    assert call(mem.ptr(state) + 8, mem.ptr(rtab_t), mem.ptr(ttab_t)) != 0 and b"state_dev" in lib.tdnet_last_error()
    assert call(mem.ptr(state), mem.ptr(rtab_t), None) != 0 and b"tracks_dev is NULL" in lib.tdnet_last_error()
    assert call(mem.ptr(state), mem.ptr(rtab_t), mem.ptr(ttab_t), 0) != 0 and b"min_overlap" in lib.tdnet_last_error()
    assert not bool(state.view(torch.int32).any())
    mem.verify(untouched=True)


# ---- whole frames ------------------------------------------------------------------------------------------------------------------
CLASSES, CONN, MAXR, MIN_AREA, MIN_OVERLAP = (0, 2, 5, 8, 11, 13, 17), 8, 64, 2, 2


def make_model(name):
    from tdnet_amd.model import td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0)
    else:
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0)
    return m.eval().to("cuda")


def check_step(got, want, what=()):
    """a model method's (labels, ids or None, [RegionTable], track map or None, [TrackTable]) for ONE sample against an oracle step"""
    _, ids, tables, tmap, tracks = got
    want_ids, table, want_map, hdr, recs = want
    assert tables[0].tolist() == table.tolist(), what
    assert ids is None or np.array_equal(ids[0].cpu().numpy(), want_ids), what
    assert tmap is None or np.array_equal(tmap[0].cpu().numpy(), want_map), what
    t = tracks[0]
    assert (len(t), t.matched, t.ended, t.status) == (int(hdr["count"]), int(hdr["matched"]), int(hdr["ended"]), 0), what + (t.matched, t.ended, t.status, hdr)
    assert t.tolist() == recs.tolist(), what


@pytest.mark.parametrize("name,H,W,Hs,Ws", [("td2", 33, 65, 41, 83), ("td4", 33, 65, 41, 83), ("td4", 65, 129, 80, 161), ("td2", 65, 129, 80, 161)],
                         ids=["td2-33x65", "td4-33x65", "td4-65x129", "td2-65x129"])
def test_tracked_frames_equal_the_oracle_on_their_labels(name, H, W, Hs, Ws):
    """Six frames of random bytes.  Model B: forward_labels_u8; R: forward_regions_u8; A: forward_tracks_u8 throughout; C in turn forward_tracks_u8,
    forward_labels_u8 + labels_tracks (with an untracked regions call in between), and encode_u8 + propagate_tracks.  The oracle's tables and maps, the regions
    entry's labels, ids and table, the launch-count relation, the same FIFO."""
    b = make_model(name)
    b.ensure_engine(H, W, "cuda")
    r, a, c = (make_model(name).share_weights_with(b) for _ in range(3))
    for m in (r, a, c):
        m.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
    for m in (a, c):
        m.set_tracks(MIN_OVERLAP)
    P = b.path_num
    rng = np.random.default_rng(47)
    oracle = TrackOracle(CLASSES, CONN, MIN_AREA, MAXR, MIN_OVERLAP)
    matched = 0
    with torch.no_grad():
        for t in range(6):
            u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
            l8 = b.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            want = oracle.step(np.ascontiguousarray(l8[0].cpu().numpy()))
            matched += int(want[3]["matched"])
            rl, rids, rtables = r.forward_regions_u8(u, t % P, (H, W))
            got = a.forward_tracks_u8(u, t % P, (H, W), return_ids=t % 2 == 0, return_track_ids=t % 3 != 1)
            assert a.engine.last_launch_count() == r.engine.last_launch_count() + LAUNCHES == b.engine.last_launch_count() - 1 + REGIONS_LAUNCHES + LAUNCHES, t
            assert torch.equal(got[0], l8) and (got[1] is None) == bool(t % 2) and (got[3] is None) == (t % 3 == 1), t
            assert got[1] is None or torch.equal(got[1], rids)
            assert got[2][0].tobytes() == rtables[0].tobytes() and got[2][0].count == rtables[0].count
            check_step(got, want, ("A", t))
            if t % 3 == 0:
                gc = c.forward_tracks_u8(u, t % P, (H, W))
            elif t % 3 == 1:
                lc = c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
                c.regions_labels(torch.flip(lc, (2,)))                 # an untracked call in between: the track state stays
                gc = c.labels_tracks(lc)
            else:
                c.encode_u8(u, t % P, in_size=(H, W))
                gc = c.propagate_tracks()
            assert torch.equal(gc[0], l8), t
            check_step(gc, want, ("C", t))
        assert a.engine.fifo_len() == b.engine.fifo_len() == c.engine.fifo_len() and matched > 0
        a.reset_tracks()                                               # enqueued: the same labels again are all born, from 1
        got = a.labels_tracks(l8)
        oracle.reset()
        check_step(got, oracle.step(np.ascontiguousarray(l8[0].cpu().numpy())), ("reset",))
        assert got[4][0].matched == 0 and got[4][0]["track"].tolist() == list(range(1, len(got[4][0]) + 1))


def test_errors_name_the_missing_call():
    H, W, Hs, Ws = 33, 65, 41, 83
    m = make_model("td2")
    u = torch.from_numpy(np.random.default_rng(48).integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="set_regions"):
            m.forward_tracks_u8(u, 0, (H, W))
        m.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
        with pytest.raises(RuntimeError, match="set_tracks"):
            m.forward_tracks_u8(u, 0, (H, W))
        with pytest.raises(RuntimeError, match="min_overlap"):
            m.set_tracks(0)
        m.encode_u8(u, 0, in_size=(H, W))
        e = m.engine
        lab = torch.full((H, W), 0xEE, dtype=torch.uint8, device="cuda")
        ids, tmap = (torch.full((H, W), -7, dtype=torch.int32, device="cuda") for _ in range(2))
        rtab, ttab = torch.full((2 + 6 * MAXR,), -1, dtype=torch.int64, device="cuda"), torch.full((2 + 3 * MAXR + 1,), -1, dtype=torch.int64, device="cuda")
        with pytest.raises(_capi.TdnetError, match="tdnet_set_regions"):
            e.propagate_tracks(lab.data_ptr(), ids.data_ptr(), rtab.data_ptr(), tmap.data_ptr(), ttab.data_ptr())
        e.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
        with pytest.raises(_capi.TdnetError, match="tdnet_set_tracks"):
            e.propagate_tracks(lab.data_ptr(), ids.data_ptr(), rtab.data_ptr(), tmap.data_ptr(), ttab.data_ptr())
        with pytest.raises(_capi.TdnetError, match="min_overlap"):
            e.set_tracks(0)
        e.set_tracks(1)
        assert e.tracks_bytes() == 16 + 24 * MAXR
        for off in (1, 4):
            with pytest.raises(_capi.TdnetError, match="tracks_dev = 0x[0-9a-f]+ is not 8-byte aligned"):
                e.propagate_tracks(lab.data_ptr(), ids.data_ptr(), rtab.data_ptr(), tmap.data_ptr(), ttab.data_ptr() + off)
        with pytest.raises(_capi.TdnetError, match="tracks_dev is NULL"):
            e.propagate_tracks(lab.data_ptr(), ids.data_ptr(), rtab.data_ptr(), tmap.data_ptr(), None)
        torch.cuda.synchronize()
        assert bool((lab == 0xEE).all()) and bool((ids == -7).all()) and bool((tmap == -7).all()) and bool((rtab == -1).all()) and bool((ttab == -1).all())
        assert e.fifo_len() == 0
        m.set_tracks(1)
        got = m.propagate_tracks()                                     # the pending frame is still there
        assert got[4][0].status == 0 and got[4][0].matched == 0 and e.fifo_len() == 1


def test_a_captured_cycle_of_tracked_frames_replays_and_the_tracks_go_on():
    """One pos_id cycle of tdnet_forward_u8_tracks at 65x129 captured into a hipGraph on one stream (tdnet_warmup and the configuration before the capture)
    and replayed twice: labels, ids, track maps and both tables bit-equal to the eager frames' -- the second replay goes on from the first one's state (born ids
    carry on from next), since all state between frames lives at fixed device addresses.  Then, on label maps whose tracks are known to live (two noise maps in
    turn: the component that spans the map continues from frame to frame), a captured pair of tdnet_labels_tracks calls: ages and next carry on through two
    eager calls and two replays."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    warm = 2 * P
    T = warm + cycles * P
    rng = np.random.default_rng(49)
    base = rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)
    clip = []
    for t in range(T):                                                 # a slowly changing clip, so that tracks really live for many frames
        f = base.copy()
        f[:, :, (5 * t) % Ws:(5 * t) % Ws + 9] = rng.integers(0, 256, f[:, :, (5 * t) % Ws:(5 * t) % Ws + 9].shape, dtype=np.uint8)
        clip.append(torch.from_numpy(f).cuda())
    with torch.no_grad():
        m = make_model("td4")
        m.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
        m.set_tracks(MIN_OVERLAP)
        eager = []
        for t in range(T):
            l8, ids, tables, tmap, tracks = m.forward_tracks_u8(clip[t], t % P, (H, W))
            eager.append((l8.clone(), ids.clone(), tables[0], tmap.clone(), tracks[0]))
        m.reset()
        m.reset_tracks()
        for t in range(warm):
            l8, ids, tables, tmap, tracks = m.forward_tracks_u8(clip[t], t % P, (H, W))
            assert torch.equal(l8, eager[t][0]) and torch.equal(tmap, eager[t][3]) and tracks[0].tobytes() == eager[t][4].tobytes()
        e = m.engine
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        lab = torch.zeros((P, H, W), dtype=torch.uint8, device="cuda")
        ids, tmap = (torch.zeros((P, H, W), dtype=torch.int32, device="cuda") for _ in range(2))
        rtab = torch.zeros((P, 2 + 6 * MAXR), dtype=torch.int64, device="cuda")
        ttab = torch.zeros((P, 2 + 3 * MAXR), dtype=torch.int64, device="cuda")
        e.warmup(stream.cuda_stream)
        e.set_regions(CLASSES, CONN, MAXR, MIN_AREA)
        e.set_tracks(MIN_OVERLAP)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for j in range(P):
                e.forward_u8_tracks(xin[j].data_ptr(), j, lab[j].data_ptr(), ids[j].data_ptr(), rtab[j].data_ptr(), tmap[j].data_ptr(), ttab[j].data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        matched = 0
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            lab.fill_(0xEE); ids.fill_(-7); tmap.fill_(-7); rtab.fill_(-1); ttab.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            host = ttab.cpu().numpy()
            for j in range(P):
                want_l8, want_ids, want_table, want_map, want_tracks = eager[t0 + j]
                assert torch.equal(lab[j], want_l8[0]) and torch.equal(ids[j], want_ids[0]) and torch.equal(tmap[j], want_map[0]), (c, j)
                got = track_table(host[j], MAXR)
                assert (got.matched, got.ended, got.status) == (want_tracks.matched, want_tracks.ended, 0) and got.tobytes() == want_tracks.tobytes(), (c, j)
                matched += got.matched
        assert matched > 0
        # ---- the unfused entry on maps with long-lived tracks: eager, eager, replay (2 calls), replay (2 calls) against the oracle's six steps
        classes, maxr = (3, 7, 11), 4096
        noise = [regions_cases.noise(H, W, seed=k) for k in (0, 1)]
        want = cases.oracle([noise[k % 2] for k in range(6)], classes, 8, 1, maxr, 1)
        assert int(want[5][4]["age"].max()) == 6 and int(want[5][4]["track"].max()) > int(want[3][4]["track"].max()) > int(want[1][4]["track"].max())
        dl = [torch.from_numpy(n.copy()).cuda() for n in noise]
        ids2, tmap2 = (torch.zeros((2, H, W), dtype=torch.int32, device="cuda") for _ in range(2))
        rtab2, ttab2 = torch.zeros((2, 2 + 6 * maxr), dtype=torch.int64, device="cuda"), torch.zeros((2, 2 + 3 * maxr), dtype=torch.int64, device="cuda")
        e.set_regions(classes, 8, maxr, 1)
        e.set_tracks(1)

        def pair(s):
            for j in range(2):
                e.labels_tracks(dl[j].data_ptr(), ids2[j].data_ptr(), rtab2[j].data_ptr(), tmap2[j].data_ptr(), ttab2[j].data_ptr(), s)

        def check(step):
            torch.cuda.synchronize()
            host = ttab2.cpu().numpy()
            for j in range(2):
                cases.check_frame((ids2[j].cpu().numpy(), rtab2[j].cpu().numpy(), tmap2[j].cpu().numpy(), host[j]), want[step + j], maxr, ("unfused", step + j))

        with torch.cuda.stream(stream):
            e.tracks_reset(stream.cuda_stream)
            pair(stream.cuda_stream)
        check(0)
        graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph2, stream=stream):
            pair(torch.cuda.current_stream().cuda_stream)
        for step in (2, 4):
            ids2.fill_(-7); tmap2.fill_(-7); rtab2.fill_(-1); ttab2.fill_(-1)
            graph2.replay()
            check(step)


def test_cli_writes_the_track_columns_of_the_oracle(tmp_path):
    """Five 80x161 frames, --in_size 65x129 --u8 --regions ... --tracks 2 --regions_out DIR: one CSV per frame with the columns track,age,origin, equal as
    text to the oracle's records on the labels the library gives for the same frames; without --regions, --tracks is refused."""
    from PIL import Image
    from tdnet_amd.dataloader import cityscapesLoader
    from tdnet_amd.test import REGIONS_CLI_MAX, regions_csv
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(17)
    H, W = 65, 129
    base = rng.integers(0, 256, (80, 161, 3), dtype=np.uint8)
    for t in range(5):
        f = base.copy()
        f[:, 7 * t:7 * t + 9] = rng.integers(0, 256, (80, 9, 3), dtype=np.uint8)
        Image.fromarray(f).save(frames_dir / ("frame_%06d.png" % t))
    ld = cityscapesLoader(img_path=str(tmp_path / "data"), in_size=(H, W), as_uint8=True)
    ld.load_frames()
    m = make_model("td4")
    oracle = TrackOracle((0, 2, 5, 8, 11), 4, 3, REGIONS_CLI_MAX, 2)
    want, lines = {}, []
    with torch.no_grad():
        for t, item in enumerate(ld.data):
            l8 = m.forward_labels_u8(item[0].cuda(), pos_id=t % 4, in_size=(H, W))
            _, table, _, hdr, recs = oracle.step(np.ascontiguousarray(l8[0].cpu().numpy()))
            want[os.path.splitext(item[1])[0] + ".csv"] = regions_csv(table, recs)
            lines.append("matched / born / ended %d / %d / %d" % (int(hdr["matched"]), len(recs) - int(hdr["matched"]), int(hdr["ended"])))
    out, csvs = tmp_path / "out", tmp_path / "csv"
    out.mkdir()
    args = [sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0", "--in_size", "65x129", "--u8"]
    r = subprocess.run(args + ["--regions", "0,2,5,8,11", "--regions_conn", "4", "--regions_min_area", "3", "--tracks", "2", "--regions_out", str(csvs)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(csvs / "vid1")) == sorted(want)
    for name, text in want.items():
        assert open(csvs / "vid1" / name).read() == text, name
        assert text.startswith("id,label,area,x0,y0,x1,y1,cx,cy,track,age,origin\n") and text.count("\n") > 1
    assert [l.split("   ")[-1] for l in r.stdout.splitlines() if "matched / born / ended" in l] == lines
    r = subprocess.run(args + ["--tracks"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--regions IDS" in r.stderr
