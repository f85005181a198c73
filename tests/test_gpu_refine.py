"""Refined matte on the MI355X: the operator tests of tests/test_emu_refine.py on device memory -- the operator entry and its coefficient launch against
the oracle dataloader.refine_matte_u8, EXACTLY, every map at a byte offset inside guard bands with padded rows -- plus one map of the real 1080 x 1920
source size, the model classes' refine_matte on strided views, and a captured graph that replays capture time's radius and eps.  The frame's end: the gather
launch over every source form, whole frames (fp32, fp16 mode, precision 2) through the refined entry and the composite entries with launch counts and error
paths (tests/refine_cases.py check_frames), a captured cycle of refined frames, the model classes on a batch of two and the split frame, the command line."""
import numpy as np
import pytest
import torch

import refine_cases as cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import refine_matte_u8
from tdnet_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


@pytest.fixture(scope="module")
def eng(lib):
    e = Engine(2, 18, 19, 33, 65, 0, lib=lib)                         # the operator needs a handle for its device, nothing else: no weights
    yield e
    e.close()


class DevMem:
    """The shared scenarios' memory (tests/refine_cases.py): torch tensors on the device, the current stream."""

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def up(self, a, off=0):
        flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        holder = torch.full((off + flat.size,), 0xA5, dtype=torch.uint8, device="cuda")   # a fresh allocation: 256-byte aligned
        holder[off:] = torch.from_numpy(np.array(flat, copy=True)).cuda()
        return holder, holder.data_ptr() + off

    def get(self, buf):
        torch.cuda.synchronize()
        return buf.cpu().numpy()


MEM = DevMem()


def test_tile_geometry(lib):
    assert cases.tile(lib) == cases.TILE


@pytest.mark.parametrize("case", cases.exact_cases(), ids=cases.case_id)
def test_operator_and_coefficients_equal_the_oracle(lib, eng, case):
    cases.check_operator(lib, eng, MEM, case, cases.FEW_OFFSETS)


def test_every_byte_offset_of_each_of_the_three_maps(lib, eng):
    cases.check_operator(lib, eng, MEM, ("random", 5, 9, 16, 65), cases.ALL_OFFSETS, fills=cases.FILLS[:1])
    cases.check_operator(lib, eng, MEM, ("ramp", 17, 29, 4, 65), cases.ALL_OFFSETS[::5], fills=cases.FILLS)


def test_the_exact_properties(lib, eng):
    tx, cy, ay = cases.TILE
    cases.check_exact_properties(eng, MEM, 5, 9)
    cases.check_exact_properties(eng, MEM, max(cy, ay) + 1, tx + 1)


def test_a_map_of_the_real_source_size(lib, eng):
    """1080 x 1920 (the 769 x 1537 network's source), r = 16: 17 x 30 tiles of the first launch, a partial last tile row, an odd output pitch"""
    case = ("ramp", 1080, 1920, 16, 65)
    G, M, out, aq, bq = cases.want(*case)
    got = cases.refine_op(eng, MEM, G, M, 16, 65, (1, 2, 3), (3, 0, 1))
    bad = got != out
    assert not bad.any(), (int(bad.sum()), tuple(int(v) for v in np.argwhere(bad)[0]))
    ga, gb = cases.coeff_op(lib, MEM, G, M, 16, 65)
    assert np.array_equal(ga, aq) and np.array_equal(gb, bq)
    assert out.min() == 0 and out.max() == 255 and len(np.unique(out)) > 100 and np.abs(aq).max() > 1024   # the case says something: slopes above 1


def test_every_refused_argument_by_message_and_nothing_written(lib, eng):
    calls, (o, keep) = cases.refused(eng, MEM)
    for call, msg in calls:
        with pytest.raises(_capi.TdnetError, match="tdnet_refine_matte.*" + msg):
            call()
    assert np.array_equal(MEM.get(o.holder), o.host)


def test_model_class_refines_batches_and_strided_views():
    from tdnet_amd.model import td4_psp18
    m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")
    with pytest.raises(RuntimeError, match="refine_matte.*no handle yet"):
        m.refine_matte(torch.zeros((5, 9), dtype=torch.uint8, device="cuda"), torch.zeros((5, 9), dtype=torch.uint8, device="cuda"), 4)
    with torch.no_grad():
        m.forward_labels(torch.zeros((1, 3, 33, 65), device="cuda"), 0)   # creates the handle
    G0, M0 = cases.inputs("ramp", 41, 83)
    G1, M1 = cases.inputs("random", 41, 83, 1)
    g, mt = torch.from_numpy(np.stack([G0, G1])).cuda(), torch.from_numpy(np.stack([M0, M1])).cuda()
    out = m.refine_matte(g, mt, 8).cpu().numpy()                      # eps = 65
    assert np.array_equal(out[0], refine_matte_u8(G0, M0, 8, 65)) and np.array_equal(out[1], refine_matte_u8(G1, M1, 8, 65))
    big = torch.full((2, 50, 100), 0xEE, dtype=torch.uint8, device="cuda")
    big[:, 3:44, 5:88] = mt
    one = m.refine_matte(g[1], big[1, 3:44, 5:88], 2, eps=4).cpu().numpy()   # a pitched view, a single map
    assert one.shape == (41, 83) and np.array_equal(one, refine_matte_u8(G1, M1, 2, 4))
    for bad, msg in (((g.float(), mt, 4), "uint8"), ((g, mt[:1], 4), "differ in shape"), ((g.cpu(), mt, 4), "CUDA")):
        with pytest.raises(RuntimeError, match="refine_matte.*" + msg):
            m.refine_matte(*bad)
    with pytest.raises(_capi.TdnetError, match="tdnet_refine_matte: radius = 17"):
        m.refine_matte(g, mt, 17)


def test_a_captured_graph_replays_the_radius_and_eps_of_capture_time(lib, eng):
    G, M, out, _, _ = cases.want("ramp", 41, 83, 16, 65025)
    g, m = cases.place(MEM, G, 1, 2), cases.place(MEM, M, 3, 0)
    o = cases.place(MEM, np.zeros((41, 83), np.uint8), 2, 1)
    ks, ps = cases.scratch(MEM, eng, 41, 83)
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        eng.refine_matte(g.addr, g.pitch, m.addr, m.pitch, o.addr, o.pitch, 41, 83, 2, 4, ps, s.cuda_stream)   # warm-up outside the capture
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            eng.refine_matte(g.addr, g.pitch, m.addr, m.pitch, o.addr, o.pitch, 41, 83, 16, 65025, ps, s.cuda_stream)
    eng.refine_matte(g.addr, g.pitch, m.addr, m.pitch, o.addr, o.pitch, 41, 83, 2, 4, ps, MEM.stream)          # other arguments since
    torch.cuda.synchronize()
    assert np.array_equal(o.pixels(MEM.get(o.holder)), refine_matte_u8(G, M, 2, 4))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(o.pixels(MEM.get(o.holder)), out)


# ---- the frame's end ---------------------------------------------------------------------------------------------------------------------------
import matte_cases as mc  # noqa: E402
from tdnet_amd import arch, weights  # noqa: E402


class Dev:
    """tests/refine_cases.py check_frames' memory: torch tensors on the device, the current stream"""

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def put(self, a):
        return torch.from_numpy(np.array(a, copy=True)).cuda()

    def ptr(self, buf):
        return buf.data_ptr()

    def get(self, buf):
        torch.cuda.synchronize()
        a = buf.cpu().numpy()
        return a.reshape(-1) if a.ndim == 1 else a


_gather = {}


def gather_inputs(lib):
    if not _gather:
        x = mc.logits("odd_w", 19, 5, 9, 6)
        keep, px = MEM.up(x)
        _, m = mc.matte_op(lib, MEM, 19, 33, 65, mc.MOVING, px, 5, 9, want_labels=False)
        m.setflags(write=False)
        _gather["v"] = (keep, px, m)
    return _gather["v"]


@pytest.mark.parametrize("kind", mc.SOURCE_KINDS)
@pytest.mark.parametrize("size", [(41, 83), (17, 29)], ids=["41x83", "17x29"])
def test_gather_planes_equal_luma_and_the_sampled_matte(lib, size, kind):
    keep, px, m = gather_inputs(lib)
    cases.check_gather(lib, MEM, kind, size, px, mc.MOVING, m)


def _owner(lib, opts=None):
    spec = arch.model_spec("td4", 19, "resnet18")
    owner = Engine(4, 18, 19, cases.H, cases.W, 0, lib=lib, opts=opts, arch={})
    owner.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(cases.H), arch.feat_size(cases.W), 0))
    return owner


@pytest.mark.parametrize("opts", [None, {"precision": 1}, {"precision": 2}], ids=["fp32", "fp16-mode", "precision-2"])
def test_whole_frames_refined_entry_composite_counts_and_errors(opts):
    owner = _owner(_capi.lib(), opts)
    rng = np.random.default_rng(45)
    frames = [rng.integers(0, 256, (cases.HS, cases.WS, 3), dtype=np.uint8) for _ in range(5)]
    cases.check_frames(Dev(), owner, frames, 4, str(opts))
    owner.close()


def test_a_captured_cycle_of_refined_frames_replays_capture_times_radius_and_eps():
    from tdnet_amd.dataloader import luma_u8, nearest_index
    owner = _owner(_capi.lib())
    a, b = owner.share(), owner.share()
    for e in (a, b):
        e.set_matte(cases.MOVING)
        e.set_input_u8(cases.HS, cases.WS)
    b.set_matte_refine(8, 4)
    P = 4
    rng = np.random.default_rng(46)
    xin = torch.from_numpy(rng.integers(0, 256, (P, cases.HS, cases.WS, 3), dtype=np.uint8)).cuda()
    outs = torch.full((P, cases.HS, cases.WS), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b.warmup(s.cuda_stream)
        for j in range(P):                                             # the FIFO fills outside the capture
            b.forward_u8_matte_refined(xin[j].data_ptr(), j, outs[j].data_ptr(), s.cuda_stream)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            for j in range(P):
                b.forward_u8_matte_refined(xin[j].data_ptr(), j, outs[j].data_ptr(), s.cuda_stream)
    b.set_matte_refine(2, 65025)                                       # after the capture: the replays do not see it
    outs.fill_(0xEE)
    graph.replay()
    torch.cuda.synchronize()
    got = outs.cpu().numpy()
    ys, xs = nearest_index(cases.H, cases.HS), nearest_index(cases.W, cases.WS)
    l8, m8 = torch.zeros((cases.H, cases.W), dtype=torch.uint8, device="cuda"), torch.zeros((cases.H, cases.W), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for rep in range(2):                                               # a's FIFO: the fill, then the cycle the graph replayed
        for j in range(P):
            a.forward_u8_matte(xin[j].data_ptr(), j, l8.data_ptr(), m8.data_ptr(), st)
            if rep == 1:
                src = xin[j].cpu().numpy()
                m = m8.cpu().numpy()
                assert np.array_equal(got[j], refine_matte_u8(luma_u8(src), m[ys][:, xs], 8, 4)), j
    for e in (a, b, owner):
        e.close()


# ---- the model classes and the command line ----------------------------------------------------------------------------------------------------
def _model():
    from tdnet_amd.model import td4_psp18
    return td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")


def test_model_classes_a_batch_of_two_and_the_split_frame():
    """forward_matte_refined_u8 and forward_composite_u8 with set_matte_refine on a batch of two (two handles), propagate(matte_refined=True) and
    propagate(composite=True) on the split frame; radius 0 gives the composite of the plain matte again."""
    from tdnet_amd.dataloader import composite_u8, luma_u8, nearest_index
    H, W, Hs, Ws = cases.H, cases.W, cases.HS, cases.WS
    ys, xs = nearest_index(H, Hs), nearest_index(W, Ws)
    a, b = _model(), _model()
    for m in (a, b):
        m.set_matte(cases.MOVING)
    with pytest.raises(RuntimeError, match="forward_matte_refined_u8.*set_matte_refine"):
        b.forward_matte_refined_u8(torch.zeros((1, Hs, Ws, 3), dtype=torch.uint8, device="cuda"), 0, (H, W))
    for bad in ((17, 65), (4, 3), (True, 65)):
        with pytest.raises(RuntimeError, match="set_matte_refine"):
            b.set_matte_refine(*bad)
    assert b.set_matte_refine(4) == (4, 65)
    rng = np.random.default_rng(47)
    with torch.no_grad():
        for t in range(3):
            u = torch.from_numpy(rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)).cuda()
            _, mm = a.forward_matte_u8(u, t % 4, (H, W))
            ref = b.forward_matte_refined_u8(u, t % 4, (H, W)).cpu().numpy()
            assert ref.shape == (2, Hs, Ws)
            for i in range(2):
                src = u[i].cpu().numpy()
                want = refine_matte_u8(luma_u8(src), mm[i].cpu().numpy()[ys][:, xs], 4, 65)
                assert np.array_equal(ref[i], want), (t, i)
        u = torch.from_numpy(rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)).cuda()
        _, mm = a.forward_matte_u8(u, 3, (H, W))
        pic = b.forward_composite_u8(u, 3, (H, W), background=cases.BG).cpu().numpy()
        for i in range(2):
            src = u[i].cpu().numpy()
            want = refine_matte_u8(luma_u8(src), mm[i].cpu().numpy()[ys][:, xs], 4, 65)
            assert np.array_equal(pic[i], composite_u8(src, want, Hs, Ws, cases.BG)), i
        b.set_matte_refine(0)
        _, mm = a.forward_matte_u8(u, 0, (H, W))
        pic = b.forward_composite_u8(u, 0, (H, W), background=cases.BG).cpu().numpy()
        for i in range(2):
            assert np.array_equal(pic[i], composite_u8(u[i].cpu().numpy(), mm[i].cpu().numpy(), H, W, cases.BG)), i
        # the split frame, one stream
        c, d = _model(), _model()
        for m in (c, d):
            m.set_matte(cases.MOVING)
        d.set_matte_refine(8, 4)
        for t in range(2):
            u1 = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
            _, mm = c.forward_matte_u8(u1, t, (H, W))
            src = u1[0].cpu().numpy()
            want = refine_matte_u8(luma_u8(src), mm[0].cpu().numpy()[ys][:, xs], 8, 4)
            d.encode_u8(u1, t, (H, W))
            if t == 0:
                got = d.propagate(matte_refined=True, src=u1).cpu().numpy()
                assert got.shape == (1, Hs, Ws) and np.array_equal(got[0], want)
            else:
                got = d.propagate(composite=True, src=u1, background=cases.BG).cpu().numpy()
                assert np.array_equal(got[0], composite_u8(src, want, Hs, Ws, cases.BG))


def test_cli_refine_writes_the_refined_matte_and_composites_through_it(tmp_path):
    """`--u8 --matte IDS --refine R,EPS` with --matte_out: the PNG at the frame's own size is the oracle's refined matte of the frame's luma and the model
    class's matte bytes; with --composite: the frame through it.  Without a byte input the flag is refused by name."""
    import os
    import subprocess
    import sys
    from PIL import Image
    from tdnet_amd.dataloader import composite_u8, luma_u8, nearest_index
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(17)
    frames = [rng.integers(0, 256, (80, 161, 3), dtype=np.uint8) for _ in range(2)]
    for t, f in enumerate(frames):
        Image.fromarray(f).save(frames_dir / ("frame_%06d.png" % t))
    ids = ",".join(str(c) for c in cases.MOVING)
    H, W = 65, 129

    def cli(name, extra):
        out = tmp_path / name
        out.mkdir()
        return out, subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0",
                                    "--in_size", "65x129"] + extra, cwd=root, capture_output=True, text=True, timeout=120)
    out, r = cli("nobytes", ["--matte", ids, "--matte_out", str(tmp_path / "m0"), "--refine", "4"])
    assert r.returncode != 0 and "--refine" in r.stdout + r.stderr and "--u8" in r.stdout + r.stderr
    out, r = cli("bad", ["--u8", "--matte", ids, "--matte_out", str(tmp_path / "m1"), "--refine", "17"])
    assert r.returncode != 0 and "--refine" in r.stdout + r.stderr
    mdir = tmp_path / "mattes"
    out, r = cli("matte", ["--u8", "--matte", ids, "--matte_out", str(mdir), "--refine", "8,4"])
    assert r.returncode == 0, r.stdout + r.stderr
    out2, r = cli("comp", ["--u8", "--matte", ids, "--composite", ",".join(str(v) for v in cases.BG), "--refine", "4"])
    assert r.returncode == 0, r.stdout + r.stderr
    m = _model()
    m.set_matte(cases.MOVING)
    ys, xs = nearest_index(H, 80), nearest_index(W, 161)
    with torch.no_grad():
        for t, f in enumerate(frames):
            _, mm = m.forward_matte_u8(torch.from_numpy(f[None]).cuda(), t % 4, (H, W))
            msrc = mm[0].cpu().numpy()[ys][:, xs]
            got = np.asarray(Image.open(mdir / "vid1" / ("frame_%06d.png" % t)))
            assert got.shape == (80, 161) and np.array_equal(got, refine_matte_u8(luma_u8(f), msrc, 8, 4)), t
            pic = np.asarray(Image.open(out2 / "vid1" / ("frame_%06d.png" % t)))
            assert np.array_equal(pic, composite_u8(f, refine_matte_u8(luma_u8(f), msrc, 4, 65), 80, 161, cases.BG)), t
