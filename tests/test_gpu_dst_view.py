"""Destination views (include/tdnet.h "destination views") on the MI355X: the operator cases of tests/test_emu_dst_view.py on device memory, whole
frames with a destination view against a twin handle without one, the error paths, a captured pos_id cycle, the model classes with out_view= and the
command line with --out_nv12.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dst_view_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import PIX_NV12, nv12_from_rgb_u8, view_extent, view_to_rgb_u8, write_view
from tdnet_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


class DevMem:
    """The scenarios' memory: torch tensors on the device, the current stream."""

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def up(self, a, off=0):
        flat = np.array(a, copy=True).view(np.uint8).reshape(-1)       # a writable copy: the cases' arrays are read-only
        holder = torch.full((flat.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        holder[off:off + flat.size] = torch.from_numpy(flat).cuda()
        return holder, holder.data_ptr() + off

    def out(self, shape, dtype, fill):
        return torch.full(tuple(shape), fill, dtype=TORCH[dtype], device="cuda")

    def addr(self, buf):
        return buf.data_ptr()

    def get(self, buf):
        return buf.cpu().numpy()


MEM = DevMem()


@pytest.mark.parametrize("tag,fmt,layout,standard", cases.DESTS, ids=cases.DEST_IDS)
def test_pictures_into_every_destination_form(lib, tag, fmt, layout, standard):
    cases.run_dest_case(lib, MEM, fmt, layout, standard)


@pytest.mark.parametrize("frame,rect", cases.EDGES, ids=cases.EDGE_IDS)
def test_edge_rectangles(lib, frame, rect):
    cases.run_edge_case(lib, MEM, frame, rect)


def _engine(H=33, W=65):
    spec = arch.model_spec("td2", 19, "resnet18")
    e = Engine(2, 18, 19, H, W, torch.cuda.current_device())
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


def test_frames_with_a_destination_view_equal_write_view_of_the_twins_pictures():
    a = _engine(*cases.NET)
    cases.run_frame_scenario(a, MEM)
    a.close()


def test_errors_leave_the_configuration_the_fifo_and_a_pending_frame_alone():
    H, W = cases.NET
    e = _engine(H, W)
    e.set_input_view(cases.SRC_VIEW)
    e.set_output_overlay(cases.vc.overlay_palette())
    e.set_output_rgb(41, 83, cases.PAL3)
    e.set_output_view(cases.FRAME_DESTS[0])
    holder, ptr = MEM.up(cases.vc.view_bytes(cases.SRC_VIEW, 0x5A, 3), 1)
    cases.run_error_cases(e, MEM, ptr, H, W)
    e.close()


def make_model():
    from tdnet_amd.model import td2_psp50
    return td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")


def test_a_captured_cycle_with_a_destination_view_replays_to_the_eager_bytes():
    """One pos_id cycle of forward_overlay_u8(out_view=NV12) at 33x65 captured into a hipGraph (tdnet_warmup and the configurations before the
    capture) and replayed for the following cycles into the same destination tensors: byte for byte the eager frames, which are write_view of the
    contiguous overlays of a twin model."""
    H, W, Hs, Ws, P, cycles = 33, 65, 41, 83, 2, 2
    warm = 2 * P
    T = warm + cycles * P
    rng = np.random.default_rng(45)
    clip = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(T)]
    dview = cases.dest_view(PIX_NV12, 1, 1)
    n = view_extent(dview)
    with torch.no_grad():
        m, twin = make_model(), make_model()
        eager = [m.forward_overlay_u8(clip[t], t % P, (H, W), out_view=dview).clone() for t in range(T)]
        for t in range(T):
            pic = twin.forward_overlay_u8(clip[t], t % P, (H, W))[0].cpu().numpy()
            assert tuple(eager[t].shape) == (1, n) and np.array_equal(eager[t][0].cpu().numpy(), write_view(np.zeros(n, np.uint8), dview, pic)), t
        m.reset()
        for t in range(warm):                                            # steady state; the handle is configured (input, output and view) by these frames
            assert torch.equal(m.forward_overlay_u8(clip[t], t % P, (H, W), out_view=dview), eager[t])
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        outs = [torch.zeros((1, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
        m.engine.warmup(stream.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for j in range(P):
                m.forward_overlay_u8(xin[j], j, (H, W), out_view=dview, out=outs[j])
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            graph.replay()
            torch.cuda.synchronize()
            for j in range(P):
                assert torch.equal(outs[j], eager[t0 + j]), (c, j)
    assert not torch.equal(eager[-1], eager[-2])


def test_model_methods_with_out_view_on_a_batch_of_two():
    """Two whole BGRA frames read through a source view, the pictures written into caller-supplied destination frames: each sample is write_view of
    what the pre-cropped RGB batch gives without a destination view, and the bytes around the rectangle are the caller's."""
    H, W = cases.NET
    view = cases.SRC_VIEW
    frames = [cases.vc.view_bytes(view, 0x5A, 20 + t) for t in range(2)]
    rgbs = np.stack([view_to_rgb_u8(s, view) for s in frames])
    f, g = make_model(), make_model()
    both, pre = torch.from_numpy(np.stack(frames)).cuda(), torch.from_numpy(rgbs).cuda()
    pal3 = cases.PAL3

    def check(got, dview, pictures, prefill):
        assert tuple(got.shape) == (2, view_extent(dview))
        for i in range(2):
            assert np.array_equal(got[i].cpu().numpy(), write_view(prefill, dview, pictures[i].cpu().numpy())), (dview, i)

    with torch.no_grad():
        for dview in cases.FRAME_DESTS:
            n = view_extent(dview)
            mine = torch.full((2, n + 7), 0xA5, dtype=torch.uint8, device="cuda")[:, :n].contiguous()
            got = g.forward_overlay_u8(both, 0, (H, W), alpha=0.5, view=view, out_view=dview, out=mine)
            assert got is mine
            check(got, dview, f.forward_overlay_u8(pre, 0, (H, W), alpha=0.5), np.full(n, 0xA5, np.uint8))
            check(g.forward_rgb_u8(both, 1, (H, W), (41, 83), pal3, view=view, out_view=dview), dview, f.forward_rgb_u8(pre, 1, (H, W), (41, 83), pal3), np.zeros(n, np.uint8))
            lf, lg = f.forward_labels_u8(pre, 0, (H, W)), g.forward_labels_u8(both, 0, (H, W), view=view)
            assert torch.equal(lf, lg)
            check(g.labels_overlay(lg, both, alpha=0.5, view=view, out_view=dview), dview, f.labels_overlay(lf, pre, alpha=0.5), np.zeros(n, np.uint8))
            check(g.labels_rgb(lg, (41, 83), pal3, out_view=dview), dview, f.labels_rgb(lf, (41, 83), pal3), np.zeros(n, np.uint8))
            x = torch.from_numpy(np.concatenate([cases.vc.expected_image(view, H, W, 20 + t) for t in range(2)])).cuda()
            check(g.forward_rgb(x, 1, (41, 83), pal3, out_view=dview), dview, f.forward_rgb(x, 1, (41, 83), pal3), np.zeros(n, np.uint8))
            # a method without out_view on the same engines is contiguous again
            assert torch.equal(g.forward_overlay_u8(both, 0, (H, W), alpha=0.5, view=view).flip(-1), f.forward_overlay_u8(pre, 0, (H, W), alpha=0.5))


def test_cli_out_nv12_is_the_integer_oracle_of_the_pngs_the_same_run_writes(tmp_path):
    """Four random 50 x 90 PNGs through `--nv12 --overlay 0.5 --out_nv12 f.yuv`: the raw file is the concatenation of nv12_from_rgb_u8 of the overlay
    PNGs the run wrote, and those PNGs are the ones the run writes without --out_nv12."""
    from PIL import Image
    d = tmp_path / "data" / "vid1"
    d.mkdir(parents=True)
    rng = np.random.default_rng(29)
    for t in range(4):
        Image.fromarray(rng.integers(0, 256, (50, 90, 3), dtype=np.uint8)).save(d / ("frame_%06d.png" % t))

    def run(name, flags):
        out = tmp_path / name
        out.mkdir()
        r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out), "--synthetic_seed", "0",
                            "--in_size", "33x65", "--model", "td2-psp18"] + flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return out

    raw = tmp_path / "f.yuv"
    a = run("a", ["--nv12", "--overlay", "0.5", "--out_nv12", str(raw)])
    b = run("b", ["--nv12", "--overlay", "0.5"])
    names = sorted(os.listdir(a / "vid1"))
    assert len(names) == 4
    want = b""
    for nm in names:
        assert (a / "vid1" / nm).read_bytes() == (b / "vid1" / nm).read_bytes(), nm
        want += nv12_from_rgb_u8(np.asarray(Image.open(a / "vid1" / nm).convert("RGB"))).tobytes()
    assert raw.read_bytes() == want and len(want) == 4 * (50 + 25) * 90
