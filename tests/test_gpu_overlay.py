"""Overlay out on the MI355X: the operator and frame scenarios of tests/test_emu_overlay.py on device memory (plus rows wider than one workgroup's
strip and the real 769x1537-from-1024x2048 geometry), the model classes, a captured pos_id cycle, and the command line with --overlay.  Every
comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opcheck
import overlay_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import nv12_to_rgb_u8, overlay_u8
from tdnet_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


class DevMem:
    """The scenarios' memory: torch tensors on the device, the current stream.  fp32 inputs (the logits) sit between opcheck.GuardedTorchMem's NaN
    guard bands; byte inputs `off` bytes into holders of 0xA5, byte outputs in holders of 0xEE the scenarios check themselves."""
    def __init__(self):
        self.guarded = opcheck.GuardedTorchMem()

    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def up(self, a, off=0):
        a = np.asarray(a)
        if a.dtype == np.float32 and off == 0:
            t = self.guarded.put(np.array(a, copy=True))                 # a writable copy: the cases' arrays are read-only
            return t, t.data_ptr()
        flat = np.array(a, copy=True).view(np.uint8).reshape(-1)         # a writable copy: the cases' arrays are read-only
        holder = torch.full((flat.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        holder[off:off + flat.size] = torch.from_numpy(flat).cuda()
        return holder, holder.data_ptr() + off

    def out(self, nbytes):
        return torch.full((nbytes,), 0xEE, dtype=torch.uint8, device="cuda")

    def addr(self, buf):
        return buf.data_ptr()

    def get(self, buf):
        torch.cuda.synchronize()
        return buf.cpu().numpy()


@pytest.fixture()
def mem():
    m = DevMem()
    yield m
    m.guarded.verify()                                                   # the bands around every fp32 input still hold their fill


# ---- operator level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_kernels_equal_the_oracle_over_rgb_and_nv12_sources(lib, mem, name, C, lo, hi):
    labels = cases.run_operator_case(lib, mem, name, C, lo, hi, nv12_offs=(0, 1, 2, 3))
    if name == "c256":
        assert (labels == 255).any()


def test_nv12_layouts_standards_and_poisoned_padding(lib, mem):
    cases.run_nv12_layouts_and_standards(lib, mem)


def test_palettes_per_class_alpha_and_labels_outside_the_table(lib, mem):
    cases.run_palettes(lib, mem)


def test_every_alpha_and_source_byte_against_python_integers(lib, mem):
    cases.run_exhaustive_blend(lib, mem)


@pytest.mark.parametrize("name,lo,hi,sizes", cases.WIDE_CASES, ids=[c[0] for c in cases.WIDE_CASES])
def test_wide_rows_and_the_real_geometry(lib, mem, name, lo, hi, sizes):
    cases.run_wide_case(lib, mem, name, lo, hi, sizes)


# ---- frame level ---------------------------------------------------------------------------------------------------------------------------
def _engine(lib, model=4):
    name = {4: "td4", 2: "td2", 1: "psp"}[model]
    spec = arch.model_spec(name, 19, "resnet18")
    e = Engine(model, 18, 19, cases.H, cases.W, torch.cuda.current_device(), lib=lib, arch={})
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(cases.H), arch.feat_size(cases.W), 0))
    return e


@pytest.fixture(scope="module")
def owner(lib):
    e = _engine(lib, 4)
    yield e
    e.close()


@pytest.mark.parametrize("overlay_first", [True, False], ids=["overlay_configured_first", "input_configured_first"])
def test_overlay_frames_follow_the_input_configuration(owner, mem, overlay_first):
    cases.run_frames_follow_the_input(owner, mem, overlay_first)


def test_overlay_entries_mixed_on_one_handle(owner, mem):
    cases.run_entries_mixed(owner, mem)


def test_alpha_extremes_colour_map_equivalence_and_rejected_pixels(owner, mem):
    cases.run_alpha_extremes_and_rejection(owner, mem)


def test_single_frame_pspnet(lib, mem):
    e = _engine(lib, 1)
    cases.run_pspnet_single_frame(e, mem)
    e.close()


def test_errors_leave_the_fifo_and_a_pending_frame_alone(lib, owner, mem):
    cases.run_errors(owner, mem, lib, lambda: Engine(2, 18, 19, cases.H, cases.W, torch.cuda.current_device(), lib=lib), _capi.TdnetError)


# ---- model classes -------------------------------------------------------------------------------------------------------------------------
def make_model(name):
    from tdnet_amd.model import td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0)
    else:
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0)
    return m.eval().to("cuda")


def test_model_classes_batches_surfaces_and_the_split_frame():
    """A batch of two streams through forward_overlay_u8 / forward_overlay_nv12, then labels_overlay and encode_u8 + propagate(labels="overlay") on one
    stream: the definition on the labels a label-only model gives."""
    H, W, Hs, Ws = cases.H, cases.W, cases.HS, cases.WS
    b = make_model("td2")
    b.ensure_engine(H, W, "cuda")
    a = make_model("td2").share_weights_with(b)
    rng = np.random.default_rng(41)
    alpha = np.linspace(0.0, 1.0, 19)
    pal = a._palette_rgba(None, alpha)
    with torch.no_grad():
        for t in range(3):
            src = rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)
            if t == 1:                                                   # the same two frames as decoder surfaces
                surfs = np.stack([cases.nv12_surface(src[i], cases.PITCH, Hs * cases.PITCH, 1, 0x5A, 0xC3) for i in range(2)])
                rows = -(-surfs.shape[1] // cases.PITCH)
                padded = np.zeros((2, rows * cases.PITCH), np.uint8)
                padded[:, :surfs.shape[1]] = surfs
                src = np.stack([nv12_to_rgb_u8(surfs[i], Hs, Ws, cases.PITCH, Hs * cases.PITCH, 1) for i in range(2)])
                got = a.forward_overlay_nv12(torch.from_numpy(padded.reshape(2, rows, cases.PITCH)).cuda(), t % 2, (Hs, Ws), (H, W), alpha=alpha, standard=1)
            else:
                got = a.forward_overlay_u8(torch.from_numpy(src).cuda(), t % 2, (H, W), alpha=alpha)
            l8 = b.forward_labels_u8(torch.from_numpy(src).cuda(), pos_id=t % 2, in_size=(H, W)).cpu().numpy()
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, Hs, Ws, 3)
            for i in range(2):
                assert np.array_equal(got[i].cpu().numpy(), overlay_u8(src[i], l8[i], pal)), (t, i)
        one = make_model("td2").share_weights_with(b)
        ref = make_model("td2").share_weights_with(b)
        u = torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
        l8 = ref.forward_labels_u8(u, pos_id=0, in_size=(H, W))
        want = overlay_u8(u[0].cpu().numpy(), l8[0].cpu().numpy(), cases.pal_half())
        one.encode_u8(u, 0, in_size=(H, W))
        got = one.propagate(labels="overlay", src=u, palette=cases.pal_half())
        assert np.array_equal(got[0].cpu().numpy(), want)
        assert np.array_equal(one.labels_overlay(l8, u, alpha=128 / 255)[0].cpu().numpy(), want)


def test_a_captured_cycle_of_overlay_frames_replays_to_the_eager_pictures():
    """One pos_id cycle of forward_overlay_u8 at 65x129 captured into a hipGraph (tdnet_warmup and the configurations before the capture) and
    replayed for the following cycles: byte for byte the eager pictures."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    warm = 2 * P
    T = warm + cycles * P
    rng = np.random.default_rng(44)
    clip = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(T)]
    with torch.no_grad():
        m = make_model("td4")
        eager = [m.forward_overlay_u8(clip[t], t % P, (H, W)).clone() for t in range(T)]
        m.reset()
        for t in range(warm):                                            # steady state; the handle is configured (input and output) by these frames
            assert torch.equal(m.forward_overlay_u8(clip[t], t % P, (H, W)), eager[t])
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        m.engine.warmup(stream.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = [m.forward_overlay_u8(xin[j], j, (H, W)) for j in range(P)]
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            graph.replay()
            torch.cuda.synchronize()
            for j in range(P):
                assert torch.equal(outs[j], eager[t0 + j]), (c, j)
    assert not torch.equal(eager[-1], eager[-2]) and not torch.equal(eager[-1], clip[-1])


def test_cli_overlay_writes_the_source_size_picture(tmp_path):
    from PIL import Image
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(15)
    frames = [rng.integers(0, 256, (80, 161, 3), dtype=np.uint8) for _ in range(3)]
    for t, f in enumerate(frames):
        Image.fromarray(f).save(frames_dir / ("frame_%06d.png" % t))

    def run(extra, name):
        out = tmp_path / name
        out.mkdir()
        return out, subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out),
                                    "--synthetic_seed", "0", "--in_size", "65x129"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
    out, r = run(["--overlay", "0.5"], "none")
    assert r.returncode != 0 and "--u8 or --nv12" in r.stderr, r.stdout + r.stderr
    out, r = run(["--u8", "--overlay", "0.5"], "u8")
    assert r.returncode == 0, r.stdout + r.stderr
    m = make_model("td4")
    pal = cases.rgba(cases.palette19(), 128)
    with torch.no_grad():
        for t, f in enumerate(frames):
            l8 = m.forward_labels_u8(torch.from_numpy(f[None]).cuda(), pos_id=t % 4, in_size=(65, 129))[0].cpu().numpy()
            got = np.asarray(Image.open(out / "vid1" / ("frame_%06d.png" % t)))
            assert got.shape == (80, 161, 3) and np.array_equal(got, overlay_u8(f, l8, pal)), t
    out, r = run(["--nv12", "--overlay", "0.5", "--min_conf", "0.999"], "nv12")
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.asarray(Image.open(out / "vid1" / "frame_000000.png")).shape == (80, 161, 3)
