"""Surfaces (include/tdnet.h "surfaces") on the MI355X: the operator cases of tests/test_emu_surface.py on device memory (plus shapes wider than one
workgroup's strip, one per sample width), whole frames given as surfaces against the same frames given as RGB bytes for every layout, pictures into
destination surfaces against a twin handle, the error paths, a captured pos_id cycle, the model classes with surface= / out_surface= and the command
line with --yuv / --out_yuv.  Every comparison is exact; the guard holders turn an out-of-range write into a failed comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surface_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import (SURF_DST, SURF_I420, SURF_NV12, SURF_P010, Surface, pack_surface, surface_extent, surface_to_rgb_u8, write_surface)
from tdnet_amd.engine import Engine
from tdnet_amd.test import yuv_surface

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH = {np.float32: torch.float32, np.uint8: torch.uint8, np.int32: torch.int32}
IDS = [cases.NAMES[l] for l in cases.LAYOUTS]
LAYOUT_VARIANTS = [(l, v) for l in cases.LAYOUTS for v in cases.variants(l)]
LV_IDS = ["%s_%s" % (cases.NAMES[l], v) for l, v in LAYOUT_VARIANTS]


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


@pytest.mark.parametrize("layout,variant", LAYOUT_VARIANTS, ids=LV_IDS)
def test_surfaces_match_the_rgb_route_bit_for_bit(lib, layout, variant):
    for name, rect, net in cases.RECTS:
        cases.run_stem_case(lib, MEM, cases.surface(layout, rect, variant), net, fills=(0x00, 0xFF) if variant != "tight" or name == "phase_3_7" else (0x00,))


@pytest.mark.parametrize("layout", cases.LAYOUTS, ids=IDS)
def test_all_four_standards_at_an_odd_origin(lib, layout):
    for standard in range(4):
        cases.run_stem_case(lib, MEM, cases.surface(layout, (3, 7, 41, 83), "padded", standard=standard), (33, 65), offsets=(1,), fills=(0x33,))


@pytest.mark.parametrize("layout", cases.WIDE_LAYOUTS, ids=[cases.NAMES[l] for l in cases.WIDE_LAYOUTS])
def test_wider_than_one_workgroups_strip(lib, layout):
    """I420 and P010 9 x 2200, rectangle (1, 3, 8, 2100) -> 8 x 2051: more than one strip of 256 lanes x 4 columns per row."""
    for variant in ("tight", "padded"):
        cases.run_stem_case(lib, MEM, cases.surface(layout, cases.WIDE_RECT, variant, frame=cases.WIDE_FRAME), cases.WIDE_NET, offsets=(1,))


def test_a_p010_destination_wider_than_one_workgroup(lib):
    """The colour map and the overlay over an I420 source into a P010 rectangle of 8 x 2100 (525 lane blocks a row: three workgroups)."""
    layout, size = cases.WIDE_DST
    dsurf = cases.surface(layout, (0, 2) + size, "padded", frame=(9, 2104), standard=1)
    pal4 = cases.dvc.palette(12)
    pal3 = np.ascontiguousarray(pal4[:, :3])
    l8 = cases.vc.overlay_labels()
    x, lab = cases.dvc.fused_labels(lib, MEM, 19)
    desc, sbytes, rgb = cases.overlay_source("i420", size)
    for name, how, labels in (("labels", dict(labels_u8=l8), l8), ("fused", dict(x=x), lab)):
        cases.check_picture(lib, MEM, dsurf, cases.dvc.colour_map(labels, pal3, size), pal3, size=size, offsets=(0, 1), what=name + " colour map", **how)
        cases.check_picture(lib, MEM, dsurf, cases.overlay_u8(rgb, labels, pal4), pal4, src=(desc, sbytes), offsets=(3,), what=name + " overlay", **how)


@pytest.mark.parametrize("layout", cases.LAYOUTS, ids=IDS)
def test_overlay_over_surfaces(lib, layout):
    for rect in cases.OVERLAY_RECTS:
        cases.run_overlay_case(lib, MEM, cases.surface(layout, rect, "v_first" if layout == SURF_I420 else "padded", standard=1))


@pytest.mark.parametrize("layout,variant", [(l, v) for l in SURF_DST for v in cases.variants(l)], ids=["%s_%s" % (cases.NAMES[l], v) for l in SURF_DST for v in cases.variants(l)])
def test_pictures_into_surfaces(lib, layout, variant):
    for case in cases.DST_CASES:
        cases.run_dest_case(lib, MEM, layout, variant, case, standard=1 if variant == "padded" else 2, offsets=(0, 1, 2, 3) if variant == "padded" else (1,))


def test_pictures_into_surfaces_other_standards_and_views_behind_surface_sources(lib):
    for standard in (0, 3):
        for layout in (SURF_I420, SURF_P010):
            cases.run_dest_case(lib, MEM, layout, "padded", "corner_odd", standard=standard, sources=("nv12_view", "uyvy", "rgb24_whole"), offsets=(3,))
    cases.run_view_dest_behind_surface_source(lib, MEM)


def _engine(H=33, W=65):
    spec = arch.model_spec("td2", 19, "resnet18")
    e = Engine(2, 18, 19, H, W, torch.cuda.current_device())
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


@pytest.fixture(scope="module")
def engine():
    e = _engine(*cases.NET)
    yield e
    e.close()


@pytest.mark.parametrize("layout", cases.LAYOUTS, ids=IDS)
def test_frames_given_as_surfaces_equal_frames_given_as_rgb_bytes(engine, layout):
    cases.run_surface_scenario(engine, MEM, layouts=(layout,))


def test_frames_into_destination_surfaces_equal_write_surface_of_the_twins_pictures(engine):
    cases.run_output_scenario(engine, MEM)


def test_errors_leave_the_configuration_the_fifo_and_a_pending_frame_alone():
    H, W = cases.NET
    e = _engine(H, W)
    surf = cases.surface(SURF_I420, cases.SCENARIO_RECT, "padded")
    s = cases.surface_bytes(surf)
    ks, ps = MEM.up(s, 1)
    kr, pr = MEM.up(surface_to_rgb_u8(s, surf))
    ref = MEM.out((1, 19, H, W), np.float32, 0.0)
    e.set_input_surface(surf)
    e.forward_u8(ps, 0, ref.data_ptr(), MEM.stream)
    bits = MEM.get(ref).view(np.uint32).copy()
    cases.run_error_cases(e, MEM, "surface", ps, bits, H, W)
    e.set_input_u8(41, 83)
    cases.run_error_cases(e, MEM, "u8", pr, bits, H, W)
    e.set_input_surface(surf)
    e.set_output_overlay(cases.vc.overlay_palette())
    dsurf = cases.surface(SURF_P010, (2, 6, 41, 83), "padded", frame=cases.DST_FRAME, standard=1)
    e.set_output_surface(dsurf)
    cases.run_output_error_cases(e, MEM, ps, dsurf, H, W)
    fresh = Engine(2, 18, 19, H, W, torch.cuda.current_device())
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_input_surface(surf)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_output_surface(dsurf)
    fresh.close()
    e.close()


def make_model():
    from tdnet_amd.model import td2_psp50
    return td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")


def test_a_captured_cycle_from_p010_into_i420_replays_to_the_eager_bytes():
    """One pos_id cycle of forward_overlay_u8(surface=P010, out_surface=I420) at 33x65 captured into a hipGraph (tdnet_warmup and the configurations
    before the capture) and replayed for the following cycles into the same destination tensors: byte for byte the eager frames, which are
    write_surface of the contiguous overlays a twin model gives on the oracle's RGB bytes."""
    H, W, P, cycles = 33, 65, 2, 2
    warm = 2 * P
    T = warm + cycles * P
    src = cases.surface(SURF_P010, cases.SCENARIO_RECT, "padded", standard=1)
    h, w = src.size
    dsurf = cases.surface(SURF_I420, (2, 6, h, w), "padded", frame=cases.DST_FRAME, standard=1)
    n = surface_extent(dsurf)
    host = [cases.surface_bytes(src, 0x5A, 50 + t) for t in range(T)]
    clip = [torch.from_numpy(b.copy())[None].cuda() for b in host]
    with torch.no_grad():
        m, twin = make_model(), make_model()
        eager = [m.forward_overlay_u8(clip[t], t % P, (H, W), surface=src, out_surface=dsurf).clone() for t in range(T)]
        for t in range(T):
            rgb = torch.from_numpy(surface_to_rgb_u8(host[t], src))[None].cuda()
            pic = twin.forward_overlay_u8(rgb, t % P, (H, W))[0].cpu().numpy()
            assert tuple(eager[t].shape) == (1, n) and np.array_equal(eager[t][0].cpu().numpy(), write_surface(np.zeros(n, np.uint8), dsurf, pic)), t
        m.reset()
        for t in range(warm):                                            # steady state; the handle is configured (input, output, destination) by these frames
            assert torch.equal(m.forward_overlay_u8(clip[t], t % P, (H, W), surface=src, out_surface=dsurf), eager[t])
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, clip[0].shape[1]), dtype=torch.uint8, device="cuda")
        outs = [torch.zeros((1, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
        m.engine.warmup(stream.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            for j in range(P):
                m.forward_overlay_u8(xin[j], j, (H, W), surface=src, out_surface=dsurf, out=outs[j])
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            graph.replay()
            torch.cuda.synchronize()
            for j in range(P):
                assert torch.equal(outs[j], eager[t0 + j]), (c, j)
    assert not torch.equal(eager[-1], eager[-2])


def test_model_methods_with_surface_and_out_surface_on_a_batch_of_two():
    """Two whole P010 frames read as surfaces, the pictures written into caller-supplied NV21 frames: each sample is write_surface of what the oracle's
    RGB batch gives without a destination, and the bytes around the rectangle's samples are the caller's.  Giving both of a pair is an error."""
    H, W = cases.NET
    src = cases.surface(SURF_P010, cases.SCENARIO_RECT, "padded", standard=1)
    h, w = src.size
    frames = [cases.surface_bytes(src, 0x5A, 20 + t) for t in range(2)]
    rgbs = np.stack([surface_to_rgb_u8(s, src) for s in frames])
    f, g = make_model(), make_model()
    both, pre = torch.from_numpy(np.stack(frames)).cuda(), torch.from_numpy(rgbs).cuda()
    pal3 = cases.dvc.PAL3
    dsurf = cases.surface(cases.SURF_NV21, (2, 6, h, w), "padded", frame=cases.DST_FRAME, standard=1)
    n = surface_extent(dsurf)

    def check(got, pictures, prefill):
        assert tuple(got.shape) == (2, n)
        for i in range(2):
            assert np.array_equal(got[i].cpu().numpy(), write_surface(prefill, dsurf, pictures[i].cpu().numpy())), i

    with torch.no_grad():
        of, og = f.forward_u8(pre, pos_id=0, in_size=(H, W)), g.forward_u8(both, pos_id=0, in_size=(H, W), surface=src)
        assert torch.equal(of.view(torch.int32), og.view(torch.int32)) and not torch.equal(og[0], og[1])
        mine = torch.full((2, n + 7), 0xA5, dtype=torch.uint8, device="cuda")[:, :n].contiguous()
        got = g.forward_overlay_u8(both, 1, (H, W), alpha=0.5, surface=src, out_surface=dsurf, out=mine)
        assert got is mine
        check(got, f.forward_overlay_u8(pre, 1, (H, W), alpha=0.5), np.full(n, 0xA5, np.uint8))
        check(g.forward_rgb_u8(both, 0, (H, W), (h, w), pal3, surface=src, out_surface=dsurf), f.forward_rgb_u8(pre, 0, (H, W), (h, w), pal3), np.zeros(n, np.uint8))
        lf, lg = f.forward_labels_u8(pre, 1, (H, W)), g.forward_labels_u8(both, 1, (H, W), surface=src)
        assert torch.equal(lf, lg)
        check(g.labels_overlay(lg, both, alpha=0.5, surface=src, out_surface=dsurf), f.labels_overlay(lf, pre, alpha=0.5), np.zeros(n, np.uint8))
        check(g.labels_rgb(lg, (h, w), pal3, out_surface=dsurf), f.labels_rgb(lf, (h, w), pal3), np.zeros(n, np.uint8))
        assert torch.equal(g.forward_overlay_u8(both, 0, (H, W), alpha=0.5, surface=src), f.forward_overlay_u8(pre, 0, (H, W), alpha=0.5))   # contiguous again, r g b
        with pytest.raises(RuntimeError, match="not both"):
            g.forward_u8(both, 0, (H, W), surface=src, view=cases.vc.packed_view(cases.vc.PACKED[3], (3, 7, 41, 83)))
        with pytest.raises(RuntimeError, match="not both"):
            g.labels_rgb(lg, (h, w), pal3, out_surface=dsurf, out_view=cases.dvc.FRAME_DESTS[0])
        with pytest.raises(RuntimeError, match="below"):
            g.forward_u8(both[:, :surface_extent(src) - 1].contiguous(), 0, (H, W), surface=src)
        with pytest.raises(RuntimeError, match="destination"):
            g.labels_rgb(lg, (h, w), pal3, out_surface=cases.surface(cases.SURF_YUY2, (2, 6, h, w), "tight", frame=cases.DST_FRAME))


def _run_cli(data, out, flags):
    out.mkdir()
    r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(data), "--output_path", str(out), "--synthetic_seed", "0",
                        "--in_size", "33x65", "--model", "td2-psp18"] + flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_cli_yuv_with_crop_and_out_yuv(tmp_path):
    """F1: random 50 x 90 PNGs.  `--yuv i420 --crop 3,7,41,83` on F1 == `--u8` on the PNGs of the oracle's pre-cropped frames (the rectangle of
    surface_to_rgb_u8 of the surface the run packs), byte for byte.  `--yuv i420 --overlay 0.5 --out_yuv p010:FILE`: the raw file is the concatenation of
    write_surface of the overlay PNGs the same run wrote."""
    from PIL import Image
    d1, d2 = (tmp_path / n / "vid1" for n in ("f1", "f2"))
    for d in (d1, d2):
        d.mkdir(parents=True)
    rng = np.random.default_rng(31)
    for t in range(4):
        im = rng.integers(0, 256, (50, 90, 3), dtype=np.uint8)
        Image.fromarray(im).save(d1 / ("frame_%06d.png" % t))
        whole = yuv_surface(SURF_I420, 50, 90, 0)
        Image.fromarray(np.ascontiguousarray(surface_to_rgb_u8(pack_surface(im, whole), whole)[3:44, 7:90])).save(d2 / ("frame_%06d.png" % t))
    a = _run_cli(tmp_path / "f1", tmp_path / "o1", ["--yuv", "i420", "--crop", "3,7,41,83"])
    b = _run_cli(tmp_path / "f2", tmp_path / "o2", ["--u8"])
    names = sorted(os.listdir(a / "vid1"))
    assert len(names) == 4
    for nm in names:
        assert (a / "vid1" / nm).read_bytes() == (b / "vid1" / nm).read_bytes(), nm
    raw = tmp_path / "f.p010"
    c = _run_cli(tmp_path / "f1", tmp_path / "o3", ["--yuv", "i420", "--overlay", "0.5", "--out_yuv", "p010:" + str(raw)])
    want = b""
    dst = yuv_surface(SURF_P010, 50, 90, 0)
    for nm in names:
        want += write_surface(np.zeros(surface_extent(dst), np.uint8), dst, np.asarray(Image.open(c / "vid1" / nm).convert("RGB"))).tobytes()
    assert raw.read_bytes() == want and len(want) == 4 * 2 * (50 + 25) * 90
