"""Source views (include/tdnet.h "source views") on the MI355X: the operator cases of tests/test_emu_view.py on device memory (plus shapes wider
than one workgroup's strip), whole frames given as views against the same frames given as RGB bytes, the error paths, the model classes with
view= and the command line with --crop.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import view_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import PIX_NV12, PIX_RGB24, SourceView, nv12_to_rgb_u8, rgb_to_nv12, view_extent, view_to_rgb_u8
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


def test_whole_tight_rgb24_view_is_the_uint8_entry_bit_for_bit(lib):
    H, W = 33, 65
    view = SourceView(PIX_RGB24, H, W)
    s = cases.view_bytes(view)
    for rows in (1, 0):
        n = cases.stem_buffer_size(lib, H, W, rows)
        out = MEM.out((n,), np.float32, 1234.5)
        holder, addr = MEM.up(s, 1)
        assert lib.check(lib.tdnet_op_stem_image(None, addr, H, W, H, W, None, None, rows, out.data_ptr(), n, MEM.stream)) == n
        assert np.array_equal(cases.stem_image_view(lib, MEM, addr, view, H, W, rows), MEM.get(out).view(np.uint32))
    cases.run_stem_case(lib, MEM, view, [(H, W)])


@pytest.mark.parametrize("fmt", cases.PACKED, ids=[cases.NAMES[f] for f in cases.PACKED])
@pytest.mark.parametrize("name,rect,nets", cases.PACKED_CASES, ids=[c[0] for c in cases.PACKED_CASES])
def test_packed_views_match_the_rgb_route_bit_for_bit(lib, name, rect, nets, fmt):
    cases.run_stem_case(lib, MEM, cases.packed_view(fmt, rect), nets)


@pytest.mark.parametrize("layout", [0, 1], ids=["tight", "padded"])
@pytest.mark.parametrize("name,rect,net", cases.NV12_CASES, ids=[c[0] for c in cases.NV12_CASES])
def test_nv12_views_match_the_rgb_route_bit_for_bit(lib, name, rect, net, layout):
    cases.run_stem_case(lib, MEM, cases.nv12_view(rect, layout), [net], fills=(0x00, 0xFF) if layout else (0x00,))


@pytest.mark.parametrize("standard", [0, 1, 2, 3])
def test_nv12_view_all_four_standards_at_an_odd_origin(lib, standard):
    cases.run_stem_case(lib, MEM, cases.nv12_view((3, 7, 41, 83), 1, standard=standard), [(33, 65)], offsets=(1,), fills=(0x33,))


def test_wider_than_one_workgroups_strip(lib):
    """RGBA32 9 x 2200, rectangle (0, 3, 9, 2100) -> 8 x 2051, and NV12 of the same geometry at origin (1, 3)."""
    fmt, rect = cases.WIDE_PACKED
    Hf, Wf = cases.WIDE_FRAME
    cases.run_stem_case(lib, MEM, SourceView(fmt, Hf, Wf, pitch=Wf * 4 + 5, crop=rect), [cases.WIDE_NET], offsets=(0, 3))
    for layout in (0, 1):
        cases.run_stem_case(lib, MEM, cases.nv12_view(cases.WIDE_NV12, layout, frame=cases.WIDE_FRAME), [cases.WIDE_NET], offsets=(1,))


@pytest.mark.parametrize("fmt", cases.OVERLAY_PACKED, ids=[cases.NAMES[f] for f in cases.OVERLAY_PACKED])
def test_overlay_of_packed_views(lib, fmt):
    cases.run_overlay_case(lib, MEM, cases.packed_view(fmt, cases.OVERLAY_RECT))


@pytest.mark.parametrize("origin", cases.OVERLAY_NV12_ORIGINS, ids=["2_5", "3_4"])
def test_overlay_of_nv12_views(lib, origin):
    cases.run_overlay_case(lib, MEM, cases.nv12_view(origin + (41, 83), 1))


def _engine(H=33, W=65):
    spec = arch.model_spec("td2", 19, "resnet18")
    e = Engine(2, 18, 19, H, W, torch.cuda.current_device())
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


def test_frames_given_as_views_equal_frames_given_as_rgb_bytes():
    a = _engine(*cases.FRAME_NET)
    cases.run_view_scenario(a, MEM)
    a.close()


def test_errors_leave_the_configuration_and_the_fifo_alone():
    H, W = cases.FRAME_NET
    e = _engine(H, W)
    view = cases.packed_view(cases.PACKED[3], (3, 7, 41, 83))
    s = cases.view_bytes(view)
    ks, ps = MEM.up(s, 1)
    kr, pr = MEM.up(view_to_rgb_u8(s, view))
    ref = MEM.out((1, 19, H, W), np.float32, 0.0)
    e.set_input_view(view)
    e.forward_u8(ps, 0, ref.data_ptr(), MEM.stream)
    bits = MEM.get(ref).view(np.uint32).copy()
    cases.run_error_cases(e, MEM, "view", ps, bits, H, W)
    e.set_input_u8(41, 83)
    cases.run_error_cases(e, MEM, "u8", pr, bits, H, W)
    fresh = Engine(2, 18, 19, H, W, torch.cuda.current_device())
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_input_view(view)
    fresh.close()
    e.close()


def make_model():
    from tdnet_amd.model import td2_psp50
    return td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")


def test_model_methods_with_a_view_on_a_batch_of_two():
    """forward_u8(view=...) and forward_overlay_u8(view=...) on two whole BGRA frames against the pre-cropped RGB batch."""
    H, W = 33, 65
    view = cases.packed_view(cases.PACKED[3], (3, 7, 41, 83))
    frames = [cases.view_bytes(view, 0x5A, 20 + t) for t in range(2)]
    rgbs = np.stack([view_to_rgb_u8(s, view) for s in frames])
    f, g = make_model(), make_model()
    f.ensure_engine(H, W, "cuda")
    g.ensure_engine(H, W, "cuda")
    both = torch.from_numpy(np.stack(frames)).cuda()
    pre = torch.from_numpy(rgbs).cuda()
    with torch.no_grad():
        of, og = f.forward_u8(pre, pos_id=0, in_size=(H, W)), g.forward_u8(both, pos_id=0, in_size=(H, W), view=view)
        assert torch.equal(of.view(torch.int32), og.view(torch.int32)) and not torch.equal(og[0], og[1])
        pf, pg = f.forward_overlay_u8(pre, 1, (H, W), alpha=0.5), g.forward_overlay_u8(both, 1, (H, W), alpha=0.5, view=view)
        assert tuple(pg.shape) == (2, 41, 83, 3) and torch.equal(pf.flip(-1), pg)   # b g r out for a b g r source
        lf, lg = f.forward_labels_u8(pre, 0, (H, W)), g.forward_labels_u8(both, 0, (H, W), view=view)
        assert torch.equal(lf, lg)
        assert torch.equal(f.labels_overlay(lf, pre, alpha=0.5).flip(-1), g.labels_overlay(lg, both, alpha=0.5, view=view))


def test_model_classes_check_the_frame_tensor_before_an_engine_exists():
    m = make_model()
    view = cases.packed_view(cases.PACKED[3], (3, 7, 41, 83))
    n = view_extent(view)
    with pytest.raises(RuntimeError, match="uint8"):
        m.forward_u8(torch.zeros(1, n, device="cuda"), 0, (33, 65), view=view)
    with pytest.raises(RuntimeError, match="N,nbytes"):
        m.forward_overlay_u8(torch.zeros(1, 50, 365, dtype=torch.uint8, device="cuda"), 0, (33, 65), view=view)
    with pytest.raises(RuntimeError, match="below"):
        m.forward_u8(torch.zeros(1, n - 1, dtype=torch.uint8, device="cuda"), 0, (33, 65), view=view)
    assert m.engine is None


def _run_cli(data, out, flags):
    out.mkdir()
    r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(data), "--output_path", str(out), "--synthetic_seed", "0",
                        "--in_size", "33x65", "--model", "td2-psp18"] + flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


def test_cli_with_crop_writes_the_pngs_of_the_precropped_frames(tmp_path):
    """F1: random 50 x 90 PNGs.  `--u8 --crop 3,7,41,83` on F1 == `--u8` on the PNGs of F1[3:44, 7:90], byte for byte.  With `--nv12` the frame on
    the device is rgb_to_nv12(F1), so its pre-cropped counterpart is the rectangle of nv12_to_rgb_u8 of THAT surface, given as `--u8`: the same
    overlay PNGs with `--overlay 0.5`."""
    from PIL import Image
    d1, d2, d3 = (tmp_path / n / "vid1" for n in ("f1", "f2", "f3"))
    for d in (d1, d2, d3):
        d.mkdir(parents=True)
    rng = np.random.default_rng(23)
    for t in range(4):
        im = rng.integers(0, 256, (50, 90, 3), dtype=np.uint8)
        Image.fromarray(im).save(d1 / ("frame_%06d.png" % t))
        Image.fromarray(np.ascontiguousarray(im[3:44, 7:90])).save(d2 / ("frame_%06d.png" % t))
        s = rgb_to_nv12(im)
        Image.fromarray(np.ascontiguousarray(nv12_to_rgb_u8(s, 50, 90, s.shape[1], 50 * s.shape[1])[3:44, 7:90])).save(d3 / ("frame_%06d.png" % t))
    pairs = [(_run_cli(tmp_path / "f1", tmp_path / "o1", ["--u8", "--crop", "3,7,41,83"]), _run_cli(tmp_path / "f2", tmp_path / "o2", ["--u8"])),
             (_run_cli(tmp_path / "f1", tmp_path / "o3", ["--nv12", "--overlay", "0.5", "--crop", "3,7,41,83"]),
              _run_cli(tmp_path / "f3", tmp_path / "o4", ["--u8", "--overlay", "0.5"]))]
    for a, b in pairs:
        names = sorted(os.listdir(a / "vid1"))
        assert len(names) == 4
        for nm in names:
            assert (a / "vid1" / nm).read_bytes() == (b / "vid1" / nm).read_bytes(), nm
    assert Image.open(tmp_path / "o3" / "vid1" / names[0]).size == (83, 41)
