"""NV12 surfaces into the frame's first launch on the MI355X: the op-level cases of tests/test_emu_nv12.py on device memory (plus shapes wider
than one workgroup's strip), whole frames given as surfaces against the same frames given as RGB bytes, the model classes with the prefetcher,
and the command line with --nv12.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nv12_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import nv12_to_rgb_u8, rgb_to_nv12
from tdnet_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


def dev_bytes(s, off):
    """(holder, address): the bytes of s `off` bytes into a larger device buffer filled with 0xA5."""
    flat = np.array(s, copy=True).view(np.uint8).reshape(-1)           # a writable copy: the cases' arrays are read-only
    holder = torch.full((flat.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    holder[off:off + flat.size] = torch.from_numpy(flat).cuda()
    return holder, holder.data_ptr() + off


def _buffer(lib, H, W, rows):
    n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))
    return torch.full((n,), 1234.5, dtype=torch.float32, device="cuda")


def stem_image_rgb(lib, H, W, rows, img):
    out = _buffer(lib, H, W, rows)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.check(lib.tdnet_op_stem_image(img.data_ptr(), None, 0, 0, H, W, None, None, rows, out.data_ptr(), out.numel(), s)) == out.numel()
    return out.view(torch.int32)


def stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, standard, H, W, rows, mean=None, std=None):
    out = _buffer(lib, H, W, rows)
    s = torch.cuda.current_stream().cuda_stream
    got = lib.check(lib.tdnet_op_stem_image_nv12(addr, Hs, Ws, pitch, uv, standard, H, W, cases.double3(mean), cases.double3(std), rows,
                                                 out.data_ptr(), out.numel(), s))
    assert got == out.numel()
    return out.view(torch.int32)


ALL_CASES = cases.STEM_CASES + cases.WIDE_CASES


@pytest.mark.parametrize("layout", [0, 1], ids=["tight", "padded"])
@pytest.mark.parametrize("name,src_size,net_size", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_nv12_ingest_matches_the_rgb_route_bit_for_bit(lib, name, src_size, net_size, layout):
    (Hs, Ws), (H, W) = src_size, net_size
    _, pitch, uv = cases.layouts(Hs, Ws)[layout]
    want_img = torch.from_numpy(cases.expected_image(name, Hs, Ws, H, W)).cuda()
    want = {rows: stem_image_rgb(lib, H, W, rows, want_img) for rows in (1, 0)}
    for fill in ((0x00, 0xFF) if layout else (0x00,)):                 # padding and gap filled with zeros, then with ones: the same output
        s = cases.surface(name, Hs, Ws, pitch, uv, fill)
        for off in (0, 1):
            holder, addr = dev_bytes(s, off)
            for rows in (1, 0):
                got = stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, 0, H, W, rows)
                assert torch.equal(got, want[rows]), (name, rows, off, fill, int((got != want[rows]).sum()))
            h = holder.cpu().numpy()
            assert (h[:off] == 0xA5).all() and (h[off + s.size:] == 0xA5).all() and np.array_equal(h[off:off + s.size], s)


@pytest.mark.parametrize("standard", [0, 1, 2, 3])
def test_all_four_standards(lib, standard):
    name, (Hs, Ws), (H, W) = cases.STEM_CASES[5]
    _, pitch, uv = cases.layouts(Hs, Ws)[1]
    want_img = torch.from_numpy(cases.expected_image(name, Hs, Ws, H, W, standard)).cuda()
    holder, addr = dev_bytes(cases.surface(name, Hs, Ws, pitch, uv, 0x33), 1)
    for rows in (1, 0):
        assert torch.equal(stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, standard, H, W, rows), stem_image_rgb(lib, H, W, rows, want_img))


def test_other_mean_and_std(lib):
    name, (Hs, Ws), (H, W) = cases.STEM_CASES[5]
    _, pitch, uv = cases.layouts(Hs, Ws)[0]
    want_img = torch.from_numpy(cases.expected_image(name, Hs, Ws, H, W, 0, cases.ALT_MEAN, cases.ALT_STD)).cuda()
    holder, addr = dev_bytes(cases.surface(name, Hs, Ws, pitch, uv), 3)
    for rows in (1, 0):
        assert torch.equal(stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, 0, H, W, rows, cases.ALT_MEAN, cases.ALT_STD),
                           stem_image_rgb(lib, H, W, rows, want_img))


class DevMem:
    """run_frame_scenario's memory: torch tensors on the device, the default stream."""

    def up(self, a, off=0):
        return dev_bytes(a, off)

    def out(self, shape, dtype, fill):
        return torch.full(shape, fill, dtype={np.float32: torch.float32, np.uint8: torch.uint8}[dtype], device="cuda")

    def addr(self, buf):
        return buf.data_ptr()

    def get(self, buf):
        return buf.cpu().numpy()


def test_frames_given_as_surfaces_equal_frames_given_as_rgb_bytes():
    H, W = cases.FRAME_NET
    spec = arch.model_spec("td2", 19, "resnet18")
    a = Engine(2, 18, 19, H, W, torch.cuda.current_device())
    a.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    cases.run_frame_scenario(a, DevMem())
    a.close()


def make_model(name):
    from tdnet_amd.model import td2_psp50, td4_psp18
    if name == "td4":
        return td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")
    return td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval().to("cuda")


def test_model_methods_batches_and_the_prefetcher():
    """td4-psp18 at 33x65: forward_nv12 / forward_labels_nv12 / encode_nv12 of loader-style items against forward_u8 of the oracle's bytes; a
    batch of two surfaces; items travel through DevicePrefetcher with their fifth element."""
    from tdnet_amd.dataloader import DevicePrefetcher
    H, W, Hs, Ws, T = 33, 65, 41, 83, 5
    a = make_model("td4")
    a.ensure_engine(H, W, "cuda")
    b, c = make_model("td4").share_weights_with(a), make_model("td4").share_weights_with(a)
    rng = np.random.default_rng(21)
    surfs = [rgb_to_nv12(rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)) for _ in range(T)]
    pitch = surfs[0].shape[1]
    rgbs = [nv12_to_rgb_u8(s, Hs, Ws, pitch, Hs * pitch) for s in surfs]
    items = [[torch.from_numpy(s[None]).pin_memory(), "f%d.png" % t, "vid", (W, H), (Hs, Ws)] for t, s in enumerate(surfs)]
    with torch.no_grad():
        for t, (surf, name, folder, size, src_size) in enumerate(DevicePrefetcher(items, "cuda")):
            assert surf.dtype == torch.uint8 and surf.is_cuda and tuple(surf.shape) == (1, Hs + 21, pitch) and src_size == (Hs, Ws)
            u = torch.from_numpy(rgbs[t][None]).cuda()
            oa, ob = a.forward_u8(u, pos_id=t % 4, in_size=(H, W)), b.forward_nv12(surf, t % 4, src_size, (H, W))
            assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), t
            assert a.engine.last_launch_count() == b.engine.last_launch_count() > 0
            assert torch.equal(c.forward_labels_nv12(surf, t % 4, src_size, (H, W)), a.argmax_u8(oa)), t
        # the split frame
        want = a.forward_labels_u8(torch.from_numpy(rgbs[0][None]).cuda(), pos_id=1, in_size=(H, W))
        c.encode_nv12(torch.from_numpy(surfs[0][None]).cuda(), 1, (Hs, Ws), (H, W))
        assert torch.equal(c.propagate(labels="u8"), want)
        assert torch.equal(b.forward_labels_nv12(torch.from_numpy(surfs[0][None]).cuda(), 1, (Hs, Ws), (H, W)), want)   # A and B in step again
        # the other output forms: picture, score, confidence
        u0, s0 = torch.from_numpy(rgbs[1][None]).cuda(), torch.from_numpy(surfs[1][None]).cuda()
        assert torch.equal(a.forward_rgb_u8(u0, 2, (H, W), (8, 16)), b.forward_rgb_nv12(s0, 2, (Hs, Ws), (H, W), (8, 16)))
        gt = torch.from_numpy(rng.integers(0, 19, (1, H, W), dtype=np.uint8)).cuda()
        assert torch.equal(a.forward_score_u8(u0, gt, 3, (H, W), return_labels=True), b.forward_score_nv12(s0, gt, 3, (Hs, Ws), (H, W), return_labels=True))
        assert np.array_equal(a.confusion_matrix(), b.confusion_matrix()) and a.confusion_matrix().sum() == H * W
        (la, ca), (lb, cb) = a.forward_labels_conf_u8(u0, 0, (H, W)), b.forward_labels_conf_nv12(s0, 0, (Hs, Ws), (H, W))
        assert torch.equal(la, lb) and torch.equal(ca, cb)
        # a batch of two surfaces (two handles, two lanes)
        both = torch.from_numpy(np.stack(surfs[:2])).cuda()
        f, g = make_model("td2"), make_model("td2")
        f.ensure_engine(H, W, "cuda")
        g.ensure_engine(H, W, "cuda")
        of = f.forward_u8(torch.from_numpy(np.stack(rgbs[:2])).cuda(), pos_id=0, in_size=(H, W))
        og = g.forward_nv12(both, 0, (Hs, Ws), (H, W))
        assert torch.equal(of.view(torch.int32), og.view(torch.int32)) and not torch.equal(og[0], og[1])


@pytest.mark.parametrize("extra", [[], ["--prefetch"]], ids=["frame_by_frame", "prefetch"])
def test_cli_with_nv12_writes_the_pngs_of_u8_on_the_converted_frames(tmp_path, extra):
    """Frames F1: random PNGs; F2: the PNGs of nv12_to_rgb_u8(rgb_to_nv12(F1)).  `--nv12` on F1 == `--u8` on F2, byte for byte."""
    from PIL import Image
    d1, d2 = tmp_path / "f1" / "vid1", tmp_path / "f2" / "vid1"
    d1.mkdir(parents=True)
    d2.mkdir(parents=True)
    rng = np.random.default_rng(22)
    for t in range(6):
        im = rng.integers(0, 256, (41, 83, 3), dtype=np.uint8)
        Image.fromarray(im).save(d1 / ("frame_%06d.png" % t))
        s = rgb_to_nv12(im)
        Image.fromarray(nv12_to_rgb_u8(s, 41, 83, s.shape[1], 41 * s.shape[1])).save(d2 / ("frame_%06d.png" % t))
    outs = []
    for data, flag in ((tmp_path / "f1", "--nv12"), (tmp_path / "f2", "--u8")):
        out = tmp_path / ("out" + flag.replace("--", "_"))
        out.mkdir()
        r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(data), "--output_path", str(out), "--synthetic_seed", "0",
                            "--in_size", "33x65", flag] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(out)
    names = sorted(os.listdir(outs[0] / "vid1"))
    assert len(names) == 6
    for nm in names:
        assert (outs[0] / "vid1" / nm).read_bytes() == (outs[1] / "vid1" / nm).read_bytes(), nm
