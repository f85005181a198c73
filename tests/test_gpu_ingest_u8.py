"""uint8 frames in, uint8 labels out on the MI355X: the op-level cases of tests/test_emu_ingest_u8.py on device memory (plus shapes wider than
one workgroup's strip), whole frames given as bytes against the same frames given as the loader's fp32 tensors, the uint8 prefetch / download
loop, and the command line with --u8.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ingest_u8_cases as cases
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


def dev_bytes(src, off):
    """(holder, address): src's bytes `off` bytes into a larger device buffer filled with 0xA5."""
    holder = torch.full((src.size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    holder[off:off + src.size] = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).cuda()
    return holder, holder.data_ptr() + off


def stem_image(lib, H, W, rows, img=None, src_addr=None, src_size=(0, 0), mean=None, std=None):
    n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))
    out = torch.full((n,), 1234.5, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    got = lib.check(lib.tdnet_op_stem_image(None if img is None else img.data_ptr(), src_addr, src_size[0], src_size[1], H, W,
                                            cases.double3(mean), cases.double3(std), rows, out.data_ptr(), n, s))
    assert got == n
    return out.view(torch.int32)


@pytest.mark.parametrize("name,src_size,net_size", cases.STEM_CASES + cases.WIDE_CASES, ids=[c[0] for c in cases.STEM_CASES + cases.WIDE_CASES])
def test_ingest_matches_the_host_loader_bit_for_bit(lib, name, src_size, net_size):
    (Hs, Ws), (H, W) = src_size, net_size
    src = cases.source(name, Hs, Ws)
    want_img = torch.from_numpy(cases.expected_image(src, H, W)).cuda()
    want = [stem_image(lib, H, W, rows, img=want_img) for rows in (1, 0)]
    for off in (0, 1):
        holder, addr = dev_bytes(src, off)
        for rows in (1, 0):
            got = stem_image(lib, H, W, rows, src_addr=addr, src_size=(Hs, Ws))
            assert torch.equal(got, want[1 - rows]), (name, rows, off, int((got != want[1 - rows]).sum()))


def test_ingest_with_other_mean_and_std(lib):
    (Hs, Ws), (H, W) = (41, 83), (33, 65)
    src = cases.source("down_41x83", Hs, Ws)
    want_img = torch.from_numpy(cases.expected_image(src, H, W, cases.ALT_MEAN, cases.ALT_STD)).cuda()
    holder, addr = dev_bytes(src, 3)
    for rows in (1, 0):
        assert torch.equal(stem_image(lib, H, W, rows, src_addr=addr, src_size=(Hs, Ws), mean=cases.ALT_MEAN, std=cases.ALT_STD),
                           stem_image(lib, H, W, rows, img=want_img))


@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_upsample_argmax_u8_equals_the_int32_kernel(lib, name, C, lo, hi):
    (h, w), (H, W) = lo, hi
    x = torch.from_numpy(cases.lowres_logits(name, C, h, w)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for off in (0, 1):
        l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
        holder = torch.full((H * W + 8,), 0xEE, dtype=torch.uint8, device="cuda")
        lib.check(lib.tdnet_op_upsample_argmax(x.data_ptr(), C, h, w, H, W, l32.data_ptr(), holder.data_ptr() + off, s))
        l8 = holder[off:off + H * W].reshape(H, W)
        assert int(l32.min()) >= 0 and int(l32.max()) < C
        assert torch.equal(l8.to(torch.int32), l32), (name, off)
        assert bool((holder[:off] == 0xEE).all()) and bool((holder[off + H * W:] == 0xEE).all())
    if name == "c256":
        assert bool((l8 == 255).any())
    if name == "ties":
        grid = l32[::8, ::16].cpu().numpy()
        assert (grid[[0, 1, 3, 4]] == 4).all() and (grid[2] == 3).all()


def make_model(name, bb, kernel_opts=None):
    from tdnet_amd.model import td2_psp50, td4_psp18
    if name == "td4":
        return td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts).eval().to("cuda")
    return td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts).eval().to("cuda")


def _cache_stages(m):
    lk, dk, dv = m.engine.cache_dims()
    return [m.engine.stage(st, shp).view(np.uint32) for st, shp in (("cache_q", (lk, dk)), ("cache_k", (lk, dk)), ("cache_v", (lk, dv)))]


@pytest.mark.parametrize("name,bb,H,W,Hs,Ws,opts", [("td4", "resnet18", 65, 129, 80, 161, None), ("td4", "resnet18", 65, 129, 80, 161, {"precision": 1}),
                                                    ("td4", "resnet18", 65, 129, 80, 161, {"precision": 3}), ("td2", "resnet50", 33, 65, 41, 83, None)],
                         ids=["td4-psp18", "td4-psp18-precision1", "td4-psp18-precision3", "td2-psp50"])
def test_frames_given_as_bytes_equal_frames_given_as_fp32(name, bb, H, W, Hs, Ws, opts):
    """Model A gets the loader's fp32 tensors throughout, model B the bytes on even steps and the fp32 tensors on odd ones."""
    a = make_model(name, bb, opts)
    a.ensure_engine(H, W, "cuda")
    b, c, d = (make_model(name, bb, opts).share_weights_with(a) for _ in range(3))   # own FIFOs on A's weights; labels: C fp32 -> int32, D bytes -> uint8
    P = a.path_num
    rng = np.random.default_rng(11)
    with torch.no_grad():
        for t in range(5):
            src = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
            x = torch.from_numpy(cases.expected_image(src, H, W)).cuda()
            u = torch.from_numpy(src[None]).cuda()
            oa = a(x, pos_id=t % P)
            ob = b.forward_u8(u, pos_id=t % P, in_size=(H, W)) if t % 2 == 0 else b(x, pos_id=t % P)
            assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), t
            assert a.engine.last_launch_count() == b.engine.last_launch_count() > 0, t
            for sa, sb in zip(_cache_stages(a), _cache_stages(b)):
                assert np.array_equal(sa, sb), t
            l32, l8 = c.forward_labels(x, pos_id=t % P), d.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            assert l8.dtype == torch.uint8 and torch.equal(l8, l32.to(torch.uint8)) and torch.equal(l8, a.argmax_u8(oa)), t
    assert b.engine.fifo_len() == a.engine.fifo_len()


def test_a_batch_of_byte_frames():
    """Two samples at 41x83: sample 1 starts 41 * 83 * 3 = 10209 bytes behind sample 0, an odd offset."""
    H, W, Hs, Ws = 33, 65, 41, 83
    a = make_model("td2", "resnet18")
    a.ensure_engine(H, W, "cuda")
    b = make_model("td2", "resnet18").share_weights_with(a)
    rng = np.random.default_rng(12)
    with torch.no_grad():
        for t in range(3):
            src = rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)
            x = torch.cat([torch.from_numpy(cases.expected_image(src[i], H, W)) for i in range(2)]).cuda()
            u = torch.from_numpy(src).cuda()
            assert (u[1].data_ptr() - u[0].data_ptr()) % 2 == 1
            oa, ob = a(x, pos_id=t % 2), b.forward_u8(u, pos_id=t % 2, in_size=(H, W))
            assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)), t
    assert not torch.equal(oa[0], oa[1])


def test_uint8_prefetcher_and_label_downloader():
    from tdnet_amd.dataloader import DevicePrefetcher, LabelDownloader
    H, W, Hs, Ws, T = 33, 65, 41, 83, 6
    a = make_model("td4", "resnet18")
    a.ensure_engine(H, W, "cuda")
    b = make_model("td4", "resnet18").share_weights_with(a)
    rng = np.random.default_rng(13)
    srcs = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(T)]
    items = [[torch.from_numpy(s[None]).pin_memory(), "f%d.png" % t, "vid", (W, H)] for t, s in enumerate(srcs)]
    got = {}
    with torch.no_grad():
        want = [a.forward_labels(torch.from_numpy(cases.expected_image(s, H, W)).cuda(), pos_id=t % 4).cpu().numpy() for t, s in enumerate(srcs)]
        down = LabelDownloader(torch.device("cuda"))
        for t, (img, name, folder, size) in enumerate(DevicePrefetcher(items, "cuda")):
            assert img.dtype == torch.uint8 and img.is_cuda and tuple(img.shape) == (1, Hs, Ws, 3)
            for tag, lab in down.submit(b.forward_labels_u8(img, pos_id=t % 4, in_size=(H, W)), t):
                got[tag] = lab.copy()
        for tag, lab in down.drain():
            got[tag] = lab.copy()
    assert sorted(got) == list(range(T))
    for t in range(T):
        assert got[t].dtype == np.uint8 and np.array_equal(got[t], want[t].astype(np.uint8)), t


def test_cli_with_and_without_u8_writes_the_same_pngs(tmp_path):
    from PIL import Image
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(14)
    for t in range(6):
        Image.fromarray(rng.integers(0, 256, (41, 83, 3), dtype=np.uint8)).save(frames_dir / ("frame_%06d.png" % t))
    outs = []
    for extra in ([], ["--u8"], ["--prefetch"], ["--prefetch", "--u8"]):
        out = tmp_path / ("out" + "".join(extra).replace("--", "_"))
        out.mkdir()
        r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out),
                            "--synthetic_seed", "0", "--in_size", "33x65"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(out)
    names = sorted(os.listdir(outs[0] / "vid1"))
    assert len(names) == 6
    for out in outs[1:]:
        for nm in names:
            assert (out / "vid1" / nm).read_bytes() == (outs[0] / "vid1" / nm).read_bytes(), (out.name, nm)
