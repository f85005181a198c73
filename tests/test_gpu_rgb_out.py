"""Colour maps out on the MI355X: the operator cases of tests/test_emu_rgb_out.py on device memory (plus rows wider than one workgroup's strip
and the real 769x1537 geometry), whole frames asked for as pictures against the same frames asked for as labels, a captured pos_id cycle, and
the command line with --rgb.  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import opcheck
import rgb_out_cases as cases
from tdnet_amd import _capi
from tdnet_amd.dataloader import nearest_index

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


def test_c_tables_equal_nearest_index(lib):
    def c_table(n, on):
        out = np.full(on, -7, np.int32)
        lib.check(lib.tdnet_op_nearest_index(n, on, out.ctypes.data))
        return out
    for n, on in cases.TABLE_PAIRS + [(n, on) for n in range(1, 41) for on in range(1, 41)]:
        assert np.array_equal(c_table(n, on), nearest_index(n, on)), (n, on)


def labels_of(lib, x, C, h, w, H, W):
    l32 = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    lib.check(lib.tdnet_op_upsample_argmax(x.data_ptr(), C, h, w, H, W, l32.data_ptr(), None, torch.cuda.current_stream().cuda_stream))
    l32 = l32.cpu().numpy()
    assert l32.min() >= 0 and l32.max() < C
    return l32


@opcheck.guarded_arg("x", True)
def picture(lib, H, W, oh, ow, palette, off, x=None, C=0, h=0, w=0, labels_u8=None):
    """The picture written `off` bytes into a device holder of 0xEE; the guard bytes around it must survive."""
    n = oh * ow * 3
    holder = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    palette = np.ascontiguousarray(palette)
    lib.check(lib.tdnet_op_upsample_argmax_rgb(None if x is None else x.data_ptr(), C, h, w, H, W, oh, ow, palette.ctypes.data, len(palette),
                                               holder.data_ptr() + off, None if labels_u8 is None else labels_u8.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
    host = holder.cpu().numpy()
    assert (host[:off] == 0xEE).all() and (host[off + n:] == 0xEE).all(), (oh, ow, off)
    return host[off:off + n].reshape(oh, ow, 3)


@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_fused_kernel_and_labels_kernel_equal_labels_sampled_and_decoded(lib, name, C, lo, hi):
    (h, w), (H, W) = lo, hi
    x = torch.from_numpy(cases.lowres_logits(name, C, h, w)).cuda()
    labels = labels_of(lib, x, C, h, w, H, W)
    l8 = torch.from_numpy(labels.astype(np.uint8)).cuda()
    pals = [cases.palette19()] + ([cases.palette40()] if C == 19 else [])
    for pal in pals:
        for oh, ow in cases.out_sizes(H, W):
            want = cases.expected_picture(labels, oh, ow, pal)
            for off in range(4):
                assert np.array_equal(picture(lib, H, W, oh, ow, pal, off, x, C, h, w), want), (name, oh, ow, off)
            for off in (0, 1):
                assert np.array_equal(picture(lib, H, W, oh, ow, pal, off, labels_u8=l8), want), (name, oh, ow, off)
    if name == "c256":                                                 # label 255 reaches the grey branch
        assert (picture(lib, H, W, H, W, pals[0], 0, x, C, h, w) == 255).all(axis=2).any()
    if name == "ties":                                                 # the lower index still wins
        got = picture(lib, H, W, H, W, pals[0], 0, x, C, h, w)[::8, ::16]
        assert (got[[0, 1, 3, 4]] == pals[0][4]).all() and (got[2] == pals[0][3]).all()


def test_labels_outside_the_palette_are_grey(lib):
    name, C, (h, w), (H, W) = cases.ARGMAX_CASES[0]
    x40 = torch.from_numpy(cases.logits40(h, w)).cuda()
    l40 = labels_of(lib, x40, 40, h, w, H, W)
    assert (l40 >= 19).any()
    for oh, ow in cases.out_sizes(H, W):
        assert np.array_equal(picture(lib, H, W, oh, ow, cases.palette19(), 1, x40, 40, h, w), cases.expected_picture(l40, oh, ow)), (oh, ow)
    full = picture(lib, H, W, H, W, cases.palette19(), 0, x40, 40, h, w)
    grey = l40 >= 19
    assert (full[grey] == l40[grey][:, None]).all()


@pytest.mark.parametrize("name,C,lo,hi,sizes", cases.WIDE_CASES, ids=[c[0] for c in cases.WIDE_CASES])
def test_wide_rows_and_the_real_geometry(lib, name, C, lo, hi, sizes):
    (h, w), (H, W) = lo, hi
    x = torch.from_numpy(np.random.default_rng(H + W).standard_normal((C, h, w)).astype(np.float32)).cuda()
    labels = labels_of(lib, x, C, h, w, H, W)
    l8 = torch.from_numpy(labels.astype(np.uint8)).cuda()
    pal = cases.palette19()
    for oh, ow in sizes:
        want = cases.expected_picture(labels, oh, ow)
        for off in range(4):
            assert np.array_equal(picture(lib, H, W, oh, ow, pal, off, x, C, h, w), want), (name, oh, ow, off)
        for off in (0, 1):
            assert np.array_equal(picture(lib, H, W, oh, ow, pal, off, labels_u8=l8), want), (name, oh, ow, off)


def make_model(name, bb="resnet18", kernel_opts=None):
    from tdnet_amd.model import pspnet, td2_psp50, td4_psp18
    if name == "td4":
        m = td4_psp18.td4_psp18(nclass=19, path_num=4, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts)
    elif name == "td2":
        m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts)
    else:
        m = pspnet.pspnet(nclass=19, model_path=None, backbone=bb, synthetic_seed=0, kernel_opts=kernel_opts)
    return m.eval().to("cuda")


def _sizes(H, W, t):
    return (H // 4, W // 4) if t % 2 == 0 else (7, 17)


@pytest.mark.parametrize("name,H,W,Hs,Ws,opts", [("td4", 65, 129, 80, 161, None), ("td2", 33, 65, 41, 83, None), ("td4", 65, 129, 80, 161, {"precision": 1})],
                         ids=["td4-psp18-65x129", "td2-psp18-33x65", "td4-psp18-precision1"])
def test_frames_asked_for_as_pictures_equal_frames_asked_for_as_labels(name, H, W, Hs, Ws, opts):
    """Six frames of random bytes.  Model B: forward_labels_u8 throughout; A: forward_rgb_u8 throughout (quarter size on even frames, 7x17 on odd
    ones: a reconfiguration takes effect on the next frame); C in turn forward_rgb_u8, forward_labels_u8 (+ labels_rgb) and encode_u8 +
    propagate(labels="rgb").  Same pictures, same labels, same launch counts."""
    b = make_model(name, kernel_opts=opts)
    b.ensure_engine(H, W, "cuda")
    a, c = (make_model(name, kernel_opts=opts).share_weights_with(b) for _ in range(2))
    P = b.path_num
    rng = np.random.default_rng(31)
    with torch.no_grad():
        for t in range(6):
            src = rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)
            u = torch.from_numpy(src).cuda()
            out_size = _sizes(H, W, t)
            l8 = b.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
            want = cases.expected_picture(l8[0].cpu().numpy(), *out_size)
            got = a.forward_rgb_u8(u, t % P, (H, W), out_size)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + out_size + (3,)
            assert np.array_equal(got[0].cpu().numpy(), want), t
            assert a.engine.last_launch_count() == b.engine.last_launch_count() > 0, t
            if t % 3 == 0:
                got_c = c.forward_rgb_u8(u, t % P, (H, W), out_size)
                assert c.engine.last_launch_count() == b.engine.last_launch_count()
            elif t % 3 == 1:
                l8c = c.forward_labels_u8(u, pos_id=t % P, in_size=(H, W))
                assert torch.equal(l8c, l8), t
                got_c = c.labels_rgb(l8c, out_size)
            else:
                c.encode_u8(u, t % P, in_size=(H, W))
                got_c = c.propagate(labels="rgb", out_size=out_size)
            assert np.array_equal(got_c[0].cpu().numpy(), want), t
    assert a.engine.fifo_len() == b.engine.fifo_len() == c.engine.fifo_len()


def test_a_batch_of_two_and_another_palette():
    H, W, Hs, Ws = 33, 65, 41, 83
    b = make_model("td2")
    b.ensure_engine(H, W, "cuda")
    a = make_model("td2").share_weights_with(b)
    rng = np.random.default_rng(32)
    pal = cases.palette40()
    with torch.no_grad():
        for t in range(3):
            u = torch.from_numpy(rng.integers(0, 256, (2, Hs, Ws, 3), dtype=np.uint8)).cuda()
            l8 = b.forward_labels_u8(u, pos_id=t % 2, in_size=(H, W)).cpu().numpy()
            got = a.forward_rgb_u8(u, t % 2, (H, W), (9, 19), palette=pal).cpu().numpy()   # sample 1's picture starts 9 * 19 * 3 = 513 bytes in: odd
            for i in range(2):
                assert np.array_equal(got[i], cases.expected_picture(l8[i], 9, 19, pal)), (t, i)
    assert not np.array_equal(got[0], got[1])


def test_pspnet_and_fp32_frames_through_forward_rgb():
    from tdnet_amd import weights
    H, W = 33, 65
    m = make_model("psp")
    x = torch.from_numpy(weights.synth_video(H, W, 1, seed=3)[0]).cuda()
    with torch.no_grad():
        l32 = m.forward_labels(x)
        n_labels = m.engine.last_launch_count()
        got = m.forward_rgb(x, out_size=(8, 16))
    assert np.array_equal(got[0].cpu().numpy(), cases.expected_picture(l32[0].cpu().numpy(), 8, 16))
    assert m.engine.last_launch_count() == n_labels > 0


def test_errors_leave_a_pending_frame_alone():
    H, W, Hs, Ws = 33, 65, 41, 83
    m = make_model("td2")
    ref = make_model("td2")
    u = torch.from_numpy(np.random.default_rng(33).integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda()
    pal = cases.palette19()
    with torch.no_grad():
        m.encode_u8(u, 0, in_size=(H, W))
        e = m.engine
        pic = torch.zeros((8, 16, 3), dtype=torch.uint8, device="cuda")
        for call in (lambda: e.forward_u8_rgb(u.data_ptr(), 1, pic.data_ptr()), lambda: e.propagate_rgb(pic.data_ptr())):
            with pytest.raises(_capi.TdnetError, match="tdnet_set_output_rgb"):
                call()
        for bad, match in (((0, 16, pal), "at least 1"), ((8, 0, pal), "at least 1"), ((8, 16, np.zeros((257, 3), np.uint8)), "n_colours"),
                           ((8, 16, np.zeros((0, 3), np.uint8)), "n_colours")):
            with pytest.raises(_capi.TdnetError, match=match):
                e.set_output_rgb(*bad)
        assert e.lib.tdnet_set_output_rgb(e.h, 8, 16, None, 19) < 0 and b"NULL" in e.lib.tdnet_last_error()
        e.set_output_rgb(8, 16, pal)
        with pytest.raises(_capi.TdnetError, match="waiting for tdnet_propagate"):
            e.forward_u8_rgb(u.data_ptr(), 1, pic.data_ptr())
        got = m.propagate(labels="rgb", out_size=(8, 16))              # the pending frame is still there, and is the frame it was
        want = cases.expected_picture(ref.forward_labels_u8(u, pos_id=0, in_size=(H, W))[0].cpu().numpy(), 8, 16)
        assert np.array_equal(got[0].cpu().numpy(), want)
        with pytest.raises(_capi.TdnetError, match="no encoded frame"):
            e.propagate_rgb(pic.data_ptr())
        shared = e.share()                                             # a shared handle is unconfigured until it is configured itself
        shared.set_input_u8(Hs, Ws)
        with pytest.raises(_capi.TdnetError, match="tdnet_set_output_rgb"):
            shared.forward_u8_rgb(u.data_ptr(), 0, pic.data_ptr())
        shared.close()


def test_a_captured_cycle_of_picture_frames_replays_to_the_eager_pictures():
    """One pos_id cycle of forward_rgb_u8 at 65x129 captured into a hipGraph (tdnet_warmup and tdnet_set_output_rgb before the capture) and
    replayed for the following cycles: bit for bit the eager pictures."""
    H, W, Hs, Ws, P, cycles = 65, 129, 80, 161, 4, 2
    out_size = (H // 4, W // 4)
    warm = 2 * P
    T = warm + cycles * P
    rng = np.random.default_rng(34)
    clip = [torch.from_numpy(rng.integers(0, 256, (1, Hs, Ws, 3), dtype=np.uint8)).cuda() for _ in range(T)]
    with torch.no_grad():
        m = make_model("td4")
        eager = [m.forward_rgb_u8(clip[t], t % P, (H, W), out_size).clone() for t in range(T)]
        m.reset()
        for t in range(warm):                                          # steady state; the handle is configured (input and output) by these frames
            assert torch.equal(m.forward_rgb_u8(clip[t], t % P, (H, W), out_size), eager[t])
        stream = torch.cuda.Stream()
        xin = torch.zeros((P, 1, Hs, Ws, 3), dtype=torch.uint8, device="cuda")
        m.engine.warmup(stream.cuda_stream)
        m.engine.set_output_rgb(out_size[0], out_size[1], cases.palette19())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = [m.forward_rgb_u8(xin[j], j, (H, W), out_size) for j in range(P)]
        for c in range(cycles):
            t0 = warm + c * P
            for j in range(P):
                xin[j].copy_(clip[t0 + j])
            graph.replay()
            torch.cuda.synchronize()
            for j in range(P):
                assert torch.equal(outs[j], eager[t0 + j]), (c, j)
    assert not torch.equal(eager[-1], eager[-2])


def test_cli_with_and_without_rgb_writes_the_same_pngs(tmp_path):
    from PIL import Image
    frames_dir = tmp_path / "data" / "vid1"
    frames_dir.mkdir(parents=True)
    rng = np.random.default_rng(14)
    for t in range(5):
        Image.fromarray(rng.integers(0, 256, (80, 161, 3), dtype=np.uint8)).save(frames_dir / ("frame_%06d.png" % t))
    outs = []
    for extra in (["--u8", "--prefetch"], ["--u8", "--prefetch", "--rgb"], ["--rgb"]):   # the last: fp32 frames, the reference's one-by-one loop
        out = tmp_path / ("out" + "".join(extra).replace("--", "_"))
        out.mkdir()
        r = subprocess.run([sys.executable, "-m", "tdnet_amd.test", "--img_path", str(tmp_path / "data"), "--output_path", str(out),
                            "--synthetic_seed", "0", "--in_size", "65x129"] + extra, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append(out)
    names = sorted(os.listdir(outs[0] / "vid1"))
    assert len(names) == 5
    for out in outs[1:]:
        for nm in names:
            assert (out / "vid1" / nm).read_bytes() == (outs[0] / "vid1" / nm).read_bytes(), (out.name, nm)
    assert np.asarray(Image.open(outs[1] / "vid1" / names[0])).shape == (65 // 4, 129 // 4, 3)
