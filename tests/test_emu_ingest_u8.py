"""uint8 frames in, uint8 labels out (include/tdnet.h), on the CPU through the kernel emulator: the ingest kernel against the host loader's
resize + normalisation, the uint8 label kernels against the int32 ones, whole frames given as bytes against the same frames given as the
loader's fp32 tensors, and the error paths.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

import emu_util
import ingest_u8_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


def stem_image(lib, H, W, rows, img=None, src_addr=None, src_size=(0, 0), mean=None, std=None):
    """The complete stem image buffer (border included) through tdnet_op_stem_image, as raw 32-bit words."""
    n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))
    out = np.full(n, np.float32(1234.5), np.float32)
    got = lib.check(lib.tdnet_op_stem_image(None if img is None else img.ctypes.data, src_addr, src_size[0], src_size[1], H, W,
                                            cases.double3(mean), cases.double3(std), rows, out.ctypes.data, out.size, None))
    assert got == n
    return out.view(np.uint32)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("name,src_size,net_size", cases.STEM_CASES, ids=[c[0] for c in cases.STEM_CASES])
def test_ingest_matches_the_host_loader_bit_for_bit(lib, name, src_size, net_size, off):
    (Hs, Ws), (H, W) = src_size, net_size
    src = cases.source(name, Hs, Ws)
    if name == "same_33x65_all_bytes":
        assert all(len(np.unique(src[..., c])) == 256 for c in range(3))
    want_img = cases.expected_image(src, H, W)
    if name == "down_exact_2x":                                        # the pin test_dataloader.py uses: exact 2x = 2x2 box average
        assert np.array_equal(want_img, cases.loader(H, W).normalise(cases.box_average_2x(src)).numpy())
    holder, addr = cases.offset_copy(src, off)
    for rows in (1, 0):                                                # the packed-row image and NHWC4
        want = stem_image(lib, H, W, rows, img=want_img)
        got = stem_image(lib, H, W, rows, src_addr=addr, src_size=(Hs, Ws))
        assert np.array_equal(got, want), (name, rows, off, int((got != want).sum()))
    assert (holder[:off] == 0xA5).all() and (holder[off + src.size:] == 0xA5).all()


def test_ingest_with_other_mean_and_std(lib):
    (Hs, Ws), (H, W) = (41, 83), (33, 65)
    src = cases.source("down_41x83", Hs, Ws)
    want_img = cases.expected_image(src, H, W, cases.ALT_MEAN, cases.ALT_STD)
    assert not np.array_equal(want_img, cases.expected_image(src, H, W))
    holder, addr = cases.offset_copy(src, 3)
    for rows in (1, 0):
        assert np.array_equal(stem_image(lib, H, W, rows, src_addr=addr, src_size=(Hs, Ws), mean=cases.ALT_MEAN, std=cases.ALT_STD),
                              stem_image(lib, H, W, rows, img=want_img))


@pytest.mark.parametrize("name,C,lo,hi", cases.ARGMAX_CASES, ids=[c[0] for c in cases.ARGMAX_CASES])
def test_upsample_argmax_u8_equals_the_int32_kernel(lib, name, C, lo, hi):
    (h, w), (H, W) = lo, hi
    x = cases.lowres_logits(name, C, h, w)
    for off in (0, 1):                                                 # label rows at every alignment
        l32 = np.full((H, W), -1, np.int32)
        holder = np.full(H * W + 8, 0xEE, np.uint8)
        lib.check(lib.tdnet_op_upsample_argmax(x.ctypes.data, C, h, w, H, W, l32.ctypes.data, holder.ctypes.data + off, None))
        l8 = holder[off:off + H * W].reshape(H, W)
        assert l32.min() >= 0 and l32.max() < C
        assert np.array_equal(l8.astype(np.int32), l32), (name, off)
        assert (holder[:off] == 0xEE).all() and (holder[off + H * W:] == 0xEE).all()
    if name == "c256":
        assert (l8 == 255).any()
    if name == "c1":
        assert not l8.any()
    if name == "ties":                                                 # output pixels (8 k, 16 j) ARE the planted low-resolution pixels: both channels hold the same value
        grid = l32[::8, ::16]
        assert (grid[[0, 1, 3, 4]] == 4).all() and (grid[2] == 3).all()


def _engine(lib, H=33, W=65):
    spec = arch.model_spec("td2", 19, "resnet18")
    e = Engine(2, 18, 19, H, W, 0, lib=lib)
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return spec, e


def test_frames_given_as_bytes_equal_frames_given_as_fp32(lib):
    """td2-psp18 at 33x65, 5 frames of random bytes at 41x83.  Handle A gets the loader's fp32 tensors throughout; handle B the bytes on even
    steps and the fp32 tensors on odd ones: logits and cache entries identical at every step, the same number of launches."""
    H, W, Hs, Ws, nc = 33, 65, 41, 83, 19
    spec, a = _engine(lib, H, W)
    b = a.share()
    b.set_input_u8(Hs, Ws)
    b.set_input_u8(Hs, Ws)                                             # idempotent
    h, w = a.feature_dims()
    lk = ((h - 1) // 4 + 1) * ((w - 1) // 4 + 1)
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(5)]
    c, d = a.share(), a.share()                                        # labels: C fp32 -> int32, D bytes -> uint8
    d.set_input_u8(Hs, Ws)
    for t, src in enumerate(frames):
        x = cases.expected_image(src, H, W)
        oa, ob = np.full((1, nc, H, W), 7e7, np.float32), np.full((1, nc, H, W), -7e7, np.float32)
        a.forward(x, t % 2, oa)
        if t % 2 == 0:
            holder, addr = cases.offset_copy(src, t // 2)              # byte offsets 0, 1, 2
            b.forward_u8(addr, t % 2, ob)
        else:
            b.forward(x, t % 2, ob)
        assert np.array_equal(oa.view(np.uint32), ob.view(np.uint32)), t
        assert a.last_launch_count() == b.last_launch_count() > 0, t
        for st, shp in (("cache_q", (lk, 64)), ("cache_k", (lk, 64)), ("cache_v", (lk, spec.d_v))):
            assert np.array_equal(a.stage(st, shp).view(np.uint32), b.stage(st, shp).view(np.uint32)), (t, st)
        assert a.fifo_len() == b.fifo_len()
        if t < 2:                                                      # a warm-up frame and a steady one
            l32, l8 = np.full((H, W), -1, np.int32), np.full((H, W), 0xEE, np.uint8)
            c.forward_labels(x, t % 2, l32)
            d.forward_u8_labels(src, t % 2, l8)
            assert np.array_equal(l8, l32.astype(np.uint8)) and np.array_equal(l32, oa[0].argmax(0)), t
            assert c.last_launch_count() == d.last_launch_count()
            l8b = np.full((H, W), 0xEE, np.uint8)
            a.argmax_u8(oa, l8b)
            assert np.array_equal(l8b, l8), t
    # the split frame: encode_u8 + propagate_labels_u8 on D against forward_labels on C
    x = cases.expected_image(frames[2], H, W)
    l32, l8 = np.full((H, W), -1, np.int32), np.full((H, W), 0xEE, np.uint8)
    c.forward_labels(x, 0, l32)
    d.encode_u8(frames[2], 0)
    d.propagate_labels_u8(l8)
    assert np.array_equal(l8, l32.astype(np.uint8))
    for e in (b, c, d, a):
        e.close()


def test_errors_leave_the_fifo_alone(lib):
    H, W = 33, 65
    spec, e = _engine(lib, H, W)
    x = np.zeros((1, 3, H, W), np.float32)
    out = np.zeros((1, 19, H, W), np.float32)
    e.forward(x, 0, out)
    assert e.fifo_len() == 1
    src, lab = np.zeros((41, 83, 3), np.uint8), np.zeros((H, W), np.uint8)
    for call in (lambda: e.forward_u8(src, 1, out), lambda: e.forward_u8_labels(src, 1, lab), lambda: e.encode_u8(src, 1)):
        with pytest.raises(_capi.TdnetError, match="tdnet_set_input_u8"):   # a frame call before the configuration
            call()
        assert e.fifo_len() == 1
    with pytest.raises(_capi.TdnetError, match="at least 1"):
        e.set_input_u8(0, 83)
    with pytest.raises(_capi.TdnetError, match="at least 1"):
        e.set_input_u8(41, 0)
    with pytest.raises(_capi.TdnetError, match="std"):
        e.set_input_u8(41, 83, std=(0.2, 0.0, 0.2))
    with pytest.raises(_capi.TdnetError, match="std"):
        e.set_input_u8(41, 83, std=(0.2, float("nan"), 0.2))
    with pytest.raises(_capi.TdnetError, match="tdnet_set_input_u8"):   # a rejected configuration configures nothing
        e.forward_u8(src, 1, out)
    assert e.fifo_len() == 1
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_input_u8(41, 83)
    fresh.close()
    e.set_input_u8(41, 83)                                             # and a good one still works afterwards
    e.forward_u8(src, 1, out)
    assert e.fifo_len() == 1                                           # td2: depth 1
    e.close()


def test_model_classes_check_the_uint8_tensor():
    import torch
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    for call in (m.forward_u8, m.forward_labels_u8, m.encode_u8):
        with pytest.raises(RuntimeError, match="uint8"):                # dtype
            call(torch.zeros(1, 41, 83, 3), 0, in_size=(33, 65))
        with pytest.raises(RuntimeError, match="Hs,Ws,3"):              # rank
            call(torch.zeros(41, 83, 3, dtype=torch.uint8), 0, in_size=(33, 65))
        with pytest.raises(RuntimeError, match="Hs,Ws,3"):              # last dimension
            call(torch.zeros(1, 3, 41, 83, dtype=torch.uint8), 0, in_size=(33, 65))
        with pytest.raises(_capi.TdnetError):                           # no CPU fallback
            call(torch.zeros(1, 41, 83, 3, dtype=torch.uint8), 0, in_size=(33, 65))
    assert m.engine is None                                            # nothing was built on the way
    with pytest.raises(RuntimeError):                                  # forward() accepts what it accepted before
        m(torch.zeros(1, 41, 83, 3, dtype=torch.uint8), pos_id=0)
