"""NV12 surfaces into the frame's first launch (include/tdnet.h "NV12 frames in"), on the CPU through the kernel emulator: k_ingest_nv12 against
the packed-RGB route fed the oracle's bytes, whole frames given as surfaces against the same frames given as RGB bytes, and the error paths.
Every comparison is exact."""
import numpy as np
import pytest

import emu_util
import nv12_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


def _buffer(lib, H, W, rows):
    n = lib.check(lib.tdnet_op_stem_image(None, None, 0, 0, H, W, None, None, rows, None, 0, None))
    return np.full(n, np.float32(1234.5), np.float32)


def stem_image_rgb(lib, H, W, rows, img):
    """The complete stem image buffer (border included) of an fp32 NCHW image, as raw 32-bit words."""
    out = _buffer(lib, H, W, rows)
    assert lib.check(lib.tdnet_op_stem_image(img.ctypes.data, None, 0, 0, H, W, None, None, rows, out.ctypes.data, out.size, None)) == out.size
    return out.view(np.uint32)


def stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, standard, H, W, rows, mean=None, std=None):
    out = _buffer(lib, H, W, rows)
    got = lib.check(lib.tdnet_op_stem_image_nv12(addr, Hs, Ws, pitch, uv, standard, H, W, cases.double3(mean), cases.double3(std), rows,
                                                 out.ctypes.data, out.size, None))
    assert got == out.size
    return out.view(np.uint32)


@pytest.mark.parametrize("layout", [0, 1], ids=["tight", "padded"])
@pytest.mark.parametrize("name,src_size,net_size", cases.STEM_CASES, ids=[c[0] for c in cases.STEM_CASES])
def test_nv12_ingest_matches_the_rgb_route_bit_for_bit(lib, name, src_size, net_size, layout):
    (Hs, Ws), (H, W) = src_size, net_size
    _, pitch, uv = cases.layouts(Hs, Ws)[layout]
    if name == "same_33x65_all_y":
        assert len(np.unique(cases.planes(name, Hs, Ws)[0])) == 256
    want = {rows: stem_image_rgb(lib, H, W, rows, cases.expected_image(name, Hs, Ws, H, W)) for rows in (1, 0)}
    for fill in ((0x00, 0xFF) if layout else (0x00,)):                 # padding and gap filled with zeros, then with ones: the same output
        s = cases.surface(name, Hs, Ws, pitch, uv, fill)
        for off in (0, 1):
            holder, addr = cases.offset_copy(s, off)
            for rows in (1, 0):                                        # the packed-row image and NHWC4
                got = stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, 0, H, W, rows)
                assert np.array_equal(got, want[rows]), (name, rows, off, fill, int((got != want[rows]).sum()))
            assert (holder[:off] == 0xA5).all() and (holder[off + s.size:] == 0xA5).all() and np.array_equal(holder[off:off + s.size], s)


@pytest.mark.parametrize("standard", [0, 1, 2, 3])
def test_all_four_standards(lib, standard):
    name, (Hs, Ws), (H, W) = cases.STEM_CASES[5]
    _, pitch, uv = cases.layouts(Hs, Ws)[1]
    want_img = cases.expected_image(name, Hs, Ws, H, W, standard)
    if standard:
        assert not np.array_equal(want_img, cases.expected_image(name, Hs, Ws, H, W, 0))
    holder, addr = cases.offset_copy(cases.surface(name, Hs, Ws, pitch, uv, 0x33), 1)
    for rows in (1, 0):
        assert np.array_equal(stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, standard, H, W, rows), stem_image_rgb(lib, H, W, rows, want_img))


def test_other_mean_and_std(lib):
    name, (Hs, Ws), (H, W) = cases.STEM_CASES[5]
    _, pitch, uv = cases.layouts(Hs, Ws)[0]
    want_img = cases.expected_image(name, Hs, Ws, H, W, 0, cases.ALT_MEAN, cases.ALT_STD)
    assert not np.array_equal(want_img, cases.expected_image(name, Hs, Ws, H, W))
    holder, addr = cases.offset_copy(cases.surface(name, Hs, Ws, pitch, uv), 3)
    for rows in (1, 0):
        assert np.array_equal(stem_image_nv12(lib, addr, Hs, Ws, pitch, uv, 0, H, W, rows, cases.ALT_MEAN, cases.ALT_STD),
                              stem_image_rgb(lib, H, W, rows, want_img))


class HostMem:
    """run_frame_scenario's memory: numpy arrays stand in for HBM."""

    def up(self, a, off=0):
        holder, addr = cases.offset_copy(np.ascontiguousarray(a).view(np.uint8).reshape(-1), off)
        return holder, addr

    def out(self, shape, dtype, fill):
        return np.full(shape, fill, dtype)

    def addr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf


def _engine(lib, H=33, W=65):
    spec = arch.model_spec("td2", 19, "resnet18")
    e = Engine(2, 18, 19, H, W, 0, lib=lib)
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


def test_frames_given_as_surfaces_equal_frames_given_as_rgb_bytes(lib):
    a = _engine(lib, *cases.FRAME_NET)
    cases.run_frame_scenario(a, HostMem())
    a.close()


def test_errors_leave_the_configuration_and_the_fifo_alone(lib):
    H, W = cases.FRAME_NET
    Hs, Ws = 41, 83
    e = _engine(lib, H, W)
    _, pitch, uv = cases.layouts(Hs, Ws)[0]
    s = cases.surface("down_41x83", Hs, Ws, pitch, uv)
    rgb = cases.expected_rgb("down_41x83", Hs, Ws)
    out, ref = np.zeros((1, 19, H, W), np.float32), np.zeros((1, 19, H, W), np.float32)
    with pytest.raises(_capi.TdnetError, match="tdnet_set_input_u8"):  # a byte frame on an unconfigured handle: the message stays
        e.forward_u8(s, 0, out)
    with pytest.raises(_capi.TdnetError, match="pitch"):               # a rejected configuration configures nothing
        e.set_input_nv12(Hs, Ws, 82)
    with pytest.raises(_capi.TdnetError, match="tdnet_set_input_u8"):
        e.forward_u8(s, 0, out)
    assert e.fifo_len() == 0
    e.set_input_nv12(Hs, Ws, pitch, uv)
    e.forward_u8(s, 0, ref)
    assert e.fifo_len() == 1
    bad = [("at least 1", dict(src_height=0, src_width=Ws, pitch=pitch)), ("at least 1", dict(src_height=Hs, src_width=0, pitch=pitch)),
           ("pitch", dict(src_height=Hs, src_width=Ws, pitch=83)), ("pitch", dict(src_height=Hs, src_width=Ws, pitch=-4)),
           ("uv_offset", dict(src_height=Hs, src_width=Ws, pitch=pitch, uv_offset=Hs * pitch - 1)),
           ("extent", dict(src_height=Hs, src_width=Ws, pitch=pitch, uv_offset=2 ** 31)),
           ("extent", dict(src_height=40000, src_width=Ws, pitch=60000)),
           ("standard", dict(src_height=Hs, src_width=Ws, pitch=pitch, standard=4)), ("standard", dict(src_height=Hs, src_width=Ws, pitch=pitch, standard=-1)),
           ("std", dict(src_height=Hs, src_width=Ws, pitch=pitch, std=(0.2, 0.0, 0.2))), ("std", dict(src_height=Hs, src_width=Ws, pitch=pitch, std=(0.2, float("nan"), 0.2))),
           ("mean", dict(src_height=Hs, src_width=Ws, pitch=pitch, mean=(0.2, float("inf"), 0.2)))]
    for match, kw in bad:
        with pytest.raises(_capi.TdnetError, match=match) as err:
            e.set_input_nv12(**kw)
        assert "tdnet_set_input_nv12" in str(err.value), kw
        assert e.fifo_len() == 1, kw
        e.reset()                                                      # the previous configuration still serves the frame, identically
        e.forward_u8(s, 0, out)
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)) and e.fifo_len() == 1, kw
    # the same after a packed-RGB configuration: a failed NV12 call leaves THAT in force
    e.set_input_u8(Hs, Ws)
    with pytest.raises(_capi.TdnetError, match="standard"):
        e.set_input_nv12(Hs, Ws, pitch, standard=7)
    e.reset()
    e.forward_u8(rgb, 0, out)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized"):
        fresh.set_input_nv12(Hs, Ws, pitch)
    fresh.close()
    e.close()


def test_model_classes_check_the_surface_tensor():
    import torch
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    ok = torch.zeros(1, 63, 96, dtype=torch.uint8)                     # 42 + 21 rows
    for call in (m.forward_nv12, m.forward_labels_nv12, m.encode_nv12):
        with pytest.raises(RuntimeError, match="uint8"):                # dtype
            call(torch.zeros(1, 63, 96), 0, src_size=(42, 84), in_size=(33, 65))
        with pytest.raises(RuntimeError, match="N,rows,pitch"):         # rank
            call(torch.zeros(63, 96, dtype=torch.uint8), 0, src_size=(42, 84), in_size=(33, 65))
        with pytest.raises(RuntimeError, match="src_size"):
            call(ok, 0, in_size=(33, 65))
        with pytest.raises(RuntimeError, match="pitch"):
            call(ok, 0, src_size=(42, 98), in_size=(33, 65))
        with pytest.raises(RuntimeError, match="uv_offset"):
            call(ok, 0, src_size=(42, 84), in_size=(33, 65), uv_offset=41 * 96)
        with pytest.raises(RuntimeError, match="needs"):                # rows * pitch >= extent
            call(ok[:, :62], 0, src_size=(42, 84), in_size=(33, 65))
        with pytest.raises(RuntimeError, match="needs"):
            call(ok, 0, src_size=(42, 84), in_size=(33, 65), uv_offset=43 * 96)
        with pytest.raises(RuntimeError, match="standard"):
            call(ok, 0, src_size=(42, 84), in_size=(33, 65), standard=4)
        with pytest.raises(_capi.TdnetError):                           # no CPU fallback
            call(ok, 0, src_size=(42, 84), in_size=(33, 65))
    assert m.engine is None                                            # nothing was built on the way
