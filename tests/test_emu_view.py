"""Source views (include/tdnet.h "source views") on the CPU through the kernel emulator: the ingest kernels of every format against the fp32 route
fed the oracle's image, the overlay kernels against the host oracle, whole frames given as views against the same frames given as RGB bytes, and
the error paths.  An out-of-extent read shows here as a host fault or a changed guard byte.  Every comparison is exact."""
import numpy as np
import pytest

import emu_util
import view_cases as cases
from tdnet_amd import _capi, arch, weights
from tdnet_amd.dataloader import PIX_NV12, PIX_RGB24, SourceView, view_to_rgb_u8
from tdnet_amd.engine import Engine


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


class HostMem:
    """The scenarios' memory: numpy arrays stand in for HBM."""
    stream = None

    def up(self, a, off=0):
        flat = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        holder = np.full(flat.size + 64, 0xA5, np.uint8)
        holder[off:off + flat.size] = flat
        return holder, holder.ctypes.data + off

    def out(self, shape, dtype, fill):
        return np.full(shape, fill, dtype)

    def addr(self, buf):
        return buf.ctypes.data

    def get(self, buf):
        return buf


MEM = HostMem()


def test_whole_tight_rgb24_view_is_the_uint8_entry_bit_for_bit(lib):
    H, W = 33, 65
    view = SourceView(PIX_RGB24, H, W)
    s = cases.view_bytes(view)
    for rows in (1, 0):
        n = cases.stem_buffer_size(lib, H, W, rows)
        out = np.full(n, np.float32(1234.5), np.float32)
        holder, addr = MEM.up(s, 1)
        assert lib.check(lib.tdnet_op_stem_image(None, addr, H, W, H, W, None, None, rows, out.ctypes.data, n, None)) == n
        assert np.array_equal(cases.stem_image_view(lib, MEM, addr, view, H, W, rows), out.view(np.uint32))
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
    view = cases.nv12_view((3, 7, 41, 83), 1, standard=standard)
    if standard:
        assert not np.array_equal(cases.expected_image(view, 33, 65), cases.expected_image(cases.nv12_view((3, 7, 41, 83), 1), 33, 65))
    cases.run_stem_case(lib, MEM, view, [(33, 65)], offsets=(1,), fills=(0x33,))


def test_other_mean_and_std(lib):
    view = cases.packed_view(cases.PACKED[3], (3, 7, 41, 83))
    holder, addr = MEM.up(cases.view_bytes(view), 3)
    want_img = cases.expected_image(view, 33, 65, 0, cases.u8cases.ALT_MEAN, cases.u8cases.ALT_STD)
    assert not np.array_equal(want_img, cases.expected_image(view, 33, 65))
    for rows in (1, 0):
        assert np.array_equal(cases.stem_image_view(lib, MEM, addr, view, 33, 65, rows, cases.u8cases.ALT_MEAN, cases.u8cases.ALT_STD),
                              cases.stem_image_ref(lib, MEM, 33, 65, rows, want_img))


@pytest.mark.parametrize("fmt", cases.OVERLAY_PACKED, ids=[cases.NAMES[f] for f in cases.OVERLAY_PACKED])
def test_overlay_of_packed_views(lib, fmt):
    cases.run_overlay_case(lib, MEM, cases.packed_view(fmt, cases.OVERLAY_RECT))


@pytest.mark.parametrize("origin", cases.OVERLAY_NV12_ORIGINS, ids=["2_5", "3_4"])
def test_overlay_of_nv12_views(lib, origin):
    cases.run_overlay_case(lib, MEM, cases.nv12_view(origin + (41, 83), 1))


def _engine(lib, H=33, W=65):
    spec = arch.model_spec("td2", 19, "resnet18")
    e = Engine(2, 18, 19, H, W, 0, lib=lib)
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


def test_frames_given_as_views_equal_frames_given_as_rgb_bytes(lib):
    a = _engine(lib, *cases.FRAME_NET)
    cases.run_view_scenario(a, MEM)
    a.close()


def test_errors_leave_the_configuration_and_the_fifo_alone(lib):
    H, W = cases.FRAME_NET
    e = _engine(lib, H, W)
    view = cases.packed_view(cases.PACKED[3], (3, 7, 41, 83))
    s = cases.view_bytes(view)
    rgb = view_to_rgb_u8(s, view)
    ref = np.zeros((1, 19, H, W), np.float32)
    with pytest.raises(_capi.TdnetError, match="reserved"):            # a rejected configuration configures nothing
        e.lib.check(e.lib.tdnet_set_input_view(e.h, next(t for m, t, _, _ in cases.bad_views() if m == "reserved"), None, None))
    with pytest.raises(_capi.TdnetError, match="tdnet_set_input_u8"):
        e.forward_u8(s, 0, ref)
    assert e.fifo_len() == 0
    # the previous configuration a view ...
    e.set_input_view(view)
    e.forward_u8(s, 0, ref)
    cases.run_error_cases(e, MEM, "view", s.ctypes.data, ref.view(np.uint32).copy(), H, W)
    # ... plain packed RGB ...
    e.set_input_u8(41, 83)
    cases.run_error_cases(e, MEM, "u8", rgb.ctypes.data, ref.view(np.uint32).copy(), H, W)
    # ... and an NV12 surface
    nv = cases.nv12_view((0, 0, 0, 0), 1)
    surf = cases.view_bytes(nv)
    e.set_input_nv12(nv.height, nv.width, nv.row_pitch, nv.uv)
    e.reset()
    e.forward_u8(surf, 0, ref)
    cases.run_error_cases(e, MEM, "nv12", surf.ctypes.data, ref.view(np.uint32).copy(), H, W)
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized") as err:
        fresh.set_input_view(view)
    assert "tdnet_set_input_view" in str(err.value)
    fresh.close()
    e.close()


def test_rgb24_still_fits_where_the_32_bit_formats_downscale_limit_is_passed(lib):
    """2 x 8000 -> 33 x 65: 8000 columns of 3 bytes fit one strip's LDS, of 4 bytes they do not; the message states the 32-bit figure."""
    e = _engine(lib)
    e.set_input_view(SourceView(PIX_RGB24, 2, 8000))
    with pytest.raises(_capi.TdnetError, match="30x") as err:
        e.set_input_view(SourceView(cases.PACKED[2], 2, 8000))
    assert "tdnet_set_input_view" in str(err.value)
    e.close()


def test_model_classes_check_the_frame_tensor_before_an_engine_exists():
    import torch
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    view = cases.packed_view(cases.PACKED[3], (3, 7, 41, 83))
    n = cases.view_extent(view)
    ok = torch.zeros(1, n, dtype=torch.uint8)
    calls = [lambda t, v: m.forward_u8(t, 0, (33, 65), view=v), lambda t, v: m.forward_labels_u8(t, 0, (33, 65), view=v),
             lambda t, v: m.encode_u8(t, 0, (33, 65), view=v), lambda t, v: m.forward_rgb_u8(t, 0, (33, 65), (8, 16), view=v),
             lambda t, v: m.forward_score_u8(t, torch.zeros(1, 33, 65, dtype=torch.uint8), 0, (33, 65), view=v),
             lambda t, v: m.forward_labels_conf_u8(t, 0, (33, 65), view=v), lambda t, v: m.forward_overlay_u8(t, 0, (33, 65), view=v)]
    for call in calls:
        with pytest.raises(RuntimeError, match="uint8"):                # dtype
            call(torch.zeros(1, n), view)
        with pytest.raises(RuntimeError, match="N,nbytes"):             # rank
            call(torch.zeros(1, 50, 365, dtype=torch.uint8), view)
        with pytest.raises(RuntimeError, match="CONTIGUOUS"):
            call(torch.zeros(n, 2, dtype=torch.uint8).t()[:1], view)
        with pytest.raises(RuntimeError, match="below"):                # nbytes >= view_extent
            call(ok[:, :n - 1], view)
        with pytest.raises(RuntimeError, match="rectangle"):
            call(ok, cases.packed_view(cases.PACKED[3], (10, 7, 41, 83)))
        with pytest.raises(RuntimeError, match="pitch"):
            call(ok, SourceView(cases.PACKED[3], 50, 90, pitch=359))
        with pytest.raises(RuntimeError, match="SourceView"):
            call(ok, (3, 7, 41, 83))
        with pytest.raises(_capi.TdnetError):                           # no CPU fallback
            call(ok, view)
    assert m.engine is None                                            # nothing was built on the way
