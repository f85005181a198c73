"""Destination views (include/tdnet.h "destination views") on the CPU through the kernel emulator: the operator cases of tests/dst_view_cases.py
against the host oracle, whole frames with a destination view against a twin handle without one, and the error paths.  A write outside the rectangle
shows here as a changed prefill or guard byte (or a host fault).  Every comparison is exact."""
import numpy as np
import pytest

import dst_view_cases as cases
import emu_util
from tdnet_amd import _capi, arch, weights
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


@pytest.mark.parametrize("tag,fmt,layout,standard", cases.DESTS, ids=cases.DEST_IDS)
def test_pictures_into_every_destination_form(lib, tag, fmt, layout, standard):
    cases.run_dest_case(lib, MEM, fmt, layout, standard)


@pytest.mark.parametrize("frame,rect", cases.EDGES, ids=cases.EDGE_IDS)
def test_edge_rectangles(lib, frame, rect):
    cases.run_edge_case(lib, MEM, frame, rect)


def _engine(lib, H=33, W=65):
    spec = arch.model_spec("td2", 19, "resnet18")
    e = Engine(2, 18, 19, H, W, 0, lib=lib)
    e.load_state_dict(weights.synth_state_dict(spec, arch.feat_size(H), arch.feat_size(W), 0))
    return e


def test_frames_with_a_destination_view_equal_write_view_of_the_twins_pictures(lib):
    a = _engine(lib, *cases.NET)
    cases.run_frame_scenario(a, MEM, cases.FRAME_DESTS[::2])           # a 4-byte and the NV12 destination: an emulated frame takes seconds
    a.close()


def test_errors_leave_the_configuration_the_fifo_and_a_pending_frame_alone(lib):
    H, W = cases.NET
    e = _engine(lib, H, W)
    with pytest.raises(_capi.TdnetError, match="reserved"):            # a rejected configuration configures nothing
        e.lib.check(e.lib.tdnet_set_output_view(e.h, next(t for m, t in cases.bad_dst_views() if m == "reserved")))
    e.set_input_view(cases.SRC_VIEW)
    e.set_output_overlay(cases.vc.overlay_palette())
    e.set_output_rgb(41, 83, cases.PAL3)
    e.set_output_view(cases.FRAME_DESTS[0])
    holder, ptr = MEM.up(cases.vc.view_bytes(cases.SRC_VIEW, 0x5A, 3), 1)
    cases.run_error_cases(e, MEM, ptr, H, W)
    fresh = Engine(2, 18, 19, H, W, 0, lib=lib)
    with pytest.raises(_capi.TdnetError, match="not finalized") as err:
        fresh.set_output_view(cases.FRAME_DESTS[0])
    assert "tdnet_set_output_view" in str(err.value)
    fresh.close()
    e.close()


def test_model_classes_check_the_destination_tensor_before_an_engine_exists():
    import torch
    from tdnet_amd.dataloader import PIX_NV12, PIX_RGBA32, SourceView, view_extent
    from tdnet_amd.model import td2_psp50
    m = td2_psp50.td2_psp50(nclass=19, path_num=2, model_path=None, backbone="resnet18", synthetic_seed=0).eval()
    dv = cases.FRAME_DESTS[0]
    n = view_extent(dv)
    img, ok = torch.zeros(1, 41, 83, 3, dtype=torch.uint8), torch.zeros(1, n, dtype=torch.uint8)
    calls = [lambda v, o: m.forward_overlay_u8(img, 0, (33, 65), out_view=v, out=o), lambda v, o: m.forward_rgb_u8(img, 0, (33, 65), (41, 83), out_view=v, out=o)]
    for call in calls:
        with pytest.raises(RuntimeError, match="uint8"):                # dtype
            call(dv, torch.zeros(1, n))
        with pytest.raises(RuntimeError, match="N,nbytes"):             # rank, batch
            call(dv, torch.zeros(1, 50, 389, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="N,nbytes"):
            call(dv, torch.zeros(2, n, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="CONTIGUOUS"):
            call(dv, torch.zeros(n, 2, dtype=torch.uint8).t()[:1])
        with pytest.raises(RuntimeError, match="below"):                # nbytes >= view_extent
            call(dv, ok[:, :n - 1])
        with pytest.raises(RuntimeError, match="not inside"):
            call(cases.dest_view(PIX_RGBA32, rect=(10, 6, 41, 83)), ok)
        with pytest.raises(RuntimeError, match="nothing is resized"):   # the rectangle is not the picture's size
            call(cases.dest_view(PIX_RGBA32, rect=(2, 6, 40, 83)), ok)
        with pytest.raises(RuntimeError, match="pitch"):
            call(SourceView(PIX_RGBA32, 50, 96, pitch=383, crop=cases.RECT), ok)
        with pytest.raises(RuntimeError, match="even"):
            call(SourceView(PIX_NV12, 50, 96, crop=(3, 6, 41, 83)), ok)
        with pytest.raises(RuntimeError, match="SourceView"):
            call(cases.RECT, ok)
        with pytest.raises(_capi.TdnetError):                           # no CPU fallback
            call(dv, ok)
    assert m.engine is None                                            # nothing was built on the way
