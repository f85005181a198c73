"""tests/nonfinite_cases.py on the MI355X: the max-pool bit for bit F.max_pool2d on maps with NaN, +/-inf and values below -3e38; one NaN / one
+inf input element and a -inf bias through every conv route, the fused Winograd kernel, the head conv with its classifier and the stem;
fp16 storage beyond 65504; the label entries under +/-inf and NaN logits.  Every case is proven under the emulator first
(tests/test_emu_nonfinite.py); what the device adds is its own instruction selection -- v_maximum3_f32, the MFMAs' NaN and inf handling, the
hardware fp16 converts."""
import numpy as np
import pytest
import torch

import nonfinite_cases as cases
import opcheck
import out_cases
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


@pytest.fixture()
def mem():
    return opcheck.GuardedTorchMem()


class DeviceMem:
    @property
    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    @staticmethod
    def put(a):
        a = np.array(a)
        t = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
        return t, t.data_ptr()

    @staticmethod
    def holder(nbytes, off):
        hold = torch.full((nbytes + out_cases.GUARD,), 0xEE, dtype=torch.uint8, device="cuda")

        def read():
            host = hold.cpu().numpy()
            assert (host[:off] == 0xEE).all() and (host[off + nbytes:] == 0xEE).all(), off
            return host[off:off + nbytes].copy()
        return hold.data_ptr() + off, read


@pytest.mark.parametrize("mode", cases.MAXPOOL_MODES)
@pytest.mark.parametrize("hw", cases.MAXPOOL_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_maxpool_is_the_reference_bit_for_bit(lib, mem, hw, mode):
    cases.maxpool(lib, mem, hw, mode)


@pytest.mark.parametrize("kind", cases.INPUT_KINDS)
@pytest.mark.parametrize("route", cases.CONV_ROUTES, ids=cases.route_id)
def test_conv_epilogues_propagate_like_the_reference(lib, mem, route, kind):
    cases.conv(lib, mem, route, kind)


@pytest.mark.parametrize("kind", cases.INPUT_KINDS)
def test_fused_winograd_kernel_propagates_like_the_reference(lib, mem, kind):
    cases.wino_f64(lib, mem, kind)


@pytest.mark.parametrize("kind", cases.INPUT_KINDS)
@pytest.mark.parametrize("opts", cases.HEAD_OPTS, ids=lambda o: "p%d" % o.get("precision", 0))
def test_head_conv_with_the_classifier_propagates_like_the_reference(lib, mem, opts, kind):
    cases.head_cls(lib, mem, kind, opts)


@pytest.mark.parametrize("kind", cases.INPUT_KINDS)
@pytest.mark.parametrize("opts", cases.STEM_OPTS, ids=lambda o: "p%d" % o.get("precision", 0))
def test_stem_propagates_like_the_reference(lib, mem, opts, kind):
    cases.stem(lib, mem, kind, opts)


@pytest.mark.parametrize("tile", cases.F16_TILES)
def test_fp16_storage_overflows_to_the_reference_infinities(lib, mem, tile):
    cases.f16_conv(lib, mem, tile)


def test_fp16_stem_overflows_to_the_reference_infinities(lib, mem):
    cases.f16_stem(lib, mem)


@pytest.mark.parametrize("kind", cases.LABEL_KINDS)
def test_label_entries_under_non_finite_logits(lib, kind, monkeypatch):
    cases.labels(lib, DeviceMem(), kind, monkeypatch.setenv)
