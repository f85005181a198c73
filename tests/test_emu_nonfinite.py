"""tests/nonfinite_cases.py on the CPU through the kernel emulator: every case is proven here before tests/test_gpu_nonfinite.py runs it on
the device, whose instruction selection (v_maximum3_f32 for the propagating maximum, the MFMA's handling of NaN and inf) is what the
emulator cannot vouch for."""
import numpy as np
import pytest

import emu_util
import nonfinite_cases as cases
import opcheck
import out_cases


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


@pytest.fixture()
def mem():
    return opcheck.GuardedNumpyMem()


class HostMem:
    stream = None

    @staticmethod
    def put(a):
        a = np.array(a)
        return a, a.ctypes.data

    @staticmethod
    def holder(nbytes, off):
        hold = np.full(nbytes + out_cases.GUARD, 0xEE, np.uint8)

        def read():
            assert (hold[:off] == 0xEE).all() and (hold[off + nbytes:] == 0xEE).all(), off
            return hold[off:off + nbytes].copy()
        return hold.ctypes.data + off, read


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
    cases.labels(lib, HostMem, kind, monkeypatch.setenv)
