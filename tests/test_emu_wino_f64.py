"""tests/wino_f64_cases.py through the test-only fiber emulator (tests/emu/): the fused Winograd F(4x4) kernel of the 64 -> 64 3x3 convs
(k_wino4_f64, tdnet_opts.fusion bit 4194304) -- its index math proven here before tests/test_gpu_wino_f64.py runs the same cases on the device.  CPU only."""
import pytest

import emu_util
import opcheck
import wino_f64_cases as cases


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


@pytest.fixture()
def mem():
    return opcheck.GuardedNumpyMem()


@pytest.mark.parametrize("resid,act", cases.VARIANTS)
@pytest.mark.parametrize("hw", cases.MAPS, ids=lambda hw: "%dx%d" % hw)
def test_fused_kernel_against_fp64_and_the_unfused_route(lib, mem, hw, resid, act):
    cases.conv(lib, mem, hw[0], hw[1], resid, act)


@pytest.mark.parametrize("shape", cases.REFUSED, ids=lambda s: "%d-%d-k%d-s%d-d%d-a%d" % s)
def test_entry_refuses_what_the_route_does_not_take(lib, mem, shape):
    cases.refused(lib, mem, shape)


def test_entry_refuses_a_map_past_the_32_bit_offsets(lib, mem):
    cases.refused_size(lib, mem)


def test_small_maps_keep_the_direct_kernel(lib, mem):
    cases.plan_keeps_small_maps(lib, mem)
