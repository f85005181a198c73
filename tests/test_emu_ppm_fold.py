"""tests/ppm_fold_cases.py through the test-only fiber emulator (tests/emu/): the pyramid folded through the Encoding's first 1x1 convs
(tdnet_opts.fusion bit 2097152), proven here before tests/test_gpu_ppm_fold.py runs the same cases on the device.  CPU only."""
import pytest

import emu_util
import opcheck
import ppm_fold_cases as cases


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


@pytest.fixture()
def mem():
    return opcheck.GuardedNumpyMem()


@pytest.mark.parametrize("pid", [0, 1])
@pytest.mark.parametrize("hw", cases.ENC_SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_enc_first_fold_against_fp64(lib, mem, hw, pid):
    cases.enc_first(lib, mem, hw[0], hw[1], pid)


def test_enc_first_fold_resnet50_widths(lib, mem):
    h, w, C, DV = cases.ENC_WIDE
    cases.enc_first(lib, mem, h, w, 1, C=C, DV=DV)


@pytest.mark.parametrize("cap", cases.NULL_CAPS)
def test_null_second_source_gemm_is_bit_identical(lib, mem, cap):
    cases.src2_null_gemms(lib, mem, cap)


def test_null_second_source_direct_conv_is_bit_identical(lib, mem):
    cases.src2_null_direct(lib, mem)


@pytest.mark.parametrize("name,bb", cases.FRAME_MODELS)
def test_frames_with_and_without_the_fold(lib, golden_dir, name, bb):
    cases.frames(lib, opcheck.NumpyMem(), golden_dir, name, bb)


def test_two_handles_on_one_weight_block(lib):
    cases.shared(lib, opcheck.NumpyMem())
