"""tests/ppm_fold_cases.py on the device: the pyramid folded through the Encoding's first 1x1 convs (tdnet_opts.fusion bit 2097152) -- the operator
entry inside guard bands, the two-source kernel forms with a null second source, whole clips with the bit on and off, two handles on one weight block.

enc_first on an MI355X (the emulator gives the same digits): the fold's error against fp64 as a multiple of the z route's own, max / rms over v_cur, q1 and
k1 together (gate x2 / x1.25), pid 0 | pid 1:
    5x9    x0.65 / x0.67 | x0.73 / x0.69        9x17   x0.61 / x0.72 | x0.63 / x0.69
    1x7    x0.46 / x0.69 | x0.67 / x0.69        33x40  x0.69 / x0.73 | x0.73 / x0.74        5x9 at C = 2048, pid 1: x0.87 / x0.69
The largest single-output figure is q1's max at 5x9, pid 1: x1.09.  Whole frames at 33x65, bit on against bit off: max |dlogit| 4.0e-5 (td4), 3.8e-6 (td2)."""
import pytest
import torch

import opcheck
import ppm_fold_cases as cases
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()                      # the in-tree libtdnet_hip_test.so; raises if it is missing


@pytest.fixture()
def mem():
    return opcheck.GuardedTorchMem()


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
    cases.frames(lib, opcheck.TorchMem(), golden_dir, name, bb)


def test_two_handles_on_one_weight_block(lib):
    cases.shared(lib, opcheck.TorchMem())
