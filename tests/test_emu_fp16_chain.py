"""tests/fp16_chain_cases.py through the test-only emulator: every stage of a tdnet_opts.precision = 1 frame behind c4 against the
rounding-aware oracle applied to the handle's own previous stage.  CPU only; tests/test_gpu_fp16_chain.py runs the same on the device."""
import pytest

import emu_util
import fp16_chain_cases as cases
import opcheck


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: "%s-%s-%dx%d" % (c[0], c[2], c[3], c[4]))
def test_fp16_stage_chain(lib, case):
    cases.run_case(lib, opcheck.NumpyMem(), case)
