"""tests/fp16_chain_cases.py on the device: every stage of a tdnet_opts.precision = 1 frame behind c4 against the rounding-aware oracle
applied to the handle's own previous stage; the sizes tests/test_emu_fp16_chain.py proves under the emulator, and one at which layer4's
convs run on the LDS-DMA kernels (fp16_chain_cases.DEVICE_CASE)."""
import pytest
import torch

import fp16_chain_cases as cases
import opcheck
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: "%s-%s-%dx%d" % (c[0], c[2], c[3], c[4]))
def test_fp16_stage_chain(lib, case):
    cases.run_case(lib, opcheck.TorchMem(), case)


def test_fp16_stage_chain_with_layer4_on_the_lds_dma_kernels(lib):
    cases.run_case(lib, opcheck.TorchMem(), cases.DEVICE_CASE, checked=(3,))
