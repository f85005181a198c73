"""tests/label_ref_cases.py on the MI355X: tdnet_op_upsample and tdnet_op_upsample_argmax against the independent fp64 evaluation of
tests/out_ref.py, the logits in device memory inside guard bands of both fills; also on rows wider than one workgroup's strip and at the
reference's native 769x1537."""
import pytest
import torch

import label_ref_cases as cases
import opcheck
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


class DeviceMem(opcheck.GuardedTorchMem):
    def holder(self, nbytes, off):
        g = cases.GUARD
        hold = torch.full((nbytes + 2 * g,), 0xEE, dtype=torch.uint8, device="cuda")

        def read():
            host = hold.cpu().numpy()
            assert (host[:g + off] == 0xEE).all() and (host[g + off + nbytes:] == 0xEE).all(), off
            return host[g + off:g + off + nbytes].copy()
        return hold.data_ptr() + g + off, read


@pytest.mark.parametrize("case", cases.CASES + cases.GPU_ONLY_CASES, ids=cases.case_id)
def test_upsample_and_labels_against_the_independent_reference(lib, case):
    cases.check(lib, DeviceMem(), case)
