"""The output stage's forms against each other (tests/out_cases.py) on the MI355X: int32 labels, uint8 labels, the score entry, the confidence
entry in both pass forms and the colour map, from the same low-resolution logits in device memory, bit for bit."""
import numpy as np
import pytest
import torch

import opcheck
import out_cases as cases
from tdnet_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return _capi.test_lib()


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
    def put_logits(a, poison):
        """(the guarded mem that owns it -- verify() checks the bands --, address) of fp32 logits between guard bands of the fill `poison`"""
        mem = opcheck.GuardedTorchMem()
        t = mem.put(a, poison=poison)
        return mem, t.data_ptr()

    @staticmethod
    def get(keep):
        return keep.cpu().numpy().view(np.uint64)

    @staticmethod
    def holder(nbytes, off):
        hold = torch.full((nbytes + cases.GUARD,), 0xEE, dtype=torch.uint8, device="cuda")

        def read():
            host = hold.cpu().numpy()
            assert (host[:off] == 0xEE).all() and (host[off + nbytes:] == 0xEE).all(), off
            return host[off:off + nbytes].copy()
        return hold.data_ptr() + off, read


@pytest.mark.parametrize("field", cases.FIELDS)
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_every_output_form_names_the_same_labels(lib, case, field, monkeypatch):
    cases.check(lib, DeviceMem(), monkeypatch.setenv, case, field)
