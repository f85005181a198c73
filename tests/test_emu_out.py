"""The output stage's forms against each other (tests/out_cases.py), on the CPU through the kernel emulator: int32 labels, uint8 labels, the score
entry, the confidence entry in both pass forms and the colour map, from the same low-resolution logits, bit for bit."""
import numpy as np
import pytest

import emu_util
import opcheck
import out_cases as cases


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


class HostMem:
    stream = None

    @staticmethod
    def put(a):
        a = np.array(a)                                                # a writable, contiguous copy
        return a, a.ctypes.data

    @staticmethod
    def put_logits(a, poison):
        """(the guarded mem that owns it -- verify() checks the bands --, address) of fp32 logits between guard bands of the fill `poison`"""
        mem = opcheck.GuardedNumpyMem()
        t = mem.put(a, poison=poison)
        return mem, t.ctypes.data

    @staticmethod
    def get(keep):
        return keep

    @staticmethod
    def holder(nbytes, off):
        hold = np.full(nbytes + cases.GUARD, 0xEE, np.uint8)

        def read():
            assert (hold[:off] == 0xEE).all() and (hold[off + nbytes:] == 0xEE).all(), off
            return hold[off:off + nbytes].copy()
        return hold.ctypes.data + off, read


@pytest.mark.parametrize("field", cases.FIELDS)
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_every_output_form_names_the_same_labels(lib, case, field, monkeypatch):
    cases.check(lib, HostMem, monkeypatch.setenv, case, field)
