"""tests/label_ref_cases.py on the CPU through the kernel emulator: tdnet_op_upsample and tdnet_op_upsample_argmax against the independent
fp64 evaluation of tests/out_ref.py, the logits inside guard bands of both fills; and out_ref itself against the reference's definition."""
import pytest

import emu_util
import label_ref_cases as cases


@pytest.fixture(scope="module")
def lib():
    return emu_util.emu_lib()


def test_up_ref_is_the_reference_definition():
    seen = cases.check_up_ref_definition()
    assert seen["odd_w-x1"][0] <= 1e-15                                # 4 / 32 and 8 / 64: representable scales, exact coordinates
    assert seen["wide-x1"][0] > 0                                      # 299 / 2050 is not: the fp32 coordinate shows, inside its bound


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_upsample_and_labels_against_the_independent_reference(lib, case):
    cases.check(lib, cases.HostMem(), case)
