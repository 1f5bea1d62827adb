"""GPU tier of test_emu_upconv.py: the cases of upconv_cases.py on the MI355X -- the fused up-convolution and upsample2x + convolution give the
same bits, and both match the fp64 reference."""
import pytest
import torch

import upconv_cases as uc

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 1e-6     # test_gpu_ops.REL: the patch kernel's error relative to max|fp64 reference|


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from wacv23_tsnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", uc.CASES, ids=[c[0] for c in uc.CASES])
def test_fused_upconv_matches_two_launches_and_reference(lib, case):
    uc.check_case(lib, DEV, case, REL)


def test_upconv_refusals_leave_the_output_untouched(lib):
    uc.check_refusals(lib, DEV)
