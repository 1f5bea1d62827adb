"""GPU tier of test_emu_epilogue_parent_bits.py: the cases of epilogue_bits_cases.py on the MI355X, every word -- y, every fp64 partial, alpha,
beta, amax_out -- equal to what the commit before gave ON THE DEVICE (tests/golden/epilogue_parent_bits_gpu*.npz, recorded by
tools/probes/epilogue_capture_bits.py --gpu with that commit's libtsnet_hip.so).  The emulator's record cannot serve here: the hardware's MFMA
sums a k-step in an order of its own, and the parent's library itself differs from that record in most words of y.  The kernels fix every
order they control (chains, fold points, the statistics' association, the finalize fold), so the device's bits repeat from run to run."""
import pytest
import torch

import epilogue_bits_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from wacv23_tsnet_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    rec = bc.load_golden(gpu=True)
    assert sorted({k.split("/", 1)[0] for k in rec}) == sorted(bc.NAMES), sorted(rec)
    return rec


@pytest.mark.parametrize("case", bc.CASES, ids=bc.NAMES)
def test_epilogue_bits_of_the_parent(lib, golden, case):
    keys = bc.check_case(lib, DEV, case, golden)
    print(f"{case[0]}: {' '.join(keys)} equal to the parent's")
