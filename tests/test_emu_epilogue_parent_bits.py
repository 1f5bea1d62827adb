"""conv_epilogue's index arithmetic and the stem's staging (csrc/conv_common.hpp, conv_h2.hpp) in the CPU emulation: the row map is taken once
per row group, the output offsets are 32-bit, the addend's image comes from the tile and the stem folds its power-of-two scale into the split --
the values, their order of summation and the stores did not change.  Every case of epilogue_bits_cases gives the BITS that the commit before
gave (tests/golden/epilogue_parent_bits*.npz, recorded by tools/probes/epilogue_capture_bits.py): y, every fp64 partial, alpha, beta, amax_out."""
import pytest

import epilogue_bits_cases as bc


@pytest.fixture(scope="module")
def golden():
    rec = bc.load_golden()
    assert sorted({k.split("/", 1)[0] for k in rec}) == sorted(bc.NAMES), sorted(rec)
    return rec


def test_every_kernel_family_has_a_case():
    assert {c[1] for c in bc.CASES} == set(bc.ec.FAMILIES)


@pytest.mark.parametrize("case", bc.CASES, ids=bc.NAMES)
def test_epilogue_bits_of_the_parent(emu_lib, golden, case):
    keys = bc.check_case(emu_lib, "cpu", case, golden)
    print(f"{case[0]}: {' '.join(keys)} equal to the parent's")
