"""GPU tier of test_emu_conv_epilogue.py: the cases of epilogue_cases.py on the MI355X, where workgroups really arrive concurrently, plus one
case for the in-kernel finalize hand-off under many concurrent arrivals."""
import pytest
import torch

import epilogue_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from wacv23_tsnet_amd import _lib
    return _lib.load()


def test_every_kernel_family_has_a_row():
    ec.check_all_families_occur()


@pytest.mark.parametrize("name", ec.STAT_ROWS)
def test_partials_alpha_beta_amax_every_word(lib, name):
    ec.check_stats(lib, DEV, name)


@pytest.mark.parametrize("name,add_nmod", ec.ADDEND_CASES, ids=[f"{n}-nmod{m}" for n, m in ec.ADDEND_CASES])
def test_addend_is_one_fp32_addition(lib, name, add_nmod):
    ec.check_addend(lib, DEV, name, add_nmod)


@pytest.mark.parametrize("name", ec.BF16_ROWS)
def test_bf16_storage_is_rne_of_the_fp32_values(lib, name):
    ec.check_bf16_storage(lib, DEV, name)


@pytest.mark.parametrize("pair", list(ec.AMAX_PAIRS))
@pytest.mark.parametrize("name,nprod", ec.IN_AMAX_CASES, ids=[f"{n}-nprod{p}" for n, p in ec.IN_AMAX_CASES])
def test_device_scale_from_in_amax_matches_the_host_bound(lib, name, nprod, pair):
    ec.check_in_amax(lib, DEV, name, nprod, pair)


def test_refusals_leave_every_output_untouched(lib):
    ec.check_refusals(lib, DEV)


@pytest.mark.parametrize("tile", ec.HANDOFF_TILES)
def test_in_kernel_finalize_under_concurrent_arrivals(lib, tile):
    """H2 16 -> 200 channels, 13 images of 32 x 64: 16 tiles per image, seven (tile 32) or two (tile 128) channel tiles with a ragged last one,
    neither count a multiple of the eight XCDs -- about 90 (tile 32: 91) concurrent (image, channel-tile) hand-offs, three launches back to back on
    NaN-primed partials with stats = 2.  It checks every word of the partials, alpha / beta and amax_out against one fp64 reduction of the returned
    y, and that the counters are left zero.  It cannot force an interleaving: a hand-off that is wrong only under an ordering the run did not
    take passes here.  No more than that."""
    ec.check_handoff(lib, DEV, tile)
