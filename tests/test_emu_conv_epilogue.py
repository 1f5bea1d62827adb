"""CPU tier: the convolutions' epilogue and operand hand-offs per kernel family (tsnet_op_conv2d_epi) on the emulation build -- the cases of
epilogue_cases.py.  The emulator runs workgroups one after another, so the arrival-counter route is checked here for its indexing, its counts and
its fold, not for visibility between workgroups: that is the GPU tier's (test_gpu_conv_epilogue.py), which adds the 13-image hand-off case."""
import pytest

import epilogue_cases as ec


def test_every_kernel_family_has_a_row():
    ec.check_all_families_occur()


@pytest.mark.parametrize("name", ec.STAT_ROWS)
def test_partials_alpha_beta_amax_every_word(emu_lib, name):
    ec.check_stats(emu_lib, "cpu", name)


@pytest.mark.parametrize("name,add_nmod", ec.ADDEND_CASES, ids=[f"{n}-nmod{m}" for n, m in ec.ADDEND_CASES])
def test_addend_is_one_fp32_addition(emu_lib, name, add_nmod):
    ec.check_addend(emu_lib, "cpu", name, add_nmod)


@pytest.mark.parametrize("name", ec.BF16_ROWS)
def test_bf16_storage_is_rne_of_the_fp32_values(emu_lib, name):
    ec.check_bf16_storage(emu_lib, "cpu", name)


@pytest.mark.parametrize("pair", list(ec.AMAX_PAIRS))
@pytest.mark.parametrize("name,nprod", ec.IN_AMAX_CASES, ids=[f"{n}-nprod{p}" for n, p in ec.IN_AMAX_CASES])
def test_device_scale_from_in_amax_matches_the_host_bound(emu_lib, name, nprod, pair):
    ec.check_in_amax(emu_lib, "cpu", name, nprod, pair)


def test_refusals_leave_every_output_untouched(emu_lib):
    ec.check_refusals(emu_lib, "cpu")
