"""CPU tier: one slot table for every forward (one_table_cases.py).  The kernels that read the encoded sources lost their cache forms; the
one-shot forward, both clip modes and every spelling of the operator entry points now run the slot form on a table the engine writes.  The
change moved addresses, not arithmetic: every case gives the BITS the commit before gave (tests/golden/one_table_parent_bits*.npz, recorded
by tools/probes/one_table_capture_bits.py), and an engine driven through every mode in turn never reads a table left by an earlier forward."""
import pytest
import torch

import one_table_cases as tc


@pytest.fixture(scope="module")
def golden():
    return tc.load_golden()


def _check(golden, prefix, got):
    want = {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want) and want                               # none of the recorded cases is left out
    for name, y in got.items():
        assert y.shape == want[name].shape and torch.equal(y, want[name]), (name, float((y - want[name]).abs().max()))


def test_forwards_keep_the_bits_of_the_parent(emu_lib, golden):
    _check(golden, "forward.", tc.forward_outputs(emu_lib))


def test_operator_spellings_keep_the_bits_of_the_parent(emu_lib, golden):
    _check(golden, "op.", tc.op_outputs(emu_lib))


def test_record_holds_nothing_else(golden):
    assert all(k.startswith(("forward.", "op.")) for k in golden)


def test_no_stale_table(emu_lib):
    """one engine through every mode in turn, with tables of different content and length, and the same table twice"""
    tc.check_stale_table(tc.Net(), emu_lib)
