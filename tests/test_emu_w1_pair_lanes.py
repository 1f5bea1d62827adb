"""conv_w1's producers, one lane = two adjacent column pairs (csrc/conv_w1.hpp w1_item_*), in the CPU emulation: the item shape, the lane
mapping and the LDS pads changed, the arithmetic per element did not -- every case of w1_pair_cases gives the BITS that the half-row items
of the commit before gave (tests/golden/w1_parent_bits*.npz, recorded by tools/probes/w1_capture_bits.py), in every chunk size, and stays
under the fp32-class line against fp64."""
import pytest
import torch

import op_cases as oc
import w1_pair_cases as wc
from test_emu_ops import REL


@pytest.fixture(scope="module")
def golden():
    rec = wc.load_golden()
    assert sorted(rec) == sorted(c[0] for c in wc.CASES), sorted(rec)
    return rec


@pytest.mark.parametrize("case", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_w1_pair_lanes_bits_of_the_parent(emu_lib, golden, case):
    name, args, kw, chunks, line = case
    ys = wc.outputs(oc, emu_lib, "cpu", name, args, kw, chunks)
    want = torch.from_numpy(golden[name])
    for c, y in ys.items():
        assert torch.equal(y, want), (name, c, float((y - want).abs().max()))          # (so the chunk sizes agree among themselves too)
    err = oc.conv_w1_case(emu_lib, "cpu", *args, chunk=chunks[-1], **kw)
    print(f"{name}: rel err vs fp64 {err:.3e}")
    assert err < (REL if line is None else line), (name, err)
