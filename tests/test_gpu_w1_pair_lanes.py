"""conv_w1's producers, one lane = two adjacent column pairs (csrc/conv_w1.hpp w1_item_*), on the GPU: the cases of w1_pair_cases against
fp64 under the fp32-class line, equal bits between chunk sizes -- chunk 1 runs the one-tile kernel (conv_w1_one.hpp), 2 and 3 the chunk
kernel, so that is also the two kernels against each other.  (GPU bits are not compared with the emulator's record: the MFMA's internal
order is the hardware's.)"""
import pytest
import torch

import op_cases as oc
import w1_pair_cases as wc
from test_gpu_ops import REL

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from wacv23_tsnet_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("case", wc.CASES, ids=[c[0] for c in wc.CASES])
def test_w1_pair_lanes(lib, case):
    name, args, kw, chunks, line = case
    ys = wc.outputs(oc, lib, DEV, name, args, kw, chunks)
    for c in chunks[1:]:
        assert torch.equal(ys[chunks[0]], ys[c]), (name, chunks[0], c, float((ys[chunks[0]] - ys[c]).abs().max()))
    for c in chunks:
        err = oc.conv_w1_case(lib, DEV, *args, chunk=c, **kw)
        print(f"{name} chunk {c}: rel err vs fp64 {err:.3e}")
        assert err < (REL if line is None else line), (name, c, err)
