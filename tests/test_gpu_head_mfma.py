"""GPU tier: the RGB head's folded MFMA form (csrc/head_mfma.hpp) on the MI355X, through tsnet_op_head: the cases of
tests/test_emu_head_mfma.py on the real matrix pipe."""
import pytest
import torch

import head_mfma_cases as hc
import op_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-5     # the head's operator tolerance in this tier (tests/test_gpu_ops.py)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from wacv23_tsnet_amd import _lib
    return _lib.load()       # raises if the HIP extension is missing: no fallback


@pytest.mark.parametrize("composite", [False, True])
@pytest.mark.parametrize("N,H,W", hc.SHAPES)
@pytest.mark.parametrize("C", [16, 64])
def test_folded_head_shapes(lib, C, N, H, W, composite):
    assert oc.head_case(lib, DEV, N, H, W, C, composite=composite) < TOL


@pytest.mark.parametrize("N,H,W", hc.RAGGED)
def test_folded_head_tile_rows_give_the_same_bits(lib, N, H, W):
    assert hc.rows_give_equal_bits(lib, DEV, N, H, W)


@pytest.mark.parametrize("H,W", [(9, 7), (10, 12)])
def test_folded_head_batch_gives_the_same_bits(lib, H, W):
    assert hc.batch_gives_equal_bits(lib, DEV, H, W)


@pytest.mark.parametrize("H,W", [(9, 7), (12, 16)])
@pytest.mark.parametrize("o,c,ky,kx", hc.ONE_HOT)
def test_folded_head_one_hot_filters(lib, H, W, o, c, ky, kx):
    assert hc.one_hot_case(lib, DEV, H, W, o, c, ky, kx) < TOL


@pytest.mark.parametrize("N,H,W", hc.SHAPES)
def test_folded_head_against_fp64(lib, N, H, W, capsys):
    """printed for profiles/head_mfma.txt: the folded head's error against fp64 beside that of PyTorch's fp32 CPU evaluation"""
    for C in (16, 64):
        e, e32 = hc.fp64_errors(lib, DEV, N, H, W, C)
        with capsys.disabled():
            print(f"\n[head_mfma gpu] N={N} H={H} W={W} C={C}: folded head vs fp64 {e:.3e}   torch fp32 CPU vs fp64 {e32:.3e}", end="")
        assert e < TOL
