"""CPU tier: the RGB head's folded MFMA form (csrc/head_mfma.hpp: a 2 x 4 block of output pixels x 3 channels in the MFMA's N) under the
fiber emulator, through tsnet_op_head: fold indexing, reflection at the borders, ragged frames, tile heights, batch independence."""
import pytest

import head_mfma_cases as hc
import op_cases as oc

TOL = 2e-5     # the head's operator tolerance in this tier (tests/test_emu_ops.py)


@pytest.mark.parametrize("composite", [False, True])
@pytest.mark.parametrize("N,H,W", hc.SHAPES)
@pytest.mark.parametrize("C", [16, 64])
def test_folded_head_shapes(emu_lib, C, N, H, W, composite):
    assert oc.head_case(emu_lib, "cpu", N, H, W, C, composite=composite) < TOL


@pytest.mark.parametrize("N,H,W", hc.RAGGED)
def test_folded_head_tile_rows_give_the_same_bits(emu_lib, N, H, W):
    """rows 8 / 16 / 32 / the launcher's choice at C = 64: a pixel's chains do not depend on the tile it sits in"""
    assert hc.rows_give_equal_bits(emu_lib, "cpu", N, H, W)


@pytest.mark.parametrize("H,W", [(9, 7), (10, 12)])
def test_folded_head_batch_gives_the_same_bits(emu_lib, H, W):
    assert hc.batch_gives_equal_bits(emu_lib, "cpu", H, W)


@pytest.mark.parametrize("H,W", [(9, 7), (12, 16)])
@pytest.mark.parametrize("o,c,ky,kx", hc.ONE_HOT)
def test_folded_head_one_hot_filters(emu_lib, H, W, o, c, ky, kx):
    """tanh of the shifted, reflected input plus bias: any indexing error of the fold or at the borders shows"""
    assert hc.one_hot_case(emu_lib, "cpu", H, W, o, c, ky, kx) < TOL


@pytest.mark.parametrize("N,H,W", hc.SHAPES)
def test_folded_head_against_fp64(emu_lib, N, H, W, capsys):
    """the folded head's error against an fp64 evaluation beside that of PyTorch's fp32 CPU evaluation (printed: profiles/head_mfma.txt);
    the folded head stays inside the operator tolerance of the exact result"""
    for C in (16, 64):
        e, e32 = hc.fp64_errors(emu_lib, "cpu", N, H, W, C)
        with capsys.disabled():
            print(f"\n[head_mfma emu] N={N} H={H} W={W} C={C}: folded head vs fp64 {e:.3e}   torch fp32 CPU vs fp64 {e32:.3e}", end="")
        assert e < TOL
