"""GPU tier: the kernels of csrc/train_extras.hpp one operator at a time on the device, the cases of tests/train_extras_cases.py
(tests/test_train_extras_ops.py runs them under the emulator), plus what only the device can show: the patch warp's grid-stride loop taking a
second trip, and the engine's extras against the two operators at the face golden's shape."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_extras_cases as tc
from test_train_extras_ops import _assert_tail

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from wacv23_tsnet_amd import _lib
    return _lib.load()       # raises if the HIP extension is missing: no fallback


@pytest.mark.parametrize("case", list(tc.EXACT_CASES))
def test_patch_warp_moves_whole_patches_exactly(lib, case):
    """identity, a permutation on a non-square map, grid -1 / +1 (1/2, 1/4 in the corners), a whole cell outside (0): EQUAL to patches of
    src / div moved whole"""
    K, B, h, w, down, divs, coords = tc.EXACT_CASES[case]
    out, exp, ref64, ref32 = tc.exact_patch_warp_case(lib, DEV, K, B, h, w, down, divs, coords(K * B, h, w))
    assert torch.equal(ref64, exp) and torch.equal(ref32, exp)
    assert torch.equal(out, exp), (out - exp).abs().max().item()


@pytest.mark.parametrize("case", list(tc.PATCH_WARP_SHAPES) + ["big"])
def test_patch_warp_random_flows(lib, case):
    """flows in [-1.3, 1.3) and half-cell flows at the smallest extents, and K = 3, B = 3 at 256 x 256 on a 32 x 32 map (589 824 pixels: the
    grid-stride loop's second trip, one launch): max|d| against the fp64 chain at most 4 x that of torch's fp32 chain on the same case.
    Measured on an MI355X, max|d| of the kernel = that of torch's fp32 chain to three digits: the emulator's figures on the small cases
    (6.71e-8 .. 2.53e-7, tests/test_train_extras_ops.py), big 1.33e-7 (bounds: 4 x these)."""
    e, e32, rmax = tc.toleranced_patch_warp_case(lib, DEV, *(tc.PATCH_WARP_BIG if case == "big" else tc.PATCH_WARP_SHAPES[case]))
    print(f"patch warp {case}: kernel {e:.2e}, torch fp32 {e32:.2e}, of max|ref| {rmax:.2f}")
    assert e <= tc.PATCH_WARP_MARGIN * e32


def test_patch_warp_refusals(lib):
    n, msgs = tc.patch_warp_refusals(lib, DEV)
    assert n >= 12 and len(msgs) >= 4


@pytest.mark.parametrize("case", list(tc.TAIL_CASES))
def test_tail_statistics_image_and_loss_warp(lib, case):
    """statistics EQUAL to fp32(two-pass fp64) (1 ulp on the mean-heavy std), the image EQUAL to torch's fp32 chain with the returned
    statistics, the composite's columns EQUAL bg, loss_warp within 2 ulp of the kernel's arithmetic and 4 x torch's fp32 distance + 2 ulp of
    fp64 (tests/test_train_extras_ops.py states the rules)."""
    K, B, H, W, kind, fore, bg = tc.TAIL_CASES[case]
    _assert_tail(tc.tail_case(lib, DEV, K, B, H, W, kind, fore, bg), B, W, kind, fore, bg)


@pytest.mark.parametrize("C", tc.COS_C)
@pytest.mark.parametrize("rows", tc.COS_ROWS)
def test_loss_align(lib, rows, C):
    """|loss_align - fp64| within (8 ceil(C / 256) + 20) 2^-24 with planted rows among the random ones"""
    err, _, loss = tc.cos_case(lib, DEV, rows, C)
    print(f"loss_align rows={rows} C={C}: {loss:.9g}, |d| {err:.2e} (bound {tc.cos_bound(C):.2e})")
    assert err <= tc.cos_bound(C)


def test_loss_align_planted_rows_only(lib):
    err, cs, loss = tc.cos_case(lib, DEV, 10, 64, only_planted=True)
    assert torch.allclose(cs, torch.tensor([0.0, 0.0, 0.1, 1.0, -1.0] * 2, dtype=torch.float64), atol=1e-12)
    assert err <= tc.cos_bound(64) and abs(loss - 0.98) <= 1e-6


def test_tail_refusals(lib):
    assert tc.tail_refusals(lib, DEV) >= 10


def test_engine_runs_the_operators_launches():
    """the face golden's configuration (256 x 256, K = 2): tsnet_train_extras after a forward EQUALS tsnet_op_patch_warp + tsnet_op_train_tail
    on the forward's flows and pg / sg -- images and both losses"""
    import helpers as Hh
    from oracle import tsnet_oracle as O
    meta, _, cfg, sd, inp = Hh.golden_case("g5_train_extras_256_k2")
    tar_img = O.synth_inputs(cfg, meta["B"], 256, 256, seed=meta["iseed"] + 1000, mask_mode="box")[0][0]
    eng = Hh.make_engine(cfg, sd, 256, 256, meta["B"], DEV)
    (img_a, loss_a), (img_b, loss_b) = tc.engine_tie_case(eng, inp, tar_img, DEV)
    eng.close()
    assert torch.equal(img_a, img_b) and torch.equal(loss_a, loss_b)
