"""CPU tier: the four kernels of csrc/train_extras.hpp (and frame_stats_kernel as they use it) under the fiber emulator, one operator at a
time through tsnet_op_patch_warp / tsnet_op_train_tail, against exact references (tests/train_extras_cases.py).  tests/test_train_extras.py
reaches them only behind a whole forward, whose flows are smooth and never leave the map; tests/test_gpu_train_extras_ops.py runs the same
cases on the device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_extras_cases as tc

DEV = "cpu"


@pytest.mark.parametrize("case", list(tc.EXACT_CASES))
def test_patch_warp_moves_whole_patches_exactly(emu_lib, case):
    """flows on cell centres (identity; a permutation on a 4 x 8 map of a 16 x 32 image), on grid -1 / +1 (the zero padding carries 1/2; 1/4 in
    the corners) and a whole cell outside (0); B = 2, K = 2 with divisors (255, 1), every image different: the output EQUALS patches of
    src / div moved whole -- and so do torch's fp64 and fp32 chains"""
    K, B, h, w, down, divs, coords = tc.EXACT_CASES[case]
    out, exp, ref64, ref32 = tc.exact_patch_warp_case(emu_lib, DEV, K, B, h, w, down, divs, coords(K * B, h, w))
    assert torch.equal(ref64, exp) and torch.equal(ref32, exp)
    assert torch.equal(out, exp), (out - exp).abs().max().item()


@pytest.mark.parametrize("case", list(tc.PATCH_WARP_SHAPES))
def test_patch_warp_random_flows(emu_lib, case):
    """flows in [-1.3, 1.3) (zero padding with real weights) at down = 1, at K = 8 on a 2 x 2 map and on a 3 x 5 map, and half-cell flows (four
    weights of 1/4): max|d| against the fp64 unfold / grid_sample / fold chain at most 4 x that of torch's fp32 chain on the same case.
    Measured, max|d| of the kernel = that of torch's fp32 chain to three digits, under the emulator and on an MI355X alike: down1 8.33e-8,
    k8_2x2 1.04e-7, 3x5_k3 2.53e-7, 4x8_uniform 1.15e-7, 4x8_half_cells 6.71e-8 (bounds: 4 x these)."""
    e, e32, rmax = tc.toleranced_patch_warp_case(emu_lib, DEV, *tc.PATCH_WARP_SHAPES[case])
    print(f"patch warp {case}: kernel {e:.2e}, torch fp32 {e32:.2e}, of max|ref| {rmax:.2f}")
    assert e <= tc.PATCH_WARP_MARGIN * e32


def test_patch_warp_refusals(emu_lib):
    n, msgs = tc.patch_warp_refusals(emu_lib, DEV)
    assert n >= 12 and len(msgs) >= 4


@pytest.mark.parametrize("case", list(tc.TAIL_CASES))
def test_tail_statistics_image_and_loss_warp(emu_lib, case):
    """tsnet_op_train_tail in the pose form at H*W = 64, 960 and 4099 (uneven shares of the 16 blocks), K = 1, 2, 8, B = 3 with three different
    targets, the composite at W = 256, a mean-heavy frame.
    Statistics: EQUAL to fp32(two-pass fp64 mean / unbiased std); on the mean-heavy frame (0.8 + 1e-3 N(0,1)) the std may differ by 1 ulp.
    Image: EQUAL to torch's fp32 ((x - gm) / gs) * rs + rm with the returned statistics, frame n on target n % B; background columns EQUAL bg.
    loss_warp: within 2 fp32 ulp of the kernel's own arithmetic on the expected image, and within 4 x torch's fp32 F.l1_loss distance from
    the fp64 value + 2 ulp.  Measured, the same under the emulator and on an MI355X: 0 ulp from the kernel's arithmetic in every case;
    |kernel - fp64| (torch fp32 - fp64): k1_hw64 7.07e-8 (4.85e-8), k8_hw960 6.43e-7 (6.43e-7), k2_b3_hw4099 1.72e-8 (2.21e-7), composite
    4.05e-7 (7.22e-8; 2 ulp of 5.87 are 9.5e-7), mean_heavy 5.62e-8 (5.62e-8); the mean-heavy std came out equal."""
    K, B, H, W, kind, fore, bg = tc.TAIL_CASES[case]
    t = tc.tail_case(emu_lib, DEV, K, B, H, W, kind, fore, bg)
    _assert_tail(t, B, W, kind, fore, bg)


def _assert_tail(t, B, W, kind, fore, bg):
    r = t["r"]
    assert torch.equal(r["ref_mean"], t["ref_mean"]) and torch.equal(r["ref_std"], t["ref_std"])
    assert torch.equal(r["gen_mean"], t["gen_mean"])
    if kind == "mean_heavy":
        assert tc.ulps_apart(r["gen_std"], t["gen_std"]) <= 1
    else:
        assert torch.equal(r["gen_std"], t["gen_std"])
    assert torch.equal(r["x"], t["exp"]), (r["x"] - t["exp"]).abs().max().item()
    if fore[1] > fore[0]:
        img = r["x"].view(r["x"].shape[0], 3, -1, W)
        for c in range(3):
            assert (img[:, c, :, :fore[0]] == bg[c]).all() and (img[:, c, :, fore[1]:] == bg[c]).all()
        assert not (img[:, 0, :, fore[0]:fore[1]] == bg[0]).all()
    lw = r["losses"][0].item()
    print(f"loss_warp {lw:.9g}: {abs(lw - t['lw']) / tc.ulp32(lw):.1f} ulp from the kernel's arithmetic, |d fp64| {abs(lw - t['lw64']):.2e} (torch fp32 {abs(t['lw_torch32'] - t['lw64']):.2e})")
    assert abs(lw - t["lw"]) <= 2 * tc.ulp32(lw)
    assert abs(lw - t["lw64"]) <= 4 * abs(t["lw_torch32"] - t["lw64"]) + 2 * tc.ulp32(lw)
    assert r["losses"][1].item() == 0.0                   # the pose form: no alignment loss


@pytest.mark.parametrize("C", tc.COS_C)
@pytest.mark.parametrize("rows", tc.COS_ROWS)
def test_loss_align(emu_lib, rows, C):
    """cosine_partial_kernel at C = 4 .. 512 (260: a second, ragged trip of the channel loop) and 1, 5 and 1025 rows (more than 256 blocks x 4
    waves), with planted rows (zero in pg, zero in both, norm 1e-9, identical, opposite) among the random ones: |loss - fp64| within
    (8 ceil(C / 256) + 20) 2^-24 = 1.67e-6 (C <= 256) / 2.15e-6.  Measured, the same under the emulator and on an MI355X: 5.9e-9 .. 5.3e-8."""
    err, _, loss = tc.cos_case(emu_lib, DEV, rows, C)
    print(f"loss_align rows={rows} C={C}: {loss:.9g}, |d| {err:.2e} (bound {tc.cos_bound(C):.2e})")
    assert err <= tc.cos_bound(C)


def test_loss_align_planted_rows_only(emu_lib):
    """ten rows, all planted, so that the mean cannot hide them: cos = 0, 0, 0.1 (the clamp at 1e-8 decides), 1, -1"""
    err, cs, loss = tc.cos_case(emu_lib, DEV, 10, 64, only_planted=True)
    assert torch.allclose(cs, torch.tensor([0.0, 0.0, 0.1, 1.0, -1.0] * 2, dtype=torch.float64), atol=1e-12)
    assert err <= tc.cos_bound(64) and abs(loss - 0.98) <= 1e-6


def test_tail_refusals(emu_lib):
    assert tc.tail_refusals(emu_lib, DEV) >= 10


def test_engine_runs_the_operators_launches(emu_lib):
    """the configuration of test_train_extras.py::test_train_extras_emulated: tsnet_train_extras after a forward EQUALS tsnet_op_patch_warp +
    tsnet_op_train_tail on the forward's flows and pg / sg -- images and both losses"""
    import helpers as Hh
    from oracle import tsnet_oracle as O
    cfg = O.TSNetConfig(label_nc=2, n_blocks=0, n_source=2, ngf=8, enc_blocks=0, fuse_ngf=128)
    sd = O.synth_state_dict(cfg, seed=3, bias_std=0.02)
    sd = {k: (v * 3 if k.endswith("weight") else v) for k, v in sd.items()}
    inp = O.synth_inputs(cfg, 2, 32, 32, seed=4, mask_mode="box")
    tar_img = O.synth_inputs(cfg, 2, 32, 32, seed=1004, mask_mode="box")[0][0]
    eng = Hh.make_engine(cfg, sd, 32, 32, 2, DEV, lib=emu_lib)
    (img_a, loss_a), (img_b, loss_b) = tc.engine_tie_case(eng, inp, tar_img, DEV)
    eng.close()
    assert torch.equal(img_a, img_b) and torch.equal(loss_a, loss_b)
