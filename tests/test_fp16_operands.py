"""CPU tier of the fp16-operand mode (tsnet_cfg.operand_mode = 3, tsnet_op_conv2d nprod = 16): every one-product kernel with the f16 operand
kind under the fiber emulator against the operand-exact reference (fp16_cases.py), the refusals, and the whole forward of a narrow net
against the oracle that rounds the same operands to fp16.  The GPU tier (test_gpu_fp16_operands.py) runs the same cases on the hardware."""
import pytest
import torch

import fp16_cases as fc
import helpers as Hh
from oracle import tsnet_oracle as O


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_fp16_operand_exact_reference(emu_lib, family):
    """every family and tile code of op_cases.BF16_CASES with the f16 kind: only fp32 accumulation error is left (3128 and the two-group
    tiles included; the 2^+-40 cases show that the operand scale follows the bound)"""
    worst = fc.family_worst(emu_lib, "cpu", family)
    print(f"fp16 {family}: worst {worst:.2e} of max|ref|")
    assert worst < fc.REL


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_fp16_rounding_bit_exact(emu_lib, family):
    """a delta filter on inputs full of fp16 ties (no transform, alpha = 2^j with and without ReLU, a random alpha / beta) returns q(t), one-hot
    inputs on tied weights return q(w): bit for bit"""
    assert fc.exact_mismatches(emu_lib, "cpu", family) == []


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_fp16_scale_covariance(emu_lib, family):
    """op(x 2^j, bound 2^j) == 2^j op(x, bound) bit for bit for j = +-40; a bound loosened by 2^8 stays inside REL_BF16; an operand exactly at
    the bound is finite and exact"""
    assert fc.covariance_problems(emu_lib, "cpu", family) == []


def test_fp16_conv_cat(emu_lib):
    worst = fc.cat_worst(emu_lib, "cpu")
    print(f"fp16 concat: worst {worst:.2e} of max|ref|")
    assert worst < fc.REL


@pytest.mark.parametrize("family", list(fc.SAME_BITS))
def test_fp16_one_group_tiles_same_bits(emu_lib, family):
    ys = fc.tile_outputs(emu_lib, "cpu", family)
    assert all(torch.equal(ys[0], y) for y in ys[1:])


def test_fp16_refusals(emu_lib):
    """not built for the f16 kind: the Winograd form (kernel = 3) and the deep stride-2 schedule (12128), each refused with a message that names
    the mode; an unknown nprod; operand_mode = 4; operands = "fp16s" """
    msgs = fc.refusals(emu_lib, "cpu")
    assert "fp16 operands" in msgs[0] and "fp16 operands" in msgs[1] and "products" in msgs[2] and "products" in msgs[3], msgs
    fc.mode_refusals(emu_lib)


# Gates (a) of the emulated forward below: 1.25 x the worst of three (weight seed, input seed) draws measured under the emulator
# (profiles/fp16_operands.txt):            src_fea    tar_fea    sg         decoder (max)  decoder (mean)
#   w3  i4                                 3.845e-3   8.427e-4   3.070e-3   2.743e-3       1.927e-4
#   w13 i14                                4.345e-3   8.427e-4   3.804e-3   2.515e-3       1.681e-4
#   w23 i24                                4.177e-3   8.880e-4   2.947e-3   2.514e-3       1.862e-4
EMU_GATES = dict(src_fea=5.44e-3, tar_fea=1.11e-3, sg=4.76e-3, decoder_on_engine_features=3.43e-3, decoder_on_engine_features_mean=2.41e-4)


def _narrow_case(wseed, iseed):
    cfg = O.TSNetConfig(label_nc=2, n_blocks=1, n_source=2, ngf=8, enc_blocks=2, fuse_ngf=128)
    sd = O.synth_state_dict(cfg, seed=wseed, bias_std=0.02)
    sd = {k: (v * 4.0 if k.endswith("weight") else v) for k, v in sd.items()}      # non-trivial activations at width 8 (test_emu_forward._case)
    return cfg, sd, O.synth_inputs(cfg, 2, 64, 64, seed=iseed, mask_mode="box")


def test_fp16_forward_narrow_net(emu_lib, monkeypatch):
    """64 x 64, K = 2, n_blocks = 1, B = 2, box masks on the emulator tier's narrow net: (a) the fp16 engine within fp16 flip noise of the oracle
    that rounds the same operands, (b) at most a quarter of the bf16 engine's distance to the fp32 oracle, (c) the transformation branch on
    the engine's features fp32-class, (d) finite; and clip mode gives the one-shot forward's bits"""
    cfg, sd, inp = _narrow_case(3, 4)
    r, eng = fc.forward_report(monkeypatch, cfg, sd, inp, 2, 64, 64, "cpu", lib=emu_lib)
    fc.check_forward("fp16 emu w3 i4", r, EMU_GATES)
    eng.set_sources(inp[0], inp[1], inp[2])
    r2, _ = eng.forward_target(inp[3], inp[4])
    assert torch.equal(r["rec"], r2)
    eng.close()
