"""GPU tier of the fp16-operand mode (tsnet_cfg.operand_mode = 3, tsnet_op_conv2d nprod = 16): the cases of test_fp16_operands.py on the
MI355X through the HIP library, the whole forward at full width (a 64 x 64 frame and the demo's shape) against the oracle that rounds the
same operands to fp16, and the mode's bit-level invariants."""
import pytest
import torch

import fp16_cases as fc
import helpers as Hh
from oracle import tsnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from wacv23_tsnet_amd import _lib
    return _lib.load()       # raises if the HIP extension is missing: no fallback


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_fp16_operand_exact_reference(lib, family):
    worst = fc.family_worst(lib, DEV, family)
    print(f"fp16 {family}: worst {worst:.2e} of max|ref|")
    assert worst < fc.REL


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_fp16_rounding_bit_exact(lib, family):
    assert fc.exact_mismatches(lib, DEV, family) == []


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_fp16_scale_covariance(lib, family):
    assert fc.covariance_problems(lib, DEV, family) == []


def test_fp16_conv_cat(lib):
    worst = fc.cat_worst(lib, DEV)
    print(f"fp16 concat: worst {worst:.2e} of max|ref|")
    assert worst < fc.REL


@pytest.mark.parametrize("family", list(fc.SAME_BITS))
def test_fp16_one_group_tiles_same_bits(lib, family):
    ys = fc.tile_outputs(lib, DEV, family)
    assert all(torch.equal(ys[0], y) for y in ys[1:])


def test_fp16_refusals(lib):
    msgs = fc.refusals(lib, DEV)
    assert "fp16 operands" in msgs[0] and "fp16 operands" in msgs[1] and "products" in msgs[2] and "products" in msgs[3], msgs
    fc.mode_refusals(lib)


# ---- the whole forward.  Gates (a): 1.25 x the worst of three (weight seed, input seed) draws measured on an MI355X (profiles/fp16_operands.txt)
#                                          src_fea    tar_fea    sg         decoder (max)  decoder (mean)
#   64^2  K=2 nb=1 B=2   w100 i200         1.522e-2  9.860e-4  5.451e-3  1.274e-3       1.791e-4
#                        w110 i210         1.509e-2  9.848e-4  5.385e-3  1.376e-3       1.924e-4
#                        w120 i220         1.469e-2  1.102e-3  6.234e-3  1.410e-3       1.816e-4
#   256^2 K=3 nb=4 B=1   w101 i201         1.757e-2  1.103e-3  5.050e-3  3.187e-3       3.407e-4
#                        w111 i211         2.147e-2  1.642e-3  5.689e-3  3.026e-3       3.272e-4
#                        w121 i221         1.955e-2  1.378e-3  6.245e-3  2.655e-3       3.403e-4
GPU_GATES = {
    "small": dict(src_fea=1.91e-2, tar_fea=1.38e-3, sg=7.80e-3, decoder_on_engine_features=1.77e-3, decoder_on_engine_features_mean=2.41e-4),
    "demo": dict(src_fea=2.69e-2, tar_fea=2.06e-3, sg=7.81e-3, decoder_on_engine_features=3.99e-3, decoder_on_engine_features_mean=4.26e-4),
}
CASES = {"small": (dict(label_nc=2, n_blocks=1, n_source=2), 2, 64, 64, 100, 200), "demo": (dict(label_nc=2, n_blocks=4, n_source=3), 1, 256, 256, 101, 201)}


def forward_case(monkeypatch, tag, wseed=None, iseed=None):
    kw, B, H, W, ws, isd = CASES[tag]
    cfg = O.TSNetConfig(**kw)
    sd = O.synth_state_dict(cfg, seed=ws if wseed is None else wseed, bias_std=0.02)
    inp = O.synth_inputs(cfg, B, H, W, seed=isd if iseed is None else iseed, mask_mode="box")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    r, eng = fc.forward_report(monkeypatch, cfg, sd, inp, B, H, W, DEV)
    eng.close()
    return r


@pytest.mark.parametrize("tag", list(CASES))
def test_fp16_forward(monkeypatch, tag):
    """(a) within fp16 flip noise of the oracle that rounds the same operands, (b) at most a quarter of the bf16 engine's distance to the fp32
    oracle on the same draw, (c) the transformation branch on the engine's features fp32-class, (d) finite"""
    fc.check_forward(f"fp16 gpu {tag}", forward_case(monkeypatch, tag), GPU_GATES[tag])


# ---- invariants: 64 x 64, K = 2, n_blocks = 1
@pytest.fixture(scope="module")
def small():
    cfg = O.TSNetConfig(label_nc=2, n_blocks=1, n_source=2)
    sd = O.synth_state_dict(cfg, seed=100, bias_std=0.02)
    eng = Hh.make_engine(cfg, sd, 64, 64, 3, DEV, operands="fp16")
    yield cfg, sd, eng
    eng.close()


def test_fp16_frame_alone_equals_frame_in_batch(small):
    cfg, sd, eng = small
    inp = O.synth_inputs(cfg, 3, 64, 64, seed=200, mask_mode="box")
    full, fl = Hh.run_engine(eng, inp, DEV)
    sub = ([x[1:2] for x in inp[0]], [x[1:2] for x in inp[1]], [x[1:2] for x in inp[2]], inp[3][1:2], inp[4][1:2])
    one, f1 = Hh.run_engine(eng, sub, DEV)
    assert torch.equal(one, full[1:2]) and all(torch.equal(a, b[1:2]) for a, b in zip(f1, fl))


def test_fp16_shared_sources_equal_forward(small):
    cfg, sd, eng = small
    src = O.synth_inputs(cfg, 1, 64, 64, seed=201, mask_mode="box")[:3]
    tar_lbl, tar_bbox = O.synth_inputs(cfg, 3, 64, 64, seed=202, mask_mode="box")[3:]
    rep = tuple([x.repeat(3, *([1] * (x.dim() - 1))) for x in part] for part in src)
    ref, rf = Hh.run_engine(eng, (*rep, tar_lbl, tar_bbox), DEV)
    eng.set_sources(*[[t.to(DEV) for t in part] for part in src], shared=True)
    rec, flows = eng.forward_target(tar_lbl.to(DEV), tar_bbox.to(DEV), return_flow=True)
    torch.cuda.synchronize()
    assert torch.equal(rec.cpu(), ref) and all(torch.equal(a.cpu(), b) for a, b in zip(flows, rf))


def test_fp16_replica_through_packed_weights(small):
    """what a replica receives is what its kernels read: an engine finalised from zeros that takes the first one's packed buffer (one fp16 plane
    per layer and the un-scale factors) computes the same bits"""
    cfg, sd, eng = small
    inp = O.synth_inputs(cfg, 2, 64, 64, seed=203, mask_mode="box")
    ref, _ = Hh.run_engine(eng, inp, DEV, return_flow=False)
    e2 = Hh.make_engine(cfg, {k: torch.zeros_like(v) for k, v in sd.items()}, 64, 64, 3, DEV, operands="fp16")
    zero, _ = Hh.run_engine(e2, inp, DEV, return_flow=False)
    src, dst = eng.packed_weights(DEV), e2.packed_weights(DEV)
    assert src.numel() == dst.numel()
    dst.copy_(src)
    torch.cuda.synchronize()
    rec, _ = Hh.run_engine(e2, inp, DEV, return_flow=False)
    e2.close()
    assert torch.equal(rec, ref) and not torch.equal(zero, ref)
