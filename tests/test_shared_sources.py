"""CPU tier: clip mode with ONE source set shared by a batch of driving frames (tsnet_set_sources_shared), under the fiber emulator on a
narrow net (ngf=8).  The shared cache holds K encoded images; frame b of forward_target must carry the bits of the one-shot forward on
(the same sources replicated, driving frame b) -- in any batch up to max_batch, ragged tails included, against one cache.

(The pose variant on a 256 x 256 frame is not run here: one emulated pose forward takes ~47 s, the case needs four.  The GPU tier holds
it: tests/test_gpu_shared_sources.py::test_pose_shared.)"""
import pytest
import torch

import helpers as Hh
from oracle import tsnet_oracle as O

B = 3


def _case(K=2, nb=1, L=2, H=32, W=32, enc_blocks=2, wscale=4.0, bias_std=0.02, mask="box", seed=3):
    """(cfg, weights, one source set of batch 1, B driving frames)"""
    cfg = O.TSNetConfig(label_nc=L, n_blocks=nb, n_source=K, ngf=8, enc_blocks=enc_blocks, fuse_ngf=128)
    sd = O.synth_state_dict(cfg, seed=seed, bias_std=bias_std)
    sd = {k: (v * wscale if k.endswith("weight") else v) for k, v in sd.items()}   # non-trivial activations at width 8
    src = O.synth_inputs(cfg, 1, H, W, seed=seed + 1, mask_mode=mask)[:3]
    drv = O.synth_inputs(cfg, B, H, W, seed=seed + 2, mask_mode=mask)[3:]
    return cfg, sd, src, drv


def _rep(src, n):
    return tuple([x.repeat(n, *([1] * (x.dim() - 1))) for x in part] for part in src)


def _same(a, b):
    (ra, fa), (rb, fb) = a, b
    return torch.equal(ra, rb) and len(fa) == len(fb) and all(torch.equal(x, y) for x, y in zip(fa, fb))


CASES = [dict(K=2, nb=1), dict(K=3, nb=0, mask="bernoulli"), dict(K=1, nb=2, L=5, H=48, W=32, mask="soft")]


@pytest.mark.parametrize("kw", CASES)
def test_shared_equals_replicated_sources(emu_lib, kw):
    cfg, sd, src, (tar_lbl, tar_bbox) = _case(**kw)
    H, W = tar_lbl.shape[2], tar_lbl.shape[3]
    eng = Hh.make_engine(cfg, sd, H, W, B, "cpu", lib=emu_lib)
    ref = Hh.run_engine(eng, (*_rep(src, B), tar_lbl, tar_bbox), "cpu")
    eng.set_sources(*src, shared=True)
    full = eng.forward_target(tar_lbl, tar_bbox, return_flow=True)
    assert _same(full, ref)
    assert eng.stage("src_fea", "cpu").shape[0] == cfg.n_source          # K encoded images, not K * B
    # ragged batches against the SAME cache
    for lo, hi in ((0, 1), (1, 3)):
        rec, flows = eng.forward_target(tar_lbl[lo:hi], tar_bbox[lo:hi], return_flow=True)
        assert torch.equal(rec, full[0][lo:hi])
        assert all(torch.equal(f, g[lo:hi]) for f, g in zip(flows, full[1]))
    # ... and every frame equals the per-batch clip mode at B = 1
    eng.set_sources(*src)
    for b in range(B):
        rec, flows = eng.forward_target(tar_lbl[b:b + 1], tar_bbox[b:b + 1], return_flow=True)
        assert torch.equal(rec, full[0][b:b + 1])
        assert all(torch.equal(f, g[b:b + 1]) for f, g in zip(flows, full[1]))
    eng.close()


@pytest.mark.parametrize("operands", ["bf16", "bf16s"])
def test_shared_operand_modes(emu_lib, operands):
    cfg, sd, src, (tar_lbl, tar_bbox) = _case(K=2, nb=1)
    eng = Hh.make_engine(cfg, sd, 32, 32, B, "cpu", lib=emu_lib, operands=operands)
    ref = Hh.run_engine(eng, (*_rep(src, B), tar_lbl, tar_bbox), "cpu")
    eng.set_sources(*src, shared=True)
    assert _same(eng.forward_target(tar_lbl, tar_bbox, return_flow=True), ref)
    rec, _ = eng.forward_target(tar_lbl[1:3], tar_bbox[1:3])
    assert torch.equal(rec, ref[0][1:3])
    eng.close()


def test_state_rules(emu_lib):
    cfg, sd, src, (tar_lbl, tar_bbox) = _case(K=2, nb=0)
    eng = Hh.make_engine(cfg, sd, 32, 32, 2, "cpu", lib=emu_lib)
    # shared tensors have batch 1
    with pytest.raises(ValueError, match="batch 1"):
        eng.set_sources(*_rep(src, 2), shared=True)
    # a per-batch cache keeps its rule: another batch is refused with the message it always had
    eng.set_sources(*_rep(src, 2))
    with pytest.raises(RuntimeError, match="batch differs from the cached sources"):
        eng.forward_target(tar_lbl[:1], tar_bbox[:1])
    # the shared cache takes any batch up to max_batch, and no more
    eng.set_sources(*src, shared=True)
    one, _ = eng.forward_target(tar_lbl[:1], tar_bbox[:1])
    two, _ = eng.forward_target(tar_lbl[:2], tar_bbox[:2])
    assert torch.equal(one, two[:1])
    with pytest.raises(RuntimeError, match="max_batch"):
        eng.forward_target(tar_lbl, tar_bbox)                            # B = 3 > max_batch = 2
    assert eng.stage("src_fea", "cpu").shape[0] == cfg.n_source
    # train_extras is per batch element: refused after a forward on the shared cache (at B = 1 too) ...
    img2 = [x.repeat(2, 1, 1, 1) for x in src[0]]
    with pytest.raises(RuntimeError, match="shared source set"):
        eng.train_extras(img2, img2[0])
    eng.forward_target(tar_lbl[:1], tar_bbox[:1])
    with pytest.raises(RuntimeError, match="shared source set"):
        eng.train_extras(src[0], src[0][0])
    # ... and accepted again after a per-batch forward
    Hh.run_engine(eng, (*_rep(src, 2), tar_lbl[:2], tar_bbox[:2]), "cpu")
    eng.train_extras(img2, img2[0])
    # a per-batch set_sources replaces the shared cache (B = 1 no longer fits a B = 2 cache)
    eng.set_sources(*src, shared=True)
    eng.set_sources(*_rep(src, 2))
    with pytest.raises(RuntimeError, match="batch differs from the cached sources"):
        eng.forward_target(tar_lbl[:1], tar_bbox[:1])
    # set_source_divisors drops it: the features were encoded with the previous divisors
    eng.set_sources(*src, shared=True)
    eng.set_source_divisors([1.0, 255.0])
    with pytest.raises(RuntimeError, match="set_sources"):
        eng.forward_target(tar_lbl[:2], tar_bbox[:2])
    # the one-shot forward replaces it with its own per-batch cache
    eng.set_source_divisors(None)
    eng.set_sources(*src, shared=True)
    ref = Hh.run_engine(eng, (*_rep(src, 2), tar_lbl[:2], tar_bbox[:2]), "cpu")
    with pytest.raises(RuntimeError, match="batch differs from the cached sources"):
        eng.forward_target(tar_lbl[:1], tar_bbox[:1])
    assert _same(eng.forward_target(tar_lbl[:2], tar_bbox[:2], return_flow=True), ref)
    eng.close()
