"""The engine's life cycle on a tiny model, shared by the CPU tier (emulation library) and the GPU tier: a finalize that is refused and then
retried, and what tsnet_stage_ptr("src_fea") holds after a forward of each kind.  32 x 32 frames, n_downsampling 2, ngf 8: features 8 x 8,
P = 64 positions of C = 32 channels; K = 2 sources, max_batch 3.  The transition rules and their messages are test_source_bank.py's and
test_shared_sources.py's; nothing of them is restated here."""
import pytest
import torch

import helpers as Hh
from oracle import tsnet_oracle as O

K, BMAX, H, W, P, C = 2, 3, 32, 32, 64, 32
BAD = "fuse_net.conv.weight"          # the parameter that holds a NaN in the refused attempt: packed after the encoders, before the decoder


def net():
    cfg = O.TSNetConfig(label_nc=2, n_blocks=1, n_downsampling=2, n_source=K, ngf=8, enc_blocks=1, fuse_ngf=2 * C)
    sd = O.synth_state_dict(cfg, seed=21, bias_std=0.02)
    return cfg, {k: (v * 4.0 if k.endswith("weight") else v) for k, v in sd.items()}


def new_engine(cfg, lib, dev):
    return Hh.TSNetEngine(label_nc=cfg.label_nc, n_blocks=cfg.n_blocks, n_downsampling=cfg.n_downsampling, n_source=cfg.n_source, ngf=cfg.ngf,
                          enc_blocks=cfg.enc_blocks, addcoords=cfg.addcoords, height=H, width=W, max_batch=BMAX, lib=lib)


def on(dev, inp):
    return [[t.to(dev) for t in x] if isinstance(x, list) else x.to(dev) for x in inp]


def refused(cfg, sd, lib, dev):
    """an engine with every parameter loaded, one of them holding a NaN, whose finalize has been refused"""
    eng = new_engine(cfg, lib, dev)
    bad = dict(sd)
    bad[BAD] = sd[BAD].clone()
    bad[BAD].view(-1)[3] = float("nan")
    eng.load_state_dict({k: v.to(dev) for k, v in bad.items()})
    with pytest.raises(RuntimeError, match="non-finite"):
        eng.finalize(dev)
    return eng


def failed_finalize_then_retry(lib, dev):
    cfg, sd = net()
    inp = on(dev, O.synth_inputs(cfg, 2, H, W, seed=22, mask_mode="box"))
    eng = refused(cfg, sd, lib, dev)
    eng.load_state_dict({BAD: sd[BAD].to(dev)})
    eng.finalize(dev)
    fresh = Hh.make_engine(cfg, sd, H, W, BMAX, dev, lib=lib)
    got, want = Hh.run_engine(eng, inp, dev), Hh.run_engine(fresh, inp, dev)
    assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    assert eng.packed_weights(dev).numel() == fresh.packed_weights(dev).numel() > 0
    eng.close()
    fresh.close()


def src_fea_count_by_kind(lib, dev):
    cfg, sd = net()
    eng = new_engine(cfg, lib, dev)
    eng.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    with pytest.raises(RuntimeError, match="stage_ptr before a forward"):       # not finalized
        eng.stage("src_fea", dev)
    eng.finalize(dev)
    with pytest.raises(RuntimeError, match="stage_ptr before a forward"):       # finalized, no forward yet
        eng.stage("src_fea", dev)
    Hh.run_engine(eng, on(dev, O.synth_inputs(cfg, 2, H, W, seed=22, mask_mode="box")), dev)
    assert eng.stage("src_fea", dev).numel() == K * 2 * P * C                   # one-shot forward at B = 2: K * B images
    one = on(dev, O.synth_inputs(cfg, 1, H, W, seed=23, mask_mode="box"))
    tar = on(dev, O.synth_inputs(cfg, BMAX, H, W, seed=24, mask_mode="box"))
    eng.set_sources(one[0], one[1], one[2], shared=True)
    eng.forward_target(tar[3], tar[4])
    assert eng.stage("src_fea", dev).numel() == K * P * C                       # a shared source set, B = 3: K images
    eng.bank_put(1, one[0], one[1], one[2])
    eng.forward_bank([[2, 1]] * BMAX, tar[3], tar[4])
    assert eng.stage("src_fea", dev).numel() == K * BMAX * P * C                # the bank: every slot
    eng.close()
