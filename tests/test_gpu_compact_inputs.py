"""GPU tier: compact inputs (tsnet_*_u8) on the device.  Bit equality with the float32 path: the packing kernel alone at the sizes that reach
its aligned 32-bit loads, its byte path and its tail; the narrow net's one-shot forward, shared clip mode and bank in fp32 and bf16; the pack
kernel's full-size grid once (256 x 256, 25 labels); and the reference loader's own bytes from a committed golden."""
import pytest
import torch

import compact_cases as cc
import helpers as Hh
from wacv23_tsnet_amd import frames

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, BMAX, H, W = 2, 3, 32, 32


@pytest.mark.parametrize("name", list(cc.PACK_U8_CASES))
def test_op_pack_input_u8_equals_float_op(name):
    from wacv23_tsnet_amd import _lib
    cc.check_pack(_lib.load(), DEV, name)


def test_op_pack_input_u8_refusals():
    from wacv23_tsnet_amd import _lib
    assert cc.pack_u8_refusals(_lib.load(), DEV) >= 20


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_narrow_net_forward_clip_and_bank(operands):
    """ngf = 8, 32 x 32: one-shot forward (B = 2, K = 2), the shared clip mode in every combination of forms, and a bank with slots in both
    forms, a mixed table and a compact replacement -- each equal to the all-float result"""
    cfg, sd = cc.narrow_net(L=2, n_source=K)
    eng = Hh.make_engine(cfg, sd, H, W, BMAX, DEV, operands=operands)
    cc.check_forward(eng, cc.Inputs(2, K, 2, H, W, seed=21, dev=DEV), DEV)
    inp = cc.Inputs(2, K, BMAX, H, W, seed=23, dev=DEV)
    cc.check_clip_modes(eng, inp, DEV, shared=True)
    cc.check_clip_modes(eng, inp, DEV, shared=False, combos=(("c", "c"),))
    cc.check_bank(eng, cc.Inputs(2, 7, 1, H, W, seed=24, dev=DEV), cc.Inputs(2, 1, BMAX, H, W, seed=25, dev=DEV), DEV,
                  [[4, 1], [1, 4], [0, 0]], ["c", "f", "f", "c", "c", "f"])
    eng.close()


def test_full_size_pose_grid():
    """256 x 256, L = 25 (Cp = 32 in both stems), B = 2, ngf = 8, n_blocks = 0, enc_blocks = 1: the pack kernel's full-size grid geometry
    on real hardware, one-shot and through the shared cache"""
    cfg, sd = cc.narrow_net(L=25, n_source=K, nb=0, enc_blocks=1)
    eng = Hh.make_engine(cfg, sd, 256, 256, 2, DEV)
    inp = cc.Inputs(25, K, 2, 256, 256, seed=41, dev=DEV)
    want = cc.check_forward(eng, inp, DEV)
    eng.set_sources(*inp.src("c", b=1), shared=True, mean=cc.MEAN)
    got = eng.forward_target(inp.c[3][1:], inp.c[4][1:], return_flow=True)
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0][1:]) and all(torch.equal(a, b[1:]) for a, b in zip(got[1], want[1]))
    eng.close()


def test_reference_loader_bytes_from_a_golden():
    """g10_face_test114_to_val024_b1: the reference loader's outputs for a demo pair, stored as BYTES -- the resized BGR frames before the mean
    subtraction, class maps, packed masks.  The compact forward takes those bytes as they are; the float forward takes helpers.stored_inputs'
    exact widening of them (the golden holds no float tensors: that form is derived, byte.astype(float32) - mean, one-hot, unpacked bits).
    The two must agree bit for bit, and the device frame loader's byte output on the clip's frames must BE the stored image bytes."""
    meta, cfg, sd, finp, cinp, mean = cc.golden_compact("g10_face_test114_to_val024_b1")
    B = meta["B"]
    eng = Hh.make_engine(cfg, sd, meta["H"], meta["W"], B, DEV)
    dev = lambda x: [t.to(DEV) for t in x] if isinstance(x, list) else x.to(DEV)
    want = eng.forward(*[dev(x) for x in finp], return_flow=True)
    torch.cuda.synchronize()
    want = (want[0].clone(), [f.clone() for f in want[1]])
    got = eng.forward(*[dev(x) for x in cinp], return_flow=True, mean=mean)
    torch.cuda.synchronize()
    assert torch.isfinite(want[0]).all() and cc.same(got, want)
    eng.close()
    import json
    import numpy as np
    import os
    z = np.load(os.path.join(Hh.GOLD, "g11_frames_test114.npz"))
    x0, y0, x1, y1 = json.loads(str(z["meta"]))["box"]
    img = frames.FrameLoader(DEV).face(z["crops"], [0, y1 - y0, 0, x1 - x0], as_bytes=True)
    assert img.dtype == torch.uint8 and torch.equal(img.cpu(), torch.cat([t[:1] for t in cinp[0]]))


def test_prepare_frames_u8_on_the_device():
    import numpy as np
    fr = np.random.default_rng(7).integers(0, 256, (2, 90, 70, 3), dtype=np.uint8)
    ld = frames.FrameLoader(DEV)
    for box, size, square in (((-10, -7, 50, 40), (24, 40), False), ((3, 10, 67, 74), (16, 64), True), ((0, 0, 70, 90), (130, 70), False)):
        want = ld.prepare(fr, box, size, square=square)
        got = ld.prepare(fr, box, size, square=square, as_bytes=True)
        torch.cuda.synchronize()
        assert got.dtype == torch.uint8 and torch.equal(cc.widen_img(got.cpu()), want.cpu())
