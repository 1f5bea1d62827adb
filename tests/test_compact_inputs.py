"""CPU tier: compact inputs (byte images, class-index labels, byte masks; tsnet_*_u8) under the fiber emulator, on test_source_bank.py's narrow
net (ngf = 8, 32 x 32).  The stems' packing kernel widens on load with the operations the wide tensors went through on the host, so the
acceptance criterion is bit equality with the float32 path everywhere: every comparison below is torch.equal / np.array_equal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import compact_cases as cc
import helpers as Hh
from wacv23_tsnet_amd import demo, frames, raster

K, BMAX, H, W = 2, 3, 32, 32
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.PACK_U8_CASES))
def test_op_pack_input_u8_equals_float_op(emu_lib, name):
    """out, amax (and the widened masks) of tsnet_op_pack_input_u8 == tsnet_op_pack_input on the widened tensors: Cp 8 / 16 / 32, L 2 / 25,
    nimg 3 / 0, with and without coords, S*B up to 8 with B > 1, divisors 255 and 1, label bytes >= L; 32 x 32 (aligned words), 5 x 7 (odd
    H*W: planes at every residue mod 4 and a tail), 33 x 33 (two workgroups of pixels), 363 x 362 (the grid-stride loop repeats)."""
    cc.check_pack(emu_lib, "cpu", name)


def test_op_pack_input_u8_refusals(emu_lib):
    assert cc.pack_u8_refusals(emu_lib, "cpu") >= 20


# ---------------------------------------------------------------------------------------------------------------------------------------
class Net:
    def __init__(self, lib, operands="fp32", L=2):
        self.lib, self.operands = lib, operands
        self.cfg, self.sd = cc.narrow_net(L=L, n_source=K)

    def engine(self):
        return Hh.make_engine(self.cfg, self.sd, H, W, BMAX, "cpu", lib=self.lib, operands=self.operands)


@pytest.fixture(scope="module")
def net(emu_lib):
    return Net(emu_lib)


@pytest.mark.parametrize("operands", ["fp32", "bf16"])
def test_forward_compact_equals_float(emu_lib, operands):
    n = Net(emu_lib, operands)
    eng = n.engine()
    cc.check_forward(eng, cc.Inputs(2, K, 2, H, W, seed=21), "cpu")
    eng.close()


def test_forward_compact_equals_float_pose_labels(emu_lib):
    """25 classes: Cp = 32 stems in both encoders"""
    n = Net(emu_lib, L=25)
    eng = n.engine()
    cc.check_forward(eng, cc.Inputs(25, K, 2, H, W, seed=22), "cpu")
    eng.close()


@pytest.mark.parametrize("shared", [False, True])
def test_clip_modes_in_every_combination_of_forms(net, shared):
    eng = net.engine()
    inp = cc.Inputs(2, K, BMAX, H, W, seed=23)
    want = cc.check_clip_modes(eng, inp, "cpu", shared)
    if shared:                                                   # ... and the shared cache still takes any batch
        eng.set_sources(*inp.src("c", b=0), shared=True, mean=cc.MEAN)
        one, _ = eng.forward_target(*inp.tar("c", [1]))
        assert torch.equal(one, want[0][1:2])
    eng.close()


def test_bank_with_slots_in_both_forms(net):
    """six slots put compact, float, float, compact, compact, float; a mixed table; compact and float driving frames; a compact put
    replacing slot 4 changes frames 0 and 1 (its readers) and leaves frame 2's bits"""
    eng = net.engine()
    pool = cc.Inputs(2, 7, 1, H, W, seed=24)
    tar = cc.Inputs(2, 1, BMAX, H, W, seed=25)
    cc.check_bank(eng, pool, tar, "cpu", [[4, 1], [1, 4], [0, 0]], ["c", "f", "f", "c", "c", "f"])
    eng.close()


def test_state_machine_is_the_siblings(net):
    """a compact call meets the refusals of its sibling, with its messages"""
    eng = net.engine()
    inp = cc.Inputs(2, K, 2, H, W, seed=26)
    with pytest.raises(RuntimeError, match="batch differs from the cached sources"):
        eng.forward_target(*inp.tar("c"))
    with pytest.raises(RuntimeError, match="no source bank"):
        eng.forward_bank([[0, 1]], *inp.tar("c", [0]))
    eng.bank_put(0, *inp.src("c", [0], b=0), mean=cc.MEAN)
    with pytest.raises(RuntimeError, match="slot 1 is not filled"):
        eng.forward_bank([[0, 1]], *inp.tar("c", [0]))
    with pytest.raises(RuntimeError, match=r"slots 5 \.\. 6 are outside the bank"):
        eng.bank_put(5, *inp.src("c", b=0), mean=cc.MEAN)
    with pytest.raises(RuntimeError, match="max_batch"):
        big = cc.Inputs(2, K, BMAX + 1, H, W, seed=27)
        eng.forward(*big.c, mean=cc.MEAN)
    # divisors: tsnet_set_source_divisors for the caches, `div` for a put -- as for the float calls
    eng.set_source_divisors([1.0, 255.0])
    a = eng.forward(*inp.c, mean=cc.MEAN)[0].clone()
    b = eng.forward(*inp.f)[0].clone()
    eng.set_source_divisors(None)
    c = eng.forward(*inp.c, mean=cc.MEAN)[0]
    assert torch.equal(a, b) and not torch.equal(a, c)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
def _ptrs(ts):
    return (C.c_void_p * 8)(*[t.data_ptr() for t in ts])


def test_c_entries_refuse_bad_arguments(net):
    """every new forward entry: TSNET_ERR_ARG, a message, nothing written"""
    eng = net.engine()
    lib, h = eng.lib, eng._h
    inp = cc.Inputs(2, K, 1, H, W, seed=28)
    si, sl, sb, tl, tb = inp.c
    mean = (C.c_float * 3)(*cc.MEAN)
    out = torch.full((1, 3, H, W), float("nan"))
    holed = (C.c_void_p * 8)(si[0].data_ptr(), None)
    err = lambda: lib.tsnet_last_error(h).decode()

    def refused(rc, text):
        assert rc == -1 and text in err(), (rc, err())
        assert torch.isnan(out).all()

    ft = lambda **k: lib.tsnet_forward_target_u8(h, k.get("tl", tl.data_ptr()), k.get("tb", tb.data_ptr()), out.data_ptr(), None, k.get("B", 1), None)
    refused(ft(), "batch differs from the cached sources")          # (first: a refused forward below may leave its sources cached, as tsnet_forward does)
    fwd = lambda **k: lib.tsnet_forward_u8(h, k.get("si", _ptrs(si)), _ptrs(sl), _ptrs(sb), k.get("tl", tl.data_ptr()), tb.data_ptr(),
                                           k.get("mean", mean), k.get("out", out.data_ptr()), None, k.get("B", 1), None)
    refused(fwd(mean=None), "null mean_bgr")
    refused(fwd(si=None), "null source list")
    refused(fwd(si=holed), "null source tensor")
    refused(fwd(tl=None), "null target/output tensor")
    refused(fwd(out=None), "null target/output tensor")
    refused(fwd(B=0), "batch size outside 1..max_batch")
    refused(fwd(B=BMAX + 1), "batch size outside 1..max_batch")
    ss = lambda **k: lib.tsnet_set_sources_u8(h, k.get("si", _ptrs(si)), _ptrs(sl), _ptrs(sb), k.get("mean", mean), k.get("B", 1), k.get("shared", 0), None)
    refused(ss(mean=None), "null mean_bgr")
    refused(ss(si=holed), "null source tensor")
    refused(ss(B=0), "batch size")
    refused(ss(B=2, shared=1), "a shared source set has batch 1")
    assert ss() == 0
    refused(ft(tl=None), "null target/output tensor")
    refused(ft(tb=None), "null target/output tensor")
    refused(ft(B=2), "batch differs from the cached sources")
    bp = lambda **k: lib.tsnet_bank_put_u8(h, k.get("first", 0), k.get("count", 2), k.get("si", _ptrs(si)), _ptrs(sl), _ptrs(sb), k.get("mean", mean),
                                           k.get("div", None), None)
    refused(bp(mean=None), "null mean_bgr")
    refused(bp(first=5), "are outside the bank")
    refused(bp(count=0), "are outside the bank")
    refused(bp(si=holed), "null source tensor")
    refused(bp(div=(C.c_float * 2)(255.0, -1.0)), "divisors must be positive")
    tab = (C.c_int * 2)(0, 1)
    fb = lambda **k: lib.tsnet_forward_bank_u8(h, k.get("tab", tab), k.get("Kc", 2), k.get("tl", tl.data_ptr()), tb.data_ptr(), out.data_ptr(), None, 1, None)
    refused(fb(), "no source bank")
    assert bp(count=1) == 0
    refused(fb(), "slot 1 is not filled")
    refused(fb(Kc=3), "sources per frame outside 1..n_source")
    refused(fb(tab=None), "null slot table")
    refused(fb(tl=None), "null slot table")
    refused(fb(tab=(C.c_int * 2)(0, 6)), "slot 6 is outside the bank")
    for fn in (lib.tsnet_forward_u8, lib.tsnet_set_sources_u8, lib.tsnet_forward_target_u8, lib.tsnet_bank_put_u8, lib.tsnet_forward_bank_u8):
        assert fn(*[0 if t is C.c_int else None for t in fn.argtypes]) == -1       # a null handle
    eng.close()


def test_label_nc_above_255_is_refused(emu_lib):
    cfg, sd = cc.narrow_net(L=256, n_source=1, nb=0, enc_blocks=0)
    eng = Hh.make_engine(cfg, sd, 16, 16, 1, "cpu", lib=emu_lib)
    z = torch.zeros((1, 3, 16, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="label_nc <= 255"):
        eng.forward([z], [z[:, 0]], [z[:, 0]], z[:, 0], z[:, 0], mean=cc.MEAN)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
FRAME_CASES = [                                                 # (frame h, w), box (x0, y0, x1, y1), size (ow, oh), square
    ((60, 80), (5, 3, 75, 57), (32, 32), False),
    ((60, 80), (-10, -7, 50, 40), (24, 40), False),              # the box leaves the frame
    ((48, 48), (8, 4, 40, 44), (32, 20), False),                 # the horizontal pass is skipped (32 -> 32)
    ((90, 70), (3, 10, 67, 74), (16, 64), True),                 # the vertical pass is skipped; resize_square's bars
    ((33, 37), (0, 0, 37, 33), (130, 70), False),                # upscaling, more than one tile
]


@pytest.mark.parametrize("case", FRAME_CASES)
def test_prepare_frames_u8_is_the_float_entry_before_the_mean(emu_lib, case):
    (h, w), box, size, square = case
    fr = np.random.default_rng(h * 100 + w).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    want = ld.prepare(fr, box, size, square=square)
    got = ld.prepare(fr, box, size, square=square, as_bytes=True)
    assert got.dtype == torch.uint8 and got.shape == want.shape and got.float().max() > 0
    assert torch.equal(cc.widen_img(got), want)
    if square:
        assert torch.equal(ld.pose(fr, box, size, as_bytes=True), got)
    else:
        x0, y0, x1, y1 = box
        assert torch.equal(ld.face(fr, [y0, y1, x0, x1], size, as_bytes=True), got)


def test_prepare_frames_u8_refusals(emu_lib):
    fr = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    out = torch.full((3 * 8 * 8,), 7, dtype=torch.uint8)
    call = lambda **k: emu_lib.tsnet_prepare_frames_u8(k.get("fr", fr.data_ptr()), 1, 8, 8, 0, 0, k.get("x1", 8), 8, None, None, None, 0, None, None, None, 0,
                                                       8, 8, k.get("pad", 0), 0, 8, 8, k.get("out", out.data_ptr()), None)
    assert call() == 0 and (out == 0).all()
    out.fill_(7)
    for k in ({"fr": None}, {"out": None}, {"x1": 0}, {"x1": 4}, {"pad": 1}):
        assert call(**k) == -1 and emu_lib.tsnet_op_last_error().decode().startswith("prepare_frames"), k
        assert (out == 7).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_mixed_calls(net):
    eng = net.engine()
    inp = cc.Inputs(2, K, 2, H, W, seed=29)
    si, sl, sb, tl, tb = inp.c
    fi, fl, fb, ftl, ftb = inp.f
    with pytest.raises(TypeError, match=r"src_img\[1\]"):
        eng.forward([si[0], fi[1]], sl, sb, tl, tb, mean=cc.MEAN)
    with pytest.raises(TypeError, match="tar_bbox"):
        eng.forward(si, sl, sb, tl, tb.float(), mean=cc.MEAN)
    with pytest.raises(TypeError, match=r"src_lbl\[0\]"):
        eng.forward(fi, sl, fb, ftl, ftb)                            # a float call (its tar_lbl is float) handed a byte tensor
    with pytest.raises(TypeError, match=r"src_bbox\[0\]"):
        eng.set_sources(si, sl, [sb[0].float(), sb[1]], mean=cc.MEAN)
    with pytest.raises(TypeError, match="tar_bbox"):
        eng.forward_target(tl, ftb)
    with pytest.raises(TypeError, match=r"src_img\[0\]"):
        eng.bank_put(0, [fi[0][:1]], [sl[0][:1]], [sb[0][:1]], mean=cc.MEAN)
    with pytest.raises(ValueError, match=r"src_lbl\[0\]: expected compact shape \(2, 32, 32\)"):
        eng.forward(si, [cc.widen_lbl(sl[0], 2).to(torch.uint8), sl[1]], sb, tl, tb, mean=cc.MEAN)
    with pytest.raises(ValueError, match="tar_lbl"):
        eng.forward_target(tl[:, None], tb)
    with pytest.raises(ValueError, match="tar_bbox"):
        eng.forward_bank([[0, 1]] * 2, tl, tb[:1])
    for call in (lambda: eng.forward(si, sl, sb, tl, tb), lambda: eng.set_sources(si, sl, sb), lambda: eng.bank_put(0, *inp.src("c", b=0))):
        with pytest.raises(ValueError, match="needs mean="):
            call()
    with pytest.raises(ValueError, match="three values"):
        eng.forward(si, sl, sb, tl, tb, mean=[1.0, 2.0])
    with pytest.raises(ValueError, match="belongs to a compact"):
        eng.forward(fi, fl, fb, ftl, ftb, mean=cc.MEAN)
    with pytest.raises(TypeError):                                   # (tests/test_host_logic.py's refusal of a double tensor stands)
        eng.forward([fi[0].double(), fi[1]], fl, fb, ftl, ftb)
    eng.close()


def test_face_clip_labels_compact(emu_lib):
    import demo_clip
    kps = list(demo_clip.synthetic_face_keypoints(2))
    rs = raster.FaceRasteriser("cpu", lib=emu_lib)
    lbl, box, crop = rs.clip_labels(kps, size=(256, 256))
    cl, cb, crop2 = rs.clip_labels(kps, size=(256, 256), compact=True)
    assert crop == crop2 and cl.dtype == cb.dtype == torch.uint8 and cl.shape == cb.shape == (2, 256, 256)
    assert lbl.shape == (2, 2, 256, 256) and torch.equal(rs.vl2ch(cl, 2), lbl) and torch.equal(cb.float(), box)
    assert 0 < int(cl.sum()) < cl.numel() and torch.equal(cc.widen_lbl(cl, 2), lbl)


def test_pose_clip_labels_compact(emu_lib):
    import json
    z = np.load(os.path.join(Hh.GOLD, "g9_raster_pose.npz"))
    pts, size = z["00110_pts"][:1], tuple(json.loads(str(z["meta"]))["clips"]["00110"]["size"])
    pr = raster.PoseRasteriser("cpu", lib=emu_lib)
    cls, box, win = pr.clip_labels(list(pts), size)
    ccls, cbox, win2 = pr.clip_labels(list(pts), size, compact=True)
    assert win == win2 and ccls.dtype == cbox.dtype == torch.uint8 and ccls.shape == cls.shape
    fr = raster.FaceRasteriser("cpu", lib=emu_lib)
    assert torch.equal(fr.vl2ch(ccls, 25), fr.vl2ch(cls, 25)) and torch.equal(cbox.float(), box)
    assert len(torch.unique(ccls)) > 2 and torch.equal(cc.widen_lbl(ccls, 25), fr.vl2ch(cls, 25))


class _EmuModel:
    """what demo.ClipRunner asks of a model, on the emulator"""

    def __init__(self, net):
        self.net, self.n_source = net, K

    def _device(self):
        return torch.device("cpu")

    def _new_engine(self, batch):
        return Hh.make_engine(self.net.cfg, self.net.sd, H, W, batch, "cpu", lib=self.net.lib)


def test_clip_runner_takes_either_form(net, batch=2):
    """sources / driving frames / a replaced source, compact or float: the bytes of the all-float runner (batch 2: the shared cache, groups 2 + 1)"""
    model = _EmuModel(net)
    src = cc.Inputs(2, K + 1, 1, H, W, seed=30)
    drv = cc.Inputs(2, 1, 3, H, W, seed=31)
    with demo.ClipRunner(model, *src.src("f", range(K)), batch=batch) as r:
        want = r.run(*drv.tar("f"))
        r.replace_source(1, *[p[0] for p in src.src("f", [K])])
        want2 = r.run(*drv.tar("f"))
    assert want.dtype == np.uint8 and want.shape == (3, H, W, 3) and not np.array_equal(want, want2)
    for fs, ft in (("c", "c"), ("c", "f"), ("f", "c")):
        with demo.ClipRunner(model, *src.src(fs, range(K)), batch=batch) as r:
            assert np.array_equal(r.run(*drv.tar(ft)), want), (fs, ft)
            r.replace_source(1, *[p[0] for p in src.src("c", [K])])      # a compact replacement among sources of either form
            assert np.array_equal(r.run(*drv.tar(ft)), want2), (fs, ft)
