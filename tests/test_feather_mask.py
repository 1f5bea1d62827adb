"""Feathered paste masks on the device (tsnet_blur_mask, tsnet_gaussian_box_params, FrameLoader.feather_mask / feather_inset,
paste*(feather=), ClipRunner.run(paste_feather=), csrc/mask_blur.hpp) -- CPU-emulation tier.  Everything is EQUALITY:
  * live Pillow's Image.filter(ImageFilter.GaussianBlur(r)) equals the numpy restatement of feather_cases.py (the contract) on every case;
  * tsnet_gaussian_box_params gives the restatement's constants;
  * every case through the C entry (output and intermediate between sentinels) and through FrameLoader.feather_mask;
  * the exact-support properties of three box passes; one argument-error test per cause, each asserting nothing was written;
  * paste(feather=) against paste(mask=feather_mask(...)) against live Pillow, ClipRunner against the hand-written sequence, the tools' flags.
The GPU tier (test_gpu_feather_mask.py) runs the same cases through the HIP library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter

import compact_cases as cc
import feather_cases as fc
import helpers as Hh
import paste_cases as pc
from wacv23_tsnet_amd import demo, frames

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
ALL_RADII = fc.RADII + (100,)


@pytest.mark.parametrize("cid", fc.IDS)
def test_pillow_equals_the_restatement(cid):
    e = fc.expected(cid)
    got = fc.expect_pillow(np.array(e["m"]), e["radius"], e["binary"])
    assert np.array_equal(got, e["want"]), (cid, int((got != e["want"]).sum()), fc.PIL_NOTE)
    if e["kind"] == "const255":
        assert (e["want"] == 255).all()                                     # the ww / fw rounding loses nothing
    elif fc.as_pair(e["radius"]) == (0, 0):
        assert np.array_equal(e["want"], e["m"])                            # a copy
    elif e["m"].shape[1] > 1:
        assert not np.array_equal(e["want"], np.where(e["m"] != 0, 255, 0) if e["binary"] else e["m"])     # the case changes something


def test_double_arithmetic_gives_other_constants():
    """the float32 pitfall: at r = 1 the box radius is 0.25 in exact arithmetic, and Pillow's float chain lands beside it"""
    r, ww, fw = fc.box_params(1)
    assert r == 0 and (ww, fw) != (int((1 << 24) / 1.5), ((1 << 24) - int((1 << 24) / 1.5)) // 2)


def _params_c(lib, r, passes=3):
    br, ww, fw = C.c_int(-7), C.c_uint(7), C.c_uint(7)
    rc = lib.tsnet_gaussian_box_params(r, passes, C.byref(br), C.byref(ww), C.byref(fw))
    return rc, (br.value, ww.value, fw.value)


@pytest.mark.parametrize("r", ALL_RADII + (0, 7.5, 3, 8))
def test_box_params_equal_the_restatement(emu_lib, r):
    rc, got = _params_c(emu_lib, r)
    assert rc == 0 and got == fc.box_params(r), (r, got, fc.box_params(r))
    assert frames.FrameLoader("cpu", lib=emu_lib).feather_inset(r) == 3 * (got[0] + 1) + 1


def test_box_params_refusals(emu_lib):
    for r, passes in ((-1.0, 3), (float("nan"), 3), (float("inf"), 3), (1.0, 0), (1.0, -2)):
        rc, got = _params_c(emu_lib, r, passes)
        assert rc == -1 and got == (-7, 7, 7), (r, passes)
        assert emu_lib.tsnet_op_last_error().decode().startswith("gaussian_box_params")
    assert emu_lib.tsnet_gaussian_box_params(1.0, 3, None, None, None) == -1


@pytest.mark.parametrize("cid", fc.IDS)
def test_cases_emulated(emu_lib, cid):
    fc.check_case(emu_lib, "cpu", frames.FrameLoader("cpu", lib=emu_lib), cid, routes=(0, 1))


@pytest.mark.parametrize("r", ALL_RADII)
def test_exact_support(emu_lib, r):
    """three passes of a box of radius `radius` (+ 1 for the fractional taps) reach 3 (radius + 1) pixels and no farther: zeros beyond that
    distance from the rectangle, 255 deeper than that inside it, and a rectangle shrunk by feather_inset leaves its box's outer ring at 0"""
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    reach = 3 * (fc.box_params(r)[0] + 1)
    inset = ld.feather_inset(r)
    assert inset == reach + 1
    side = 2 * inset + 2 * reach + 3
    if side + 2 > fc.MAX_SIDE:                                              # r = 100: the three regions do not fit one image; one side at a time,
        W = reach + 5                                                      # against the image's end, which clamping makes a constant continuation
        lo = ld.feather_mask(None, r, size=(1, 2, W), rect=(0, 0, 2, 2))[0].numpy()
        assert (lo[:, reach + 2:] == 0).all() and lo[0, 2] > 0
        hi = ld.feather_mask(None, r, size=(1, 2, W), rect=(1, 0, W, 2))[0].numpy()
        assert (hi[:, reach + 1:] == 255).all() and hi[0, 1] < 255
        ring = ld.feather_mask(None, r, size=(1, 2, inset + 3), rect=(inset, 0, inset + 3, 2))[0].numpy()
        assert (ring[:, 0] == 0).all() and ring[0, inset] > 0
        return
    H, W = side, side + 2
    rect = (inset, inset, W - inset, H - inset)
    got = ld.feather_mask(None, r, size=(1, H, W), rect=rect)[0].numpy()
    ref = np.zeros((1, H, W), np.uint8)
    ref[:, rect[1]:rect[3], rect[0]:rect[2]] = 255
    assert np.array_equal(got, fc.expect_numpy(ref, r)[0])
    far = np.ones((H, W), bool)
    far[rect[1] - reach:rect[3] + reach, rect[0] - reach:rect[2] + reach] = False       # farther than `reach` from the rectangle along an axis
    assert far.any() and (got[far] == 0).all()
    ring = np.ones((H, W), bool); ring[1:-1, 1:-1] = False
    assert (got[ring] == 0).all()
    deep = got[rect[1] + reach:rect[3] - reach, rect[0] + reach:rect[2] - reach]
    assert deep.size > 0 and (deep == 255).all()
    assert 0 < int(got[rect[1], rect[0]]) < 255                                           # and a soft edge in between


SHAPE = (2, 20, 30)
ARG_ERRORS = {
    "out_null": (dict(out=None), "null"),
    "tmp_null": (dict(tmp=None), "null"),
    "F_zero": (dict(F=0), "shape"),
    "H_zero": (dict(H=0), "shape"),
    "W_negative": (dict(W=-3), "shape"),
    "H_over_the_limit": (dict(H=fc.MAX_SIDE + 1), "kMbMaxSide"),
    "W_over_the_limit": (dict(W=fc.MAX_SIDE + 1), "kMbMaxSide"),
    "radius_negative": (dict(rx=-0.5), "radius"),
    "radius_nan": (dict(ry=float("nan")), "radius"),
    "rect_empty": (dict(src=None, rect=(C.c_int * 4)(5, 5, 5, 9)), "rectangle"),
    "rect_outside": (dict(src=None, rect=(C.c_int * 4)(5, 5, 31, 9)), "rectangle"),
    "rect_negative": (dict(src=None, rect=(C.c_int * 4)(-1, 5, 9, 9)), "rectangle"),
    "in_and_rect_null": (dict(src=None, rect=None), "neither"),
    "route_unknown": (dict(flags=2 << 8), "route"),
    "flag_unknown": (dict(flags=2), "flag"),
}


@pytest.mark.parametrize("cause", list(ARG_ERRORS))
def test_argument_errors_write_nothing(emu_lib, cause):
    over, word = ARG_ERRORS[cause]
    src = torch.from_numpy(fc.make_input("errors", SHAPE, "random"))
    obuf, out = fc.guarded(SHAPE, "cpu")
    tbuf, tmp = fc.guarded(SHAPE, "cpu")
    assert fc.blur_c(emu_lib, src, SHAPE, None, 2.0, 0, out, tmp) == 0      # the call is good without the fault ...
    assert not fc.untouched(obuf) and fc.sentinels_intact(obuf)
    obuf.fill_(fc.SENTINEL_BYTE); tbuf.fill_(fc.SENTINEL_BYTE)
    assert fc.blur_c(emu_lib, src, SHAPE, None, 2.0, 0, out, tmp, **over) == -1, cause       # ... and TSNET_ERR_ARG with it
    msg = emu_lib.tsnet_op_last_error().decode()
    assert msg.startswith("blur_mask") and word in msg, (cause, msg)
    assert fc.untouched(obuf) and fc.untouched(tbuf), cause


def test_aliased_output_is_refused(emu_lib):
    src = torch.from_numpy(fc.make_input("alias", SHAPE, "random"))
    keep = src.clone()
    tbuf, tmp = fc.guarded(SHAPE, "cpu")
    assert fc.blur_c(emu_lib, src, SHAPE, None, 2.0, 0, src, tmp) == -1 and fc.blur_c(emu_lib, src, SHAPE, None, 2.0, 0, tmp, tmp) == -1
    assert torch.equal(src, keep) and fc.untouched(tbuf)


def test_feather_mask_value_errors(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    m = np.zeros(SHAPE, np.uint8)
    for args, kw in (((None, 2), {}), ((None, 2), dict(size=SHAPE)), ((None, 2), dict(rect=(1, 1, 5, 5))), ((m.astype(np.float32), 2), {}), ((m[0], 2), {}),
                     ((m, -1), {}), ((None, 2), dict(size=SHAPE, rect=(5, 5, 5, 9))), ((np.zeros((1, 513, 4), np.uint8), 2), {})):
        with pytest.raises(ValueError):
            ld.feather_mask(*args, **kw)
    with pytest.raises(ValueError):
        ld.feather_inset(-2)


def test_workspace_is_kept_between_calls(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    m = fc.make_input("keep", SHAPE, "random")
    a = ld.feather_mask(m, 2)
    ws = ld._feather_tmp.data_ptr()
    b = ld.feather_mask(m[:1], (2, 2))
    assert ld._feather_tmp.data_ptr() == ws and torch.equal(a[:1], b) and a.data_ptr() != b.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------- paste integration
def _pillow_feathered_paste(fr, gen, boxes, src_box, r, inset):
    """rectangle image -> GaussianBlur -> crop / resize / paste, frame by frame, in Pillow alone"""
    F, GH, GW, _ = gen.shape
    sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, GW, GH)
    rect = np.zeros((GH, GW), np.uint8)
    rect[sy0 + inset:sy1 - inset, sx0 + inset:sx1 - inset] = 255
    m = Image.fromarray(rect, "L").filter(ImageFilter.GaussianBlur(r))
    out = []
    for f in range(F):
        x0, y0, x1, y1 = boxes[f]
        frame = Image.fromarray(fr[f])
        g = Image.fromarray(gen[f]).crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0))
        frame.paste(g, (x0, y0), m.crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0)))
        out.append(np.asarray(frame))
    return np.stack(out)


PASTE = {   # frame (h, w), gen (GH, GW), src_box, box or (F,4) boxes, radius
    "face_one_box": ((90, 120), (64, 64), None, (21, 7, 95, 81), 3.7),
    "face_box_per_frame": ((90, 120), (64, 64), None, [(21, 7, 95, 81), (-9, 12, 60, 83)], 1.5),
    "pose_src_box": ((120, 160), (64, 64), (16, 0, 48, 64), (50, -8, 112, 110), 1),
}


@pytest.mark.parametrize("name", list(PASTE))
def test_paste_with_feather(emu_lib, name):
    (h, w), (GH, GW), src_box, box, r = PASTE[name]
    F = 2
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr, gen = pc.make_inputs(name, ((h, w), F, (GH, GW), src_box, box))
    inset = ld.feather_inset(r)
    sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, GW, GH)
    mask = ld.feather_mask(None, r, size=(F, GH, GW), rect=(sx0 + inset, sy0 + inset, sx1 - inset, sy1 - inset))
    per_frame = np.ndim(box) == 2
    if name == "pose_src_box":
        S = GH
        crop, img_size = box, (sx1 - sx0, sy1 - sy0)
        got = ld.paste_pose(gen, fr, crop, img_size=img_size, feather=r)
        assert (S - img_size[0]) // 2 == sx0
    elif per_frame:
        got = ld.paste_face(gen, fr, [(b[1], b[3], b[0], b[2]) for b in box], feather=r)
    else:
        got = ld.paste_face(gen, fr, (box[1], box[3], box[0], box[2]), feather=r)
    want = ld.paste(gen, fr, box, src_box=src_box, mask=mask)
    assert torch.equal(got, want) and torch.equal(ld.paste(gen, fr, box, src_box=src_box, feather=r), want)
    boxes = box if per_frame else [box] * F
    pil = _pillow_feathered_paste(fr, gen, boxes, src_box, r, inset)
    assert np.array_equal(got.numpy(), pil), (name, int((got.numpy() != pil).sum()), fc.PIL_NOTE)
    assert not torch.equal(got, ld.paste(gen, fr, box, src_box=src_box))    # and not the hard seam


def test_feather_of_a_given_mask(emu_lib):
    """feather= with a mask blurs the mask: one of 0 / 1 as 0 / 255, any other as it is"""
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr, gen = pc.make_inputs("given", ((90, 120), 2, (64, 64), None, None))
    box = (21, 7, 95, 81)
    m01 = fc.make_input("given", (2, 64, 64), "binary01")
    got = ld.paste(gen, fr, box, mask=m01, feather=2)
    assert torch.equal(got, ld.paste(gen, fr, box, mask=torch.from_numpy(fc.expect_numpy(m01, 2, binary=True))))
    mb = pc.make_mask("given", "bands", 2, 64, 64)
    got = ld.paste(gen, fr, box, mask=mb, feather=(2, 0))
    assert torch.equal(got, ld.paste(gen, fr, box, mask=torch.from_numpy(fc.expect_numpy(mb, (2, 0)))))


def test_feather_none_is_the_existing_call(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr, gen = pc.make_inputs("none", ((90, 120), 2, (64, 64), None, None))
    box = (21, 7, 95, 81)
    mask = pc.make_mask("none", "bands", 2, 64, 64)
    assert np.array_equal(ld.paste(gen, fr, box, feather=None).numpy(), pc.expect_numpy(fr, gen, box))
    assert np.array_equal(ld.paste(gen, fr, box, mask=mask, feather=None).numpy(), pc.expect_numpy(fr, gen, box, None, mask))
    assert ld._feather_tmp is None and "feather_mask" not in ld._held      # nothing of the feather path ran


def test_box_too_small_for_its_inset(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr, gen = pc.make_inputs("small", ((90, 120), 1, (64, 64), None, None))
    inset = ld.feather_inset(12.25)
    assert 2 * inset >= 32
    with pytest.raises(ValueError, match=rf"{inset} x {inset}.*32 x 64"):
        ld.paste(gen, fr, (21, 7, 95, 81), src_box=(16, 0, 48, 64), feather=12.25)
    ld.paste(gen, fr, (21, 7, 95, 81), src_box=(16, 0, 48, 64), feather=1)


# ------------------------------------------------------------------------------------------------------------------------- the clip harness
K, H, W = 2, 32, 32


class _EmuModel:
    """what demo.ClipRunner asks of a model, on the emulator (test_compact_inputs.py's narrow net)"""

    def __init__(self, lib):
        self.lib, self.n_source = lib, K
        self.cfg, self.sd = cc.narrow_net(L=2, n_source=K)

    def _device(self):
        return torch.device("cpu")

    def _new_engine(self, batch):
        return Hh.make_engine(self.cfg, self.sd, H, W, batch, "cpu", lib=self.lib)


def test_clip_runner_feathers_its_paste(emu_lib):
    """3 driving frames at batch 2 (a ragged last group): "box", "bbox" with float32 and with compact tar_bboxs, and a given mask, each equal
    to the hand-written sequence on the runner's own bytes"""
    r = 1.5
    src, drv = cc.Inputs(2, K, 1, H, W, seed=40), cc.Inputs(2, 1, 3, H, W, seed=41)
    video = np.random.default_rng(9).integers(0, 256, (3, 50, 60, 3), dtype=np.uint8)
    pbox = (-5, 8, 41, 48)
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    given = pc.make_mask("clip", "bands", 3, H, W)
    with demo.ClipRunner(_EmuModel(emu_lib), *src.src("f", range(K)), batch=2) as runner:
        small = runner.run(*drv.tar("f"))
        kw = dict(paste_into=video, paste_box=pbox, paste_feather=r)
        box = runner.run(*drv.tar("f"), **kw)
        bbox_f = runner.run(*drv.tar("f"), paste_feather_from="bbox", **kw)
        bbox_c = runner.run(*drv.tar("c"), paste_feather_from="bbox", **kw)
        blurred = runner.run(*drv.tar("f"), paste_mask=torch.from_numpy(given), **kw)
        with pytest.raises(ValueError):
            runner.run(*drv.tar("f"), paste_feather=r)
        with pytest.raises(ValueError):
            runner.run(*drv.tar("f"), paste_feather_from="face", **kw)
    assert np.array_equal(box, ld.paste(small, video, pbox, feather=r).numpy())
    tb = drv.tar("c")[1]
    assert tb.dtype == torch.uint8 and int(tb.max()) == 1
    want = ld.paste(small, video, pbox, mask=ld.feather_mask(tb, r, binary=True)).numpy()
    assert np.array_equal(bbox_f, want) and np.array_equal(bbox_c, want) and not np.array_equal(want, box)
    assert np.array_equal(want, pc.expect_numpy(video, small, pbox, None, fc.expect_numpy(tb.numpy(), r, binary=True)))
    assert np.array_equal(blurred, pc.expect_numpy(video, small, pbox, None, fc.expect_numpy(given, r)))


@pytest.mark.parametrize("tool", ["demo_clip", "demo_pose_clip"])
def test_tools_refuse_feather_without_paste_back(tool, monkeypatch, capsys):
    mod = __import__(tool)
    for extra in (["--feather", "8"], ["--feather-from", "bbox"], ["--paste-back", "--feather-from", "bbox"]):
        monkeypatch.setattr(sys, "argv", [tool + ".py"] + extra)
        with pytest.raises(SystemExit) as e:
            mod.main()
        assert e.value.code == 2 and "--feather" in capsys.readouterr().err
