"""Generated frames pasted back into the video on the device (tsnet_paste_frames, FrameLoader.paste*, csrc/paste.hpp) -- CPU-emulation tier.
Everything is EQUALITY with the numpy restatement of paste_cases.py (the contract), which in turn is held equal to live Pillow here:
  * the two expected-value functions agree on every case (if they do not, the case list or the restatement is wrong, not the kernel);
  * every case through the C entry, into a buffer with sentinels on both sides, and through FrameLoader.paste;
  * one argument-error test per cause, each asserting nothing was written;
  * the round trip prepare -> paste, inplace against the clone, paste_face / paste_pose against paste, the ValueErrors.
The GPU tier (test_gpu_paste_frames.py) runs the same cases through the HIP library."""
import numpy as np
import pytest
import torch

import paste_cases as pc
from wacv23_tsnet_amd import frames

VARIANTS = pc.variants()
IDS = [v[0] for v in VARIANTS]


@pytest.mark.parametrize("vid", IDS)
def test_pillow_equals_the_restatement(vid):
    e = pc.expected(vid)
    got = pc.expect_pillow(np.array(e["fr"]), np.array(e["gen"]), e["box"], e["src_box"], None if e["mask"] is None else np.array(e["mask"]))
    assert np.array_equal(got, e["want"]), (vid, int((got != e["want"]).sum()), pc.PIL_NOTE)
    if vid != "box_outside":
        assert not np.array_equal(e["want"], e["fr"])                       # the case writes something


def test_mask_ends_are_the_frame_and_the_paste():
    """the blend gives the frame's byte at m = 0 and the resized byte at m = 255, on every byte pair"""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for m, want in ((0, a), (255, b)):
        t = b * m + a * (255 - m) + 128
        assert np.array_equal((t + (t >> 8)) >> 8, want)


@pytest.mark.parametrize("vid", IDS)
def test_cases_emulated(emu_lib, vid):
    pc.check_variant(emu_lib, "cpu", frames.FrameLoader("cpu", lib=emu_lib), vid)


def test_too_steep_is_refused_emulated(emu_lib):
    pc.check_too_steep(emu_lib, "cpu", frames.FrameLoader("cpu", lib=emu_lib))


def _setup(lib, F=1, hw=(40, 50), g=(24, 20)):
    ld = frames.FrameLoader("cpu", lib=lib)
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (F,) + hw + (3,), dtype=np.uint8)
    gen = torch.from_numpy(rng.integers(0, 256, (F,) + g + (3,), dtype=np.uint8))
    buf, view = pc.guarded(fr, "cpu")
    return ld, fr, gen, buf, view


BOX = (5, 6, 35, 30)                                                        # 20 x 24 -> 30 x 24: horizontal pass only
BOX2 = (5, 6, 35, 36)                                                       # 20 x 24 -> 30 x 30: both passes
ARG_ERRORS = {
    "F_zero": (BOX2, dict(F=0)),
    "gen_null": (BOX2, dict(gen=None)),
    "frames_null": (BOX2, dict(frames=None)),
    "box_empty_x": ((5, 6, 5, 30), {}),
    "box_empty_y": ((5, 9, 35, 3), {}),
    "src_empty": (BOX2, dict(sx0=7, sx1=7)),
    "src_negative": (BOX2, dict(sx0=-1)),
    "src_beyond_width": (BOX2, dict(sx1=21)),
    "src_beyond_height": (BOX2, dict(sy1=25)),
    "xtaps_narrow": (BOX2, dict(xt=3)),
    "ytaps_wide": (BOX2, dict(yt=7)),
    "x_table_missing": (BOX2, dict(xk=None)),
    "y_table_missing": (BOX2, dict(yf=None)),
}


@pytest.mark.parametrize("cause", list(ARG_ERRORS))
def test_argument_errors_write_nothing(emu_lib, cause):
    box, over = ARG_ERRORS[cause]
    ld, fr, gen, buf, view = _setup(emu_lib)
    assert pc.paste_c(emu_lib, ld, gen, None, view, BOX2, None) == 0        # the call is good without the fault ...
    assert not torch.equal(view, torch.from_numpy(fr))
    view.copy_(torch.from_numpy(fr))
    assert pc.paste_c(emu_lib, ld, gen, None, view, box, None, **over) == -1, cause       # ... and TSNET_ERR_ARG with it
    assert emu_lib.tsnet_op_last_error().decode().startswith("paste_frames"), cause
    assert torch.equal(view, torch.from_numpy(fr)) and pc.sentinels_intact(buf), cause


def test_skipped_axis_does_not_read_its_tables(emu_lib):
    ld, fr, gen, buf, view = _setup(emu_lib)
    assert pc.paste_c(emu_lib, ld, gen, None, view, BOX, None, yf=None, yc=None, yk=None, yt=0) == 0
    assert np.array_equal(view.numpy(), pc.expect_numpy(fr, gen.numpy(), BOX)) and pc.sentinels_intact(buf)


def test_round_trip_prepare_then_paste(emu_lib):
    """prepare(frame, box, (cw, ch), as_bytes=True) turned back to RGB and pasted at the same box leaves the frame as it was inside
    box ∩ frame -- both passes skipped both ways; the box leaves the frame, where crop read zeros that the paste must drop"""
    ld, fr, _, _, _ = _setup(emu_lib, F=2)
    box = (-7, 11, 33, 47)
    planes = ld.prepare(fr, box, (box[2] - box[0], box[3] - box[1]), as_bytes=True)               # (F,3,ch,cw) B, G, R
    gen = planes.flip(1).permute(0, 2, 3, 1).contiguous()
    noise = np.random.default_rng(6).integers(0, 256, fr.shape, dtype=np.uint8)
    y0, y1, x1 = 11, 40, 33
    got = ld.paste(gen, noise, box).numpy()
    assert np.array_equal(got[:, y0:y1, :x1], fr[:, y0:y1, :x1])
    keep = np.ones(fr.shape[1:3], bool); keep[y0:y1, :x1] = False
    assert np.array_equal(got[:, keep], noise[:, keep])
    assert np.array_equal(ld.paste(gen, fr, box).numpy(), fr)


def test_inplace_against_the_clone(emu_lib):
    ld, fr, gen, _, _ = _setup(emu_lib, F=2)
    t = torch.from_numpy(fr.copy())
    out = ld.paste(gen, t, BOX2)
    assert out.data_ptr() != t.data_ptr() and torch.equal(t, torch.from_numpy(fr)) and not torch.equal(out, t)
    out2 = ld.paste(gen, t, BOX2, inplace=True)
    assert out2.data_ptr() == t.data_ptr() and torch.equal(t, out)
    assert np.array_equal(out.numpy(), pc.expect_numpy(fr, gen.numpy(), BOX2))


def test_paste_face_and_pose_spellings(emu_lib):
    ld, fr, gen, _, _ = _setup(emu_lib, F=2)
    mask = torch.from_numpy(pc.make_mask("spell", "bands", 2, 24, 20))
    assert torch.equal(ld.paste_face(gen, fr, [6, 36, 5, 35]), ld.paste(gen, fr, (5, 6, 35, 36)))
    assert torch.equal(ld.paste_face(gen, fr, [6, 36, 5, 35], mask=mask), ld.paste(gen, fr, (5, 6, 35, 36), mask=mask))
    sq = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (2, 32, 32, 3), dtype=np.uint8))
    crop = (3, -4, 27, 38)
    assert torch.equal(ld.paste_pose(sq, fr, crop, img_size=(16, 32)), ld.paste(sq, fr, crop, src_box=(8, 0, 24, 32)))
    assert torch.equal(ld.paste_pose(sq, fr, crop, img_size=(32, 20)), ld.paste(sq, fr, crop, src_box=(0, 6, 32, 26)))
    big = torch.zeros((2, 256, 256, 3), dtype=torch.uint8)
    assert torch.equal(ld.paste_pose(big, fr, crop), ld.paste(big, fr, crop, src_box=(64, 0, 192, 256)))
    with pytest.raises(ValueError):
        ld.paste_pose(gen, fr, crop)                                        # not the padded square of img_size


def test_value_errors(emu_lib):
    ld, fr, gen, _, _ = _setup(emu_lib, F=2)
    bad = [dict(gen=gen.float()), dict(frames=fr.astype(np.float32)), dict(gen=gen[0]), dict(frames=fr[0]), dict(gen=gen[:1]),
           dict(gen=gen[..., :2]), dict(mask=torch.zeros((2, 24, 20), dtype=torch.float32)), dict(mask=torch.zeros((2, 24, 21), dtype=torch.uint8)),
           dict(mask=torch.zeros((1, 24, 20), dtype=torch.uint8)), dict(box=(5, 6, 5, 30)), dict(src_box=(0, 0, 21, 24)), dict(src_box=(4, 0, 4, 24))]
    for kw in bad:
        a = dict(gen=gen, frames=fr, box=BOX2)
        a.update(kw)
        with pytest.raises(ValueError):
            ld.paste(**a)
