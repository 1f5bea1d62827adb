"""Tracking crops -- a box per frame in frame loading and paste-back (`tsnet_prepare_frames_boxes[_u8]`, `tsnet_paste_frames_boxes`, the (F,4)
forms of FrameLoader; csrc/frames.hpp, csrc/paste.hpp) -- shared by the CPU-emulation tier (test_track_crop.py) and the GPU tier
(test_gpu_track_crop.py).  Everything is EQUALITY.

Expected values of frame f with box f:
  (a) the numpy restatement of paste_cases.py applied per frame (`expect_prepare_numpy`, `expect_paste_numpy`) -- the contract;
  (b) live Pillow (`expect_prepare_pillow`, paste_cases.expect_pillow per frame), held equal to (a) on the CPU tier;
  (c) the existing single-box entry called on frame f alone: the batched call must give its bits.
Destinations and outputs sit between sentinels (paste_cases.guarded, `guarded_out`); whole tensors and the sentinels are compared."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch
from PIL import Image

import paste_cases as pc
from wacv23_tsnet_amd import frames
from wacv23_tsnet_amd.demo import IMG_MEAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1

# name: (frame (h, w), F, size (ow, oh), boxes (x0, y0, x1, y1))
PREPARE_CASES = {
    # output 80 x 72: two tiles in x, three tile rows at th = 32
    "prepare_mixed": ((96, 128), 6, (80, 72), [
        (10, 8, 90, 80),                 # both axes skipped
        (20, 10, 121, 97),               # both axes shrink
        (-15, -9, 50, 40),               # leaves the frame top-left; both axes grow
        (30, 20, 110, 60),               # x skipped, y grows
        (100, 70, 140, 110),             # leaves bottom-right
        (0, -100, 80, 200)]),            # 300 -> 72 rows: this frame alone lowers the launch's th to 16
}
PREPARE_VARIANTS = [("prepare_mixed", "prepare_mixed", (80, 72), False), ("prepare_mixed-square", "prepare_mixed", (40, 72), True)]
FACE_REAL_FRAMES = (0, 9, 19, 37)        # of val024

# name: (frame (h, w), F, gen (GH, GW), boxes)
PASTE_CASES = {
    "paste_mixed": ((120, 160), 6, (96, 64), [
        (13, 20, 77, 116),               # both axes skipped, at an odd offset
        (30, 10, 131, 99),
        (-20, -31, 60, 70),
        (120, 80, 197, 211),             # leaves bottom-right
        (300, 10, 364, 106),             # entirely outside: that frame comes back unchanged while the others change
        (50, 10, 51, 110)]),             # one pixel wide
    "paste_steep": ((64, 64), 2, (256, 32), [
        (10, 10, 42, 22),                # 256 -> 12 rows: th drops
        (4, 4, 36, 60)]),
    "paste_all_outside": ((60, 80), 3, (96, 64), [(200, 10, 264, 106), (-70, 5, -5, 101), (8, 60, 72, 156)]),
}
OUTSIDE = {"paste_mixed": (4,), "paste_all_outside": (0, 1, 2)}
# (id, case, src_box, mask kind)
PASTE_VARIANTS = ([("paste_mixed" + ("" if k is None else "-mask_" + k), "paste_mixed", None, k) for k in (None,) + pc.MASK_KINDS]
                  + [("paste_mixed-src_box", "paste_mixed", (5, 7, 61, 90), None), ("paste_mixed-src_box-mask_bands", "paste_mixed", (5, 7, 61, 90), "bands"),
                     ("paste_steep", "paste_steep", None, None), ("paste_all_outside", "paste_all_outside", None, None)])


def val024_keypoints():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import demo_clip
    return demo_clip.clip_keypoints("val024")[0]


def face_real_case():
    """((480, 640), 4, (256, 256), boxes): crop_coords of four frames of val024's landmarks -- 274, 270, 272 and 272 pixels, at four positions"""
    from wacv23_tsnet_amd import raster
    kp = val024_keypoints()
    c = raster.crop_coords_clip(kp[list(FACE_REAL_FRAMES)])
    boxes = [(int(r[2]), int(r[0]), int(r[3]), int(r[1])) for r in c]
    assert len({b[2] - b[0] for b in boxes}) == 3 and len(set(boxes)) == 4
    return (480, 640), 4, (256, 256), boxes


def make_frames(name, F, h, w):
    rng = np.random.default_rng(sum(map(ord, name)))
    fr = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    fr[:, ::7, ::5] = 255; fr[:, 3::11, 2::9] = 0
    fr[:, h // 3:h // 3 + 9, :w // 2] = 255; fr[:, h // 3 + 9:h // 3 + 18, :w // 2] = 0
    return fr


# ------------------------------------------------------------------------------------------------------------------------- expected values
def _geometry(size, square):
    ow, oh = size
    S = max(ow, oh)
    OH, OW = (S, S) if square else (oh, ow)
    return ow, oh, OH, OW, (OH - oh) // 2, (OW - ow) // 2


def expect_prepare_numpy(fr, boxes, size, square):
    """(a): per frame, the box's part outside the frame zero-filled, resize_numpy, resize_square's bars, RGB -> BGR: (F,3,OH,OW) BYTES"""
    F, h, w, _ = fr.shape
    ow, oh, OH, OW, pt, pl = _geometry(size, square)
    out = np.zeros((F, 3, OH, OW), np.uint8)
    for f, (x0, y0, x1, y1) in enumerate(boxes):
        crop = np.zeros((y1 - y0, x1 - x0, 3), np.uint8)
        X0, Y0, X1, Y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
        if X0 < X1 and Y0 < Y1:
            crop[Y0 - y0:Y1 - y0, X0 - x0:X1 - x0] = fr[f, Y0:Y1, X0:X1]
        out[f, :, pt:pt + oh, pl:pl + ow] = pc.resize_numpy(crop, ow, oh)[:, :, ::-1].transpose(2, 0, 1)
    return out


def expect_prepare_pillow(fr, boxes, size, square):
    """(b): frame.crop(box).resize(size), the bars, RGB -> BGR"""
    ow, oh, OH, OW, pt, pl = _geometry(size, square)
    out = np.zeros((fr.shape[0], 3, OH, OW), np.uint8)
    for f, box in enumerate(boxes):
        r = np.asarray(Image.fromarray(fr[f]).crop(tuple(box)).resize((ow, oh)))
        out[f, :, pt:pt + oh, pl:pl + ow] = r[:, :, ::-1].transpose(2, 0, 1)
    return out


def widen(planes):
    """the float form of byte planes: (float)byte - mean, one fp32 operation"""
    return planes.astype(np.float32) - np.asarray(IMG_MEAN, np.float32).reshape(1, 3, 1, 1)


def expect_paste_numpy(fr, gen, boxes, src_box=None, mask=None):
    """(a): paste_cases.expect_numpy per frame with that frame's box"""
    return np.concatenate([pc.expect_numpy(fr[f:f + 1], gen[f:f + 1], boxes[f], src_box, None if mask is None else mask[f:f + 1]) for f in range(len(boxes))])


def expect_paste_pillow(fr, gen, boxes, src_box=None, mask=None):
    return np.concatenate([pc.expect_pillow(fr[f:f + 1], gen[f:f + 1], boxes[f], src_box, None if mask is None else mask[f:f + 1]) for f in range(len(boxes))])


_cache = {}


def prepare_expected(vid):
    """{fr, boxes, size, square, want (bytes)} of a prepare variant, computed once and shared (read-only)"""
    if vid not in _cache:
        if vid == "prepare_face_real":
            (h, w), F, size, boxes = face_real_case()
            name, square = vid, False
        else:
            _, name, size, square = next(v for v in PREPARE_VARIANTS if v[0] == vid)
            (h, w), F, _, boxes = PREPARE_CASES[name]
        fr = make_frames(name, F, h, w)
        want = expect_prepare_numpy(fr, boxes, size, square)
        fr.setflags(write=False); want.setflags(write=False)
        _cache[vid] = dict(fr=fr, boxes=boxes, size=size, square=square, want=want)
    return _cache[vid]


def paste_expected(vid):
    """{fr, gen, mask, boxes, src_box, want} of a paste variant, computed once and shared (read-only)"""
    if vid not in _cache:
        _, name, src_box, kind = next(v for v in PASTE_VARIANTS if v[0] == vid)
        (h, w), F, (GH, GW), boxes = PASTE_CASES[name]
        fr, gen = pc.make_inputs(name, ((h, w), F, (GH, GW), None, None))
        mask = None if kind is None else pc.make_mask(name, kind, F, GH, GW)
        want = expect_paste_numpy(fr, gen, boxes, src_box, mask)
        for a in (fr, gen, want) + (() if mask is None else (mask,)):
            a.setflags(write=False)
        _cache[vid] = dict(name=name, fr=fr, gen=gen, mask=mask, boxes=boxes, src_box=src_box, want=want)
    return _cache[vid]


# ------------------------------------------------------------------------------------------------------------------------- the device side
def guarded_out(shape, dtype, dev):
    """an output tensor inside a larger allocation: SENTINEL bytes | tensor | SENTINEL bytes, the tensor's own bytes SENTINEL_BYTE too -> (buffer, view)"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((n + 2 * pc.SENTINEL,), pc.SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    return buf, buf[pc.SENTINEL:pc.SENTINEL + n].view(dtype).view(shape)


def untouched(buf):
    return bool((buf.cpu() == pc.SENTINEL_BYTE).all())


def _stream(dev):
    dev = torch.device(dev)
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None


def prepare_descriptors(ld, boxes, size):
    """(host (F,8), device copy, device pool) from the loader's pool"""
    ow, oh = size
    d, dd, pool, _ = ld._descriptors(np.asarray(boxes, np.int64), lambda b: ((int(b[2] - b[0]), ow), (int(b[3] - b[1]), oh)))
    return d, dd, pool


def paste_descriptors(ld, boxes, src_wh):
    cw, ch = src_wh
    d, dd, pool, _ = ld._descriptors(np.asarray(boxes, np.int64), lambda b: ((cw, int(b[2] - b[0])), (ch, int(b[3] - b[1]))))
    return d, dd, pool


def prepare_c(lib, fr_d, desc, desc_d, pool, size, square, out, stream=None, **over):
    """the C entry on device tensors, writing into `out` (uint8: the _u8 entry); `over` replaces single arguments (the error tests)"""
    F, h, w, _ = fr_d.shape
    ow, oh, OH, OW, pt, pl = _geometry(size, square)
    a = dict(frames=fr_d.data_ptr(), F=F, host=desc.ctypes.data, dev=desc_d.data_ptr(), pool=pool.data_ptr(), pool_len=pool.numel(), out=out.data_ptr())
    a.update(over)
    geom = (a["frames"], a["F"], h, w, a["host"], a["dev"], a["pool"], a["pool_len"], oh, ow, pt, pl, OH, OW)
    if out.dtype == torch.uint8:
        return lib.tsnet_prepare_frames_boxes_u8(*geom, a["out"], stream)
    m = np.asarray(IMG_MEAN, np.float32)
    return lib.tsnet_prepare_frames_boxes(*geom, (C.c_float * 3)(float(m[0]), float(m[1]), float(m[2])), a["out"], stream)


def paste_c(lib, gen_d, mask_d, view, desc, desc_d, pool, src_box, stream=None, **over):
    F, GH, GW, _ = gen_d.shape
    sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, GW, GH)
    a = dict(gen=gen_d.data_ptr(), F=F, host=desc.ctypes.data, dev=desc_d.data_ptr(), pool=pool.data_ptr(), pool_len=pool.numel(), frames=view.data_ptr())
    a.update(over)
    return lib.tsnet_paste_frames_boxes(a["gen"], None if mask_d is None else mask_d.data_ptr(), a["F"], GH, GW, sx0, sy0, sx1, sy1,
                                        a["host"], a["dev"], a["pool"], a["pool_len"], a["frames"], view.shape[1], view.shape[2], stream)


def check_prepare(lib, dev, ld, vid):
    """a prepare variant: the two C entries into guarded outputs, FrameLoader.prepare with (F,4), and (c) the single-box entry frame by frame"""
    e = prepare_expected(vid)
    dev = torch.device(dev)
    fr, boxes, size, square = np.array(e["fr"]), e["boxes"], e["size"], e["square"]
    want_b, want_f = torch.from_numpy(np.array(e["want"])), torch.from_numpy(widen(e["want"]))
    fr_d = torch.from_numpy(fr).to(dev)
    desc, desc_d, pool = prepare_descriptors(ld, boxes, size)
    rep = dict(case=vid)
    for dtype, want in ((torch.uint8, want_b), (torch.float32, want_f)):
        buf, out = guarded_out(tuple(want.shape), dtype, dev)
        rc = prepare_c(lib, fr_d, desc, desc_d, pool, size, square, out, stream=_stream(dev))
        assert rc == 0, (vid, rc, lib.tsnet_op_last_error().decode())
        got = out.cpu()
        rep[f"differing_{'u8' if dtype == torch.uint8 else 'f32'}"] = int((got != want).sum())
        assert pc.sentinels_intact(buf), rep
        assert torch.equal(got, want), rep
    for as_bytes, want in ((True, want_b), (False, want_f)):
        got = ld.prepare(fr_d if as_bytes else fr, boxes, size, square=square, as_bytes=as_bytes).cpu()     # device tensors and arrays
        assert torch.equal(got, want), (vid, as_bytes)
        for f in range(len(boxes)):                                  # (c)
            one = ld.prepare(fr[f:f + 1], boxes[f], size, square=square, as_bytes=as_bytes).cpu()
            assert torch.equal(one[0], got[f]), (vid, as_bytes, f)
    return rep


def check_paste(lib, dev, ld, vid):
    """a paste variant: the C entry into a guarded buffer, FrameLoader.paste with (F,4), and (c) the single-box entry frame by frame"""
    e = paste_expected(vid)
    dev = torch.device(dev)
    fr, gen, boxes, src_box = np.array(e["fr"]), np.array(e["gen"]), e["boxes"], e["src_box"]
    mask = None if e["mask"] is None else np.array(e["mask"])
    want = torch.from_numpy(np.array(e["want"]))
    gen_d = torch.from_numpy(gen).to(dev)
    mask_d = None if mask is None else torch.from_numpy(mask).to(dev)
    GH, GW = gen.shape[1:3]
    sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, GW, GH)
    desc, desc_d, pool = paste_descriptors(ld, boxes, (sx1 - sx0, sy1 - sy0))
    buf, view = pc.guarded(fr, dev)
    rc = paste_c(lib, gen_d, mask_d, view, desc, desc_d, pool, src_box, stream=_stream(dev))
    assert rc == 0, (vid, rc, lib.tsnet_op_last_error().decode())
    got = view.cpu()
    rep = dict(case=vid, differing=int((got != want).sum()), sentinels=pc.sentinels_intact(buf))
    assert rep["sentinels"], rep
    assert torch.equal(got, want), rep
    for f in range(len(boxes)):
        changed = not torch.equal(got[f], torch.from_numpy(fr[f]))
        assert changed == (f not in OUTSIDE.get(e["name"], ())), (vid, f)       # a frame whose box is outside comes back as it was, the others do not
    got2 = ld.paste(gen_d, fr, boxes, src_box=src_box, mask=mask).cpu()
    assert torch.equal(got2, want), vid
    for f in range(len(boxes)):                                      # (c)
        one = ld.paste(gen[f:f + 1], fr[f:f + 1], boxes[f], src_box=src_box, mask=None if mask is None else mask[f:f + 1]).cpu()
        assert torch.equal(one[0], got[f]), (vid, f)
    return rep


# ------------------------------------------------------------------------------------------------------------------------- refusals
# One per cause, the bad frame in the MIDDLE of the call (frame 2 of 5).  A cause is a change of the HOST descriptors (d), or of an argument.
BAD = 2
REFUSAL_BOXES_PREPARE = [(3, 4, 43, 40), (0, 0, 30, 30), (5, 6, 47, 41), (-4, -4, 21, 22), (10, 10, 50, 45)]      # -> 24 x 20 (ow, oh): every axis has a table
REFUSAL_BOXES_PASTE = [(3, 4, 43, 40), (0, 0, 30, 30), (5, 6, 47, 41), (-4, -4, 20, 22), (10, 10, 38, 45)]        # gen 20 x 24 (GW, GH) -> every box: every axis has a table


def _d(col, value):
    def change(d):
        d[BAD, col] = value(d) if callable(value) else value
    return change


def _empty(d):
    d[BAD, 2] = d[BAD, 0]


def _steep_prepare(d):                                               # 640 -> 20 rows, the ratio of 256 -> 8
    d[BAD, 1], d[BAD, 3] = -100, 540


REFUSALS = {
    # cause: (change of the host descriptors or None, replaced arguments, the message names the frame)
    "F_zero": (None, dict(F=0), False),
    "null_tensor": (None, dict(frames=None), False),
    "null_descriptors": (None, dict(dev=None), False),
    "empty_box": (_empty, {}, True),
    "xtaps_wrong": (_d(5, lambda d: d[BAD, 5] + 2), {}, True),
    "table_beyond_pool": (_d(6, lambda d: 10 ** 8), {}, True),
    "table_ends_beyond_pool": (None, dict(pool_len=lambda desc: int(desc[BAD, 4]) + 5), True),
    "table_missing": (_d(4, -1), {}, True),
    "too_steep": ("steep", {}, True),
}


def check_refusal(lib, dev, ld, which, cause):
    """`which`: "prepare" | "prepare_u8" | "paste".  The call is good without the fault and TSNET_ERR_ARG with it; nothing is written for any frame."""
    change, over, names_frame = REFUSALS[cause]
    dev = torch.device(dev)
    rng = np.random.default_rng(11)
    if which == "paste":
        fr = rng.integers(0, 256, (5, 48, 56, 3), dtype=np.uint8)
        gen_hw = (256, 20) if cause == "too_steep" else (24, 20)
        gen_d = torch.from_numpy(rng.integers(0, 256, (5,) + gen_hw + (3,), dtype=np.uint8)).to(dev)
        boxes = [tuple(b) for b in REFUSAL_BOXES_PASTE]
        desc, desc_d, pool = paste_descriptors(ld, boxes, (gen_hw[1], gen_hw[0]))
        buf, view = pc.guarded(fr, dev)
        call = lambda d, **o: paste_c(lib, gen_d, None, view, d, desc_d, pool, None, **o)
        written = lambda: not torch.equal(view.cpu(), torch.from_numpy(fr))
        reset = lambda: view.copy_(torch.from_numpy(fr))
    else:
        fr_d = torch.from_numpy(rng.integers(0, 256, (5, 48, 56, 3), dtype=np.uint8)).to(dev)
        boxes, size = [tuple(b) for b in REFUSAL_BOXES_PREPARE], (24, 20)
        desc, desc_d, pool = prepare_descriptors(ld, boxes, size)
        buf, out = guarded_out((5, 3, 20, 24), torch.uint8 if which == "prepare_u8" else torch.float32, dev)
        call = lambda d, **o: prepare_c(lib, fr_d, d, desc_d, pool, size, False, out, **o)
        written = lambda: not untouched(buf)
        reset = lambda: buf.fill_(pc.SENTINEL_BYTE)
    assert call(desc) == 0 and written(), (which, cause)             # the call is good without the fault ...
    reset()
    bad = desc.copy()
    if change == "steep":
        if which == "paste":
            bad[BAD, 3] = bad[BAD, 1] + 8                            # 256 -> 8 rows
            bad[BAD, 6:8] = ld._pool_axis(256, 8)
            desc_d, pool = paste_descriptors(ld, boxes, (20, 256))[1:]           # the pool grew: hand over the grown one
        else:
            _steep_prepare(bad)
            bad[BAD, 6:8] = ld._pool_axis(640, 20)
            desc_d, pool = prepare_descriptors(ld, boxes, size)[1:]
    elif change is not None:
        change(bad)
    over = {k: (v(desc) if callable(v) else v) for k, v in over.items()}
    rc = call(bad, **over)
    msg = lib.tsnet_op_last_error().decode()
    assert rc == ERR_ARG, (which, cause, rc, msg)
    assert msg.startswith("paste_frames_boxes" if which == "paste" else "prepare_frames_boxes"), (which, cause, msg)
    if names_frame:
        assert f"frame {BAD}:" in msg, (which, cause, msg)
    if cause == "too_steep":
        assert "steep" in msg, msg
    assert not written() and pc.sentinels_intact(buf), (which, cause)                # ... and nothing is written with it, for ANY frame
    return dict(which=which, cause=cause, rc=rc, message=msg)
