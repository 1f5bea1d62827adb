"""Pasting generated frames back into the video (`tsnet_paste_frames`, FrameLoader.paste, csrc/paste.hpp), shared by the CPU-emulation tier
(test_paste_frames.py) and the GPU tier (test_gpu_paste_frames.py).  Everything is EQUALITY.

Two expected-value functions:
  (a) `expect_pillow`: live Pillow, exactly the statements of the operation --
          g = Image.fromarray(gen[f]).crop(src_box).resize((x1 - x0, y1 - y0)); m likewise from the mask ("L"); frame_f.paste(g, (x0, y0), m)
  (b) `expect_numpy`: a restatement from frames.bicubic_table -- one integer pass per axis (the horizontal one first, rounded to bytes; an axis
      that keeps its size is skipped), then the clipped copy, or with a mask the blend t = b m + a (255 - m) + 128, out = (t + (t >> 8)) >> 8.
(b) does not depend on the installed Pillow and is the contract; a disagreement of (a) alone gets PIL_NOTE.  test_paste_frames.py checks
(a) == (b) on every case on the CPU.

The destination sits in a buffer with SENTINEL bytes before and after it; the whole frame is compared (untouched pixels included) and the
sentinels too: a store outside the frames shows there."""
from __future__ import annotations

import numpy as np
import torch
from PIL import Image

from wacv23_tsnet_amd import frames

PIL_NOTE = ("live Pillow %s disagrees with the numpy restatement; if the kernel equals the restatement (the contract), this Pillow's resampler or "
            "paste differs" % Image.__version__)
SENTINEL, SENTINEL_BYTE = 4096, 0xA5

# name: (frame (h, w), F, gen (GH, GW), src_box or None, box, masks too).  The smallest shapes at which each branch can go wrong; the pose shape
# keeps its real size once.
CASES = {
    "face_274_up": ((480, 640), 2, (256, 256), None, (121, 17, 395, 291), True),            # 256 -> 274 up; F > 1 with different frames
    "face_244_down": ((480, 640), 1, (256, 256), None, (200, 100, 444, 344), False),        # 256 -> 244; 7 taps
    "pose_no_bars": ((1080, 1920), 1, (256, 256), (64, 0, 192, 256), (841, 206, 1231, 986), False),
    "leaves_left_top": ((300, 200), 2, (96, 64), None, (-20, -31, 108, 161), True),
    "leaves_right_bottom": ((300, 200), 2, (96, 64), None, (150, 200, 227, 331), False),    # a 77 x 131 box off the tile
    "frame_inside_box": ((60, 80), 1, (96, 64), None, (-30, -30, 110, 90), True),           # the box leaves on all four sides
    "skip_horizontal": ((300, 200), 1, (96, 64), None, (11, 20, 75, 170), False),
    "skip_vertical": ((300, 200), 1, (96, 64), None, (11, 20, 140, 116), False),
    "skip_both_odd_offset": ((300, 200), 2, (96, 64), None, (13, 20, 77, 116), False),      # a plain paste at an odd byte offset
    "one_pixel_wide": ((300, 200), 1, (96, 64), None, (50, 10, 51, 200), False),
    "one_pixel_high": ((300, 200), 1, (96, 64), None, (10, 50, 150, 51), False),
    "source_off_origin": ((300, 200), 1, (96, 64), (5, 7, 61, 90), (30, 40, 130, 190), True),
    "steep_21x_th2": ((64, 64), 1, (256, 32), None, (10, 10, 42, 22), False),               # 256 -> 12 rows: the launcher lowers th to 2
    "box_outside": ((60, 80), 1, (96, 64), None, (200, 10, 264, 106), False),               # returns 0, nothing changes
}
TOO_STEEP = ((64, 64), 1, (256, 32), None, (10, 10, 42, 18))                                # 256 -> 8 rows does not fit the LDS buffer: TSNET_ERR_ARG
MASK_KINDS = ("bands", "binary")


def make_inputs(name, case=None):
    """(frames (F,h,w,3), gen (F,GH,GW,3)) uint8: random bytes with hard edges, so that the negative lobes clip at both ends"""
    (h, w), F, (GH, GW), _, _ = (case if case is not None else CASES[name])[:5]
    rng = np.random.default_rng(sum(map(ord, name)))
    fr = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    gen = rng.integers(0, 256, (F, GH, GW, 3), dtype=np.uint8)
    gen[:, ::7, ::5] = 255; gen[:, 3::11, 2::9] = 0
    gen[:, GH // 3:GH // 3 + 9, :GW // 2] = 255; gen[:, GH // 3 + 9:GH // 3 + 18, :GW // 2] = 0
    return fr, gen


def make_mask(name, kind, F, GH, GW):
    rng = np.random.default_rng(sum(map(ord, name)) + len(kind))
    if kind == "bands":                                                    # random bytes with bands forced to 0 and to 255
        m = rng.integers(0, 256, (F, GH, GW), dtype=np.uint8)
        m[:, GH // 4:GH // 4 + 10] = 0
        m[:, :, GW // 2:GW // 2 + 9] = 255
        m[:, GH // 2:GH // 2 + 8, :GW // 3] = 0
        return m
    m = np.zeros((F, GH, GW), np.uint8)                                    # a binary 0 / 255 rectangle
    m[:, GH // 5:GH - GH // 6, GW // 4:GW - GW // 7] = 255
    return m


def variants():
    """[(id, case name, mask kind or None)]"""
    out = []
    for name, c in CASES.items():
        out.append((name, name, None))
        if c[5]:
            out += [(f"{name}-mask_{k}", name, k) for k in MASK_KINDS]
    return out


# ------------------------------------------------------------------------------------------------------------------------- expected values
def expect_pillow(fr, gen, box, src_box=None, mask=None):
    """(a) live Pillow"""
    x0, y0, x1, y1 = box
    F, GH, GW, _ = gen.shape
    sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, GW, GH)
    out = []
    for f in range(F):
        frame_f = Image.fromarray(fr[f])
        g = Image.fromarray(gen[f]).crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0))
        m = None if mask is None else Image.fromarray(mask[f], "L").crop((sx0, sy0, sx1, sy1)).resize((x1 - x0, y1 - y0))
        frame_f.paste(g, (x0, y0), m)
        out.append(np.asarray(frame_f))
    return np.stack(out)


def _pass(a, axis, table):
    """one integer pass of the 8-bit resampler along `axis` of a uint8 array"""
    first, count, coef = table
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((len(first),) + a.shape[1:], np.uint8)
    for o in range(len(first)):
        lo, n = int(first[o]), int(count[o])
        acc = (1 << (frames.PRECISION_BITS - 1)) + np.tensordot(coef[o, :n].astype(np.int64), a[lo:lo + n], axes=1)
        out[o] = np.clip(acc >> frames.PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_numpy(a, ow, oh):
    """a: (ch, cw) or (ch, cw, 3) uint8 -> (oh, ow[, 3]): the horizontal pass first, rounded to bytes, then the vertical one"""
    ch, cw = a.shape[:2]
    if ow != cw:
        a = _pass(a, 1, frames.bicubic_table(cw, ow))
    if oh != ch:
        a = _pass(a, 0, frames.bicubic_table(ch, oh))
    return a


def expect_numpy(fr, gen, box, src_box=None, mask=None):
    """(b) the restatement: independent of the installed Pillow"""
    x0, y0, x1, y1 = box
    F, h, w, _ = fr.shape
    GH, GW = gen.shape[1:3]
    sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, GW, GH)
    out = fr.copy()
    X0, Y0, X1, Y1 = max(x0, 0), max(y0, 0), min(x1, w), min(y1, h)
    if X0 >= X1 or Y0 >= Y1:
        return out
    for f in range(F):
        b = resize_numpy(gen[f, sy0:sy1, sx0:sx1], x1 - x0, y1 - y0)[Y0 - y0:Y1 - y0, X0 - x0:X1 - x0]
        if mask is None:
            out[f, Y0:Y1, X0:X1] = b
            continue
        m = resize_numpy(mask[f, sy0:sy1, sx0:sx1], x1 - x0, y1 - y0)[Y0 - y0:Y1 - y0, X0 - x0:X1 - x0].astype(np.int64)[:, :, None]
        t = b.astype(np.int64) * m + out[f, Y0:Y1, X0:X1].astype(np.int64) * (255 - m) + 128
        out[f, Y0:Y1, X0:X1] = ((t + (t >> 8)) >> 8).astype(np.uint8)
    return out


_expected = {}


def expected(vid):
    """{fr, gen, mask, box, src_box, want} of a variant, computed once and shared (read-only arrays)"""
    if vid not in _expected:
        _, name, kind = next(v for v in variants() if v[0] == vid)
        (h, w), F, (GH, GW), src_box, box, _ = CASES[name]
        fr, gen = make_inputs(name)
        mask = None if kind is None else make_mask(name, kind, F, GH, GW)
        want = expect_numpy(fr, gen, box, src_box, mask)
        for a in (fr, gen, want) + (() if mask is None else (mask,)):
            a.setflags(write=False)
        _expected[vid] = dict(fr=fr, gen=gen, mask=mask, box=box, src_box=src_box, want=want)
    return _expected[vid]


# ------------------------------------------------------------------------------------------------------------------------- the device side
def guarded(fr, dev):
    """the frames inside a larger allocation: SENTINEL bytes | frames | SENTINEL bytes -> (buffer, view of the frames)"""
    n = fr.size
    buf = torch.full((n + 2 * SENTINEL,), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    view = buf[SENTINEL:SENTINEL + n].view(fr.shape)
    view.copy_(torch.from_numpy(np.array(fr)))
    return buf, view


def sentinels_intact(buf):
    b = buf.cpu()
    return bool((b[:SENTINEL] == SENTINEL_BYTE).all()) and bool((b[-SENTINEL:] == SENTINEL_BYTE).all())


def tables(ld, n_in, n_out):
    """(first, count, coef pointers, taps) of an axis from the loader's cache"""
    t, taps = ld._axis(n_in, n_out)
    return [t.data_ptr() + 4 * off for off in (0, n_out, 2 * n_out)] + [taps]


def paste_c(lib, ld, gen_d, mask_d, view, box, src_box, stream=None, **over):
    """the C entry on device tensors, writing into `view`; `over` replaces single arguments (the error tests)"""
    F, GH, GW, _ = gen_d.shape
    sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, GW, GH)
    x0, y0, x1, y1 = box
    xf, xc, xk, xt = tables(ld, max(sx1 - sx0, 1), max(x1 - x0, 1))
    yf, yc, yk, yt = tables(ld, max(sy1 - sy0, 1), max(y1 - y0, 1))
    a = dict(gen=gen_d.data_ptr(), mask=None if mask_d is None else mask_d.data_ptr(), F=F, GH=GH, GW=GW, sx0=sx0, sy0=sy0, sx1=sx1, sy1=sy1,
             xf=xf, xc=xc, xk=xk, xt=xt, yf=yf, yc=yc, yk=yk, yt=yt, frames=view.data_ptr(), h=view.shape[1], w=view.shape[2],
             x0=x0, y0=y0, x1=x1, y1=y1)
    a.update(over)
    return lib.tsnet_paste_frames(a["gen"], a["mask"], a["F"], a["GH"], a["GW"], a["sx0"], a["sy0"], a["sx1"], a["sy1"], a["xf"], a["xc"], a["xk"], a["xt"],
                                  a["yf"], a["yc"], a["yk"], a["yt"], a["frames"], a["h"], a["w"], a["x0"], a["y0"], a["x1"], a["y1"], stream)


def check_variant(lib, dev, ld, vid):
    """one variant through the C entry (guarded buffer, in place) and through FrameLoader.paste -> report entry; asserts equality with (b)"""
    e = expected(vid)
    dev = torch.device(dev)
    want = torch.from_numpy(np.array(e["want"]))
    gen_d = torch.from_numpy(np.array(e["gen"])).to(dev)
    mask_d = None if e["mask"] is None else torch.from_numpy(np.array(e["mask"])).to(dev)
    buf, view = guarded(e["fr"], dev)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    rc = paste_c(lib, ld, gen_d, mask_d, view, e["box"], e["src_box"], stream=stream)
    assert rc == 0, (vid, rc, lib.tsnet_op_last_error().decode())
    got = view.cpu()
    rep = dict(case=vid, differing=int((got != want).sum()), sentinels=sentinels_intact(buf))
    assert rep["sentinels"], rep
    assert torch.equal(got, want), rep
    got2 = ld.paste(np.array(e["gen"]) if e["fr"].shape[0] == 1 else gen_d, np.array(e["fr"]), e["box"], src_box=e["src_box"],   # arrays and tensors
                    mask=None if e["mask"] is None else np.array(e["mask"])).cpu()
    rep["differing_loader"] = int((got2 != want).sum())
    assert torch.equal(got2, want), rep
    if e["fr"].shape[0] > 1 and vid != "box_outside":
        assert not torch.equal(got[0], got[1])
    return rep


def check_too_steep(lib, dev, ld):
    """256 -> 8 rows: refused, frame and sentinels untouched"""
    (h, w), F, (GH, GW), src_box, box = TOO_STEEP
    fr, gen = make_inputs("too_steep", TOO_STEEP)
    buf, view = guarded(fr, dev)
    rc = paste_c(lib, ld, torch.from_numpy(gen).to(dev), None, view, box, src_box)
    assert rc == -1 and "steep" in lib.tsnet_op_last_error().decode()
    assert torch.equal(view.cpu(), torch.from_numpy(fr)) and sentinels_intact(buf)
    return dict(case="too_steep", rc=rc)
