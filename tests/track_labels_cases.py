"""Face labels with a crop per frame in one pass over frames of different sizes (`tsnet_face_labels_boxes[_u8]`, csrc/track_labels.hpp;
FaceRasteriser.clip_labels(crop=(F,4))) -- shared by the CPU-emulation tier (test_track_labels.py) and the GPU tier (test_gpu_track_labels.py).
Everything is EQUALITY (torch.equal): the maps hold 0 / 1 and the operations are the single-size kernels' in the same order.

The truth of frame f is the single-crop path on frame f alone with crop f and the clip's brush, through the same library:
`clip_labels([kp[f]], crop=crops[f], bw=bw)` -- the path tests/test_raster.py, test_resize.py and test_track_crop.py pin to oracle/raster_oracle.py and
oracle/skimage_resize.py.  The small case is compared with those two oracle modules directly as well (`oracle_labels`, on the host).
C-level calls put outputs, workspace and pool between sentinels (track_crop_cases.guarded_out)."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

import paste_cases as pc
import track_crop_cases as tc
from wacv23_tsnet_amd import raster

ERR_ARG = -1
SMALL_SIZE = (64, 56)                    # (OH, OW)
# crop (h, w), (lw rows, lw columns): every kind of pass and skip meets every other inside one launch; one size twice, interleaved
SMALL_CROPS = [((60, 50), (-1, -1)),     # neither axis shrinks: no pass
               ((160, 140), (3, 3)),
               ((64, 56), (-1, -1)),     # sigma = 0: no pass
               ((80, 168), (1, 4)),
               ((72, 63), (0, 0)),       # the single weight 1.0: the identity, skipped
               ((160, 56), (3, -1)),     # rows only
               ((80, 70), (1, 1)),
               ((60, 50), (-1, -1))]
BIG = 1                                  # the (160, 140) frame: the F = 1 case
SHIFTED = 3                              # this frame's points are pushed to the right and up: several curves leave the crop, the draw clamps
SMALL_FRAMES = (0, 2, 13, 8, 3, 17, 9, 1)            # of test114
REAL_FRAMES = (0, 2, 13, 8, 3, 17, 9, 1)             # tests/test_track_crop.py LABEL_FRAMES: crops of 244 .. 250 pixels, four sizes


def expected_lw(n_in, n_out):
    sigma = max(0.0, (n_in / n_out - 1.0) / 2.0)
    return -1 if sigma <= 1e-15 else int(4.0 * sigma + 0.5)


def _test114():
    sys.path.insert(0, os.path.join(tc.ROOT, "tools"))
    import demo_clip
    return demo_clip.clip_keypoints("test114")[0]


_cache = {}


def small_case():
    """(kp (8,68,2) RELATIVE to the crops, fractional; crops (8,4); (OH, OW)): test114's faces scaled about their centre to half the crop's width"""
    if "small" not in _cache:
        src = _test114()[list(SMALL_FRAMES)]
        OH, OW = SMALL_SIZE
        kp, crops = np.empty((len(SMALL_CROPS), 68, 2)), []
        for f, ((h, w), lws) in enumerate(SMALL_CROPS):
            assert (expected_lw(h, OH), expected_lw(w, OW)) == lws, (f, h, w)
            face = src[f]
            lo, hi = face.min(0), face.max(0)
            s = min(0.5 * w / (hi[0] - lo[0]), 0.62 * h / (hi[1] - lo[1]))
            kp[f] = (face - (lo + hi) / 2) * s + np.array([w / 2, h * 0.55])
            crops.append((10 + f, 10 + f + h, 20 - f, 20 - f + w))   # min_y, max_y, min_x, max_x: the position is irrelevant to relative points
        kp[SHIFTED, :, 0] += 0.42 * SMALL_CROPS[SHIFTED][0][1]
        kp[SHIFTED, :, 1] -= 0.30 * SMALL_CROPS[SHIFTED][0][0]
        assert (kp[SHIFTED, :, 0].max() > SMALL_CROPS[SHIFTED][0][1] + 4) and (kp[SHIFTED, :, 1].min() < -4)
        kp.setflags(write=False)
        _cache["small"] = (kp, np.array(crops, np.int64), SMALL_SIZE)
    return _cache["small"]


def real_case():
    """(kp (9,68,2) in FRAME coordinates, crops (9,4), (256, 256)): the eight frames of test_track_crop.py and a ninth scaled by 2.2 (crop >= 512:
    rows and columns lw 2); bw is the first frame's, 1"""
    if "real" not in _cache:
        kp = _test114()[list(REAL_FRAMES) + [5]].copy()
        kp[8] = np.round((kp[8] - kp[8].mean(0)) * 2.2 + kp[8].mean(0))
        crops = raster.crop_coords_clip(kp)
        sides = [int(c[1] - c[0]) for c in crops]
        assert sides[:8] == [244, 246, 244, 248, 246, 250, 248, 244] and sides[8] >= 512, sides
        assert expected_lw(sides[8], 256) == 2 and expected_lw(int(crops[8, 3] - crops[8, 2]), 256) == 2
        kp.setflags(write=False)
        _cache["real"] = (kp, crops, (256, 256))
    return _cache["real"]


def truth(lib, dev, key, kp, crops, size, bw, compact, relative):
    """the per-frame loop through the single-crop path, computed once per (tier, case, bw, form) and shared (left unchanged)"""
    k = ("truth", str(dev), key, bw, compact)
    if k not in _cache:
        rs = raster.FaceRasteriser(dev, lib=lib)
        lbl, box = [], []
        for f in range(len(crops)):
            l1, b1, _ = rs.clip_labels([kp[f]], size=size, crop=tuple(int(v) for v in crops[f]), relative=relative, compact=compact, bw=bw)
            lbl.append(l1[0].cpu()); box.append(b1[0].cpu())
        _cache[k] = (torch.stack(lbl), torch.stack(box))
    return _cache[k]


def oracle_labels(kp_rel, crops, size, bw):
    """(class maps, masks) (F,OH,OW) uint8 of relative points from oracle/raster_oracle.py and oracle/skimage_resize.py, on the host"""
    k = ("oracle", bw)
    if k not in _cache:
        from oracle import raster_oracle as RO
        from oracle import skimage_resize as SR
        cls, box = [], []
        for f, c in enumerate(crops):
            h, w = int(c[1] - c[0]), int(c[3] - c[2])
            cls.append(SR.resize_bool(RO.face_edge_map(kp_rel[f], (w, h), bw), size))
            box.append(SR.resize_bool(RO.bbox_mask(kp_rel[f], (w, h)), size))
        _cache[k] = (torch.from_numpy(np.stack(cls)), torch.from_numpy(np.stack(box)))
    return _cache[k]


def check_clip(lib, dev, key, case, bw, compact, relative, frames=None):
    """clip_labels(crop=(F,4)) of a case (or of its `frames`) against the per-frame truth: values, shapes, dtypes"""
    kp, crops, size = case
    want_l, want_b = truth(lib, dev, key, kp, crops, size, bw if bw is not None else 1, compact, relative)
    idx = list(range(len(crops))) if frames is None else list(frames)
    rs = raster.FaceRasteriser(dev, lib=lib)
    lbl, box, got_crops = rs.clip_labels(list(kp[idx]), size=size, crop=crops[idx], relative=relative, compact=compact, bw=bw)
    F = len(idx)
    assert tuple(lbl.shape) == ((F,) + tuple(size) if compact else (F, 2) + tuple(size)) and tuple(box.shape) == (F,) + tuple(size)
    assert lbl.dtype == box.dtype == (torch.uint8 if compact else torch.float32) and np.array_equal(got_crops, crops[idx])
    rep = dict(case=key, bw=bw, compact=compact, F=F, differing_labels=int((lbl.cpu() != want_l[idx]).sum()), differing_masks=int((box.cpu() != want_b[idx]).sum()),
               ones=int(lbl.sum()) if compact else int(lbl[:, 1].sum()))
    print("[track_labels] " + str(rep))
    assert torch.equal(lbl.cpu(), want_l[idx]) and torch.equal(box.cpu(), want_b[idx]), rep
    assert rep["ones"] > 0 and 0 < int(box.sum()) < box.numel(), rep      # something is drawn, and not everything
    return lbl, box


# ------------------------------------------------------------------------------------------------------------------------- the C entries
class CCall:
    """The arguments of tsnet_face_labels_boxes[_u8] for relative points at given crops, laid out by hand: device key points and curves, the
    descriptors twice, pool / workspace / outputs between sentinels."""

    def __init__(self, lib, dev, kp_rel, crops, size, bw, u8):
        self.lib, self.dev, self.u8, self.bw = lib, torch.device(dev), u8, bw
        self.OH, self.OW = size
        self.F = F = len(crops)
        rs = raster.FaceRasteriser("cpu", lib=lib)
        self.desc, self.ws_len = rs._label_descriptors(np.asarray(crops, np.int64), size)
        kp = np.ascontiguousarray(kp_rel, dtype=np.float64)
        curves = np.empty((F, 34, 8))
        assert lib.tsnet_fit_face_curves(kp.ctypes.data, F, curves.ctypes.data) == 0
        self.curves = curves
        self.kp_d, self.curves_d = torch.from_numpy(kp.copy()).to(self.dev), torch.from_numpy(curves.copy()).to(self.dev)
        self.desc_d = torch.from_numpy(self.desc.copy()).to(self.dev)
        n = max(1, len(rs._wpool_host))
        self.pool_len = len(rs._wpool_host)
        self.pool_buf, self.pool = tc.guarded_out((n,), torch.float64, self.dev)
        self.pool[:self.pool_len] = torch.from_numpy(rs._wpool_host.copy()).to(self.dev)
        self.ws_buf, self.ws = tc.guarded_out((self.ws_len,), torch.uint8, self.dev)
        dt = torch.uint8 if u8 else torch.float32
        self.cls_buf, self.cls = tc.guarded_out((F, self.OH, self.OW), dt, self.dev)
        self.box_buf, self.box = tc.guarded_out((F, self.OH, self.OW), dt, self.dev)

    def reset(self):
        for b in (self.ws_buf, self.cls_buf, self.box_buf):
            b.fill_(pc.SENTINEL_BYTE)

    def written(self):
        return [not tc.untouched(b) for b in (self.cls_buf, self.box_buf, self.ws_buf)]

    def sentinels_intact(self):
        return all(pc.sentinels_intact(b) for b in (self.cls_buf, self.box_buf, self.ws_buf, self.pool_buf))

    def __call__(self, desc=None, **over):
        a = dict(kp=self.kp_d.data_ptr(), curves=self.curves_d.data_ptr(), F=self.F, host=(self.desc if desc is None else desc).ctypes.data,
                 dev=self.desc_d.data_ptr(), pool=self.pool.data_ptr(), pool_len=self.pool_len, bw=self.bw, ws=self.ws.data_ptr(), ws_len=self.ws_len,
                 OH=self.OH, OW=self.OW, cls=self.cls.data_ptr(), box=self.box.data_ptr())
        a.update(over)
        fn = self.lib.tsnet_face_labels_boxes_u8 if self.u8 else self.lib.tsnet_face_labels_boxes
        stream = torch.cuda.current_stream(self.dev).cuda_stream if self.dev.type == "cuda" else None
        return fn(a["kp"], a["curves"], a["F"], a["host"], a["dev"], a["pool"], a["pool_len"], a["bw"], a["ws"], a["ws_len"], a["OH"], a["OW"],
                  a["cls"], a["box"], stream)


def check_c_entries(lib, dev, key, bw):
    """both entries on the small case between sentinels: 0 returned, the truth's values, sentinels intact; then frame 6's curves zeroed (kind 0):
    its class map is all 0, its mask and every other frame unchanged; then each output alone (the other NULL)"""
    kp, crops, size = small_case()
    rep = []
    for u8 in (False, True):
        want_l, want_b = truth(lib, dev, key, kp, crops, size, bw, True, True)
        c = CCall(lib, dev, kp, crops, size, bw, u8)
        rc = c()
        assert rc == 0, (rc, lib.tsnet_op_last_error().decode())
        got_l, got_b = c.cls.cpu().to(torch.uint8), c.box.cpu().to(torch.uint8)
        rep.append(dict(u8=u8, bw=bw, differing_labels=int((got_l != want_l).sum()), differing_masks=int((got_b != want_b).sum()), sentinels=c.sentinels_intact()))
        assert c.sentinels_intact(), rep
        assert torch.equal(got_l, want_l) and torch.equal(got_b, want_b), rep
        assert set(np.unique(c.cls.cpu().numpy()).tolist()) == {0, 1}
        c.reset()
        c.curves_d[6] = 0
        assert c() == 0 and c.sentinels_intact()
        got_l, got_b = c.cls.cpu().to(torch.uint8), c.box.cpu().to(torch.uint8)
        keep = [f for f in range(len(crops)) if f != 6]
        assert int(got_l[6].sum()) == 0 and int(want_l[6].sum()) > 0 and torch.equal(got_l[keep], want_l[keep]) and torch.equal(got_b, want_b)
        c.curves_d.copy_(torch.from_numpy(c.curves))
        c.reset()
        assert c(box=None, kp=None) == 0 and c.written() == [True, False, True] and torch.equal(c.cls.cpu().to(torch.uint8), want_l)
        c.reset()
        assert c(cls=None, curves=None) == 0 and c.written() == [False, True, True] and torch.equal(c.box.cpu().to(torch.uint8), want_b)
        assert c.sentinels_intact()
    return rep


# ------------------------------------------------------------------------------------------------------------------------- refusals
# Five frames of the small case; one refusal per cause.  cause: (frame named or None, change of the HOST descriptors or None, replaced arguments)
REFUSAL_FRAMES = (6, 0, 1, 4, 3)         # (80, 70) | (60, 50) | (160, 140) | (72, 63) | (80, 168)


def _set(f, col, value):
    def change(d, c):
        d[f, col] = value(d, c) if callable(value) else value
    return change


REFUSALS = {
    "F_zero": (None, None, dict(F=0)),
    "F_beyond_the_grid": (None, None, dict(F=32768)),
    "both_outputs_null": (None, None, dict(cls=None, box=None)),
    "null_curves": (None, None, dict(curves=None)),
    "null_keypoints": (None, None, dict(kp=None)),
    "bw_zero": (None, None, dict(bw=0)),
    "OH_zero": (None, None, dict(OH=0)),
    "OW_negative": (None, None, dict(OW=-3)),
    "h_zero": (2, _set(2, 0, 0), {}),
    "w_negative": (2, _set(2, 1, -140), {}),
    "lw_below": (2, _set(2, 3, -2), {}),
    "lw_above": (2, _set(2, 5, 64), {}),
    "lw_on_an_axis_that_does_not_shrink": (1, _set(1, 3, 0), {}),
    "lw_not_of_the_size_pair": (2, _set(2, 5, 4), {}),
    "half_kernel_ends_beyond_the_pool": (2, None, dict(pool_len=lambda d, c: int(d[2, 4]) + 3)),        # frame 2's rows kernel has 4 entries
    "half_kernel_offset_negative": (4, _set(4, 6, -1), {}),
    "regions_overlap": (2, _set(2, 2, lambda d, c: int(d[1, 2]) + 5), {}),
    "region_overlaps_the_pairs": (0, _set(0, 2, 8), {}),
    "region_ends_beyond_the_workspace": (2, None, dict(ws_len=lambda d, c: int(d[3, 2]) - 1)),           # frame 2's region ends where frame 3's begins
}


def check_refusal(lib, dev, u8, cause):
    """The call is good without the fault and TSNET_ERR_ARG with it; outputs and workspace are untouched, the message names the frame."""
    frame, change, over = REFUSALS[cause]
    kp, crops, size = small_case()
    idx = list(REFUSAL_FRAMES)
    c = CCall(lib, dev, kp[idx], crops[idx], size, 1, u8)
    assert c() == 0 and c.written() == [True, True, True], cause
    c.reset()
    bad = c.desc.copy()
    if change is not None:
        change(bad, c)
    over = {k: (v(c.desc, c) if callable(v) else v) for k, v in over.items()}
    rc = c(bad, **over)
    msg = lib.tsnet_op_last_error().decode()
    assert rc == ERR_ARG, (cause, rc, msg)
    assert msg.startswith("face_labels_boxes"), (cause, msg)
    if frame is not None:
        assert f"frame {frame}:" in msg, (cause, msg)
    assert c.written() == [False, False, False] and c.sentinels_intact(), cause
    return dict(cause=cause, u8=u8, rc=rc, message=msg)
