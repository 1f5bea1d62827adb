"""Face labels with a crop per frame in one pass over frames of different sizes (tsnet_face_labels_boxes[_u8], FaceRasteriser.clip_labels with
(F,4) crops) -- CPU-emulation tier.  Everything is EQUALITY:
  * the small case (eight frames, six sizes, every kind of Gaussian pass and skip in one launch) with bw 1 and 2, float and byte form, and the
    (160, 140) frame alone, against the single-crop path frame by frame and against the two oracle modules directly;
  * the C entries between sentinels, a frame with zeroed curves, each output alone;
  * one refusal per cause, nothing written for any frame, the frame named;
  * a DEVICE descriptor that differs from the host copy stays inside the tensors (emulation only: not something to try on a device);
  * the real-size case: the eight frames of test_track_crop.py and a ninth of more than 512 pixels;
  * pool and workspace of the rasteriser: reused when they suffice, replaced when a clip needs more.
The GPU tier (test_gpu_track_labels.py) runs the same cases through the HIP library."""
import numpy as np
import pytest
import torch

import track_labels_cases as lc
from wacv23_tsnet_amd import _lib, raster


def test_entries_are_bound(emu_lib):
    """fails without the feature: the symbols exist, in the binding list and in the library"""
    for s in ("tsnet_face_labels_boxes", "tsnet_face_labels_boxes_u8"):
        assert s in _lib.ABI_SYMBOLS and hasattr(emu_lib, s)


@pytest.mark.parametrize("bw", [1, 2])
def test_c_entries_on_the_small_case(emu_lib, bw):
    """fails without the feature: both entries return 0 on the small case (and give the truth's values between intact sentinels)"""
    lc.check_c_entries(emu_lib, "cpu", "small", bw)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("bw", [1, 2])
def test_small_case_equals_the_per_frame_loop(emu_lib, bw, compact):
    lc.check_clip(emu_lib, "cpu", "small", lc.small_case(), bw, compact, True)


@pytest.mark.parametrize("compact", [False, True])
def test_one_frame(emu_lib, compact):
    """F = 1: the (160, 140) frame alone, both passes"""
    lc.check_clip(emu_lib, "cpu", "small", lc.small_case(), 1, compact, True, frames=[lc.BIG])


@pytest.mark.parametrize("bw", [1, 2])
def test_small_case_equals_the_oracles(emu_lib, bw):
    """oracle/raster_oracle.py + oracle/skimage_resize.py on the host, directly"""
    kp, crops, size = lc.small_case()
    want_l, want_b = lc.oracle_labels(kp, crops, size, bw)
    lbl, box, _ = raster.FaceRasteriser("cpu", lib=emu_lib).clip_labels(list(kp), size=size, crop=crops, relative=True, compact=True, bw=bw)
    diff = [(int((lbl[f] != want_l[f]).sum()), int((box[f] != want_b[f]).sum())) for f in range(len(crops))]
    print("[track_labels] differing from the oracles per frame (labels, masks):", diff)
    assert torch.equal(lbl, want_l) and torch.equal(box, want_b), diff


def test_real_size(emu_lib):
    lc.check_clip(emu_lib, "cpu", "real", lc.real_case(), None, True, False)


@pytest.mark.parametrize("cause", list(lc.REFUSALS))
@pytest.mark.parametrize("u8", [False, True])
def test_refusals_write_nothing(emu_lib, u8, cause):
    lc.check_refusal(emu_lib, "cpu", u8, cause)


def _wild(kind, d, c):
    """what the DEVICE copy says of one frame while the host copy is valid -> (the frame, whether the kernels must reject the row outright)"""
    if kind == "offset_beyond_the_workspace":
        d[2, 2] = c.ws_len + 1000
        return 2, True
    if kind == "offset_at_the_workspace_end":
        d[2, 2] = c.ws_len - 7
        return 2, True
    if kind == "negative_offset":
        d[2, 2] = -4096
        return 2, True
    if kind == "lw_63_at_the_pool_end":
        d[2, 3], d[2, 4], d[2, 5], d[2, 6] = 63, c.pool_len - 1, 63, c.pool_len
        return 2, True
    if kind == "absurd_lw":
        d[2, 3], d[2, 5] = 2 ** 31 - 1, -(2 ** 31)
        return 2, True
    if kind == "h_larger_than_the_hosts":                                # the first region: twice its rows still end inside the workspace
        d[0, 0] = 2 * d[0, 0]
        return 0, False
    if kind == "h_w_far_larger":
        d[2, 0], d[2, 1] = 30000, 30000
        return 2, True
    if kind == "h_w_beyond_the_kernels_range":
        d[2, 0], d[2, 1] = 2 ** 31 - 1, 2 ** 20
        return 2, True
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["offset_beyond_the_workspace", "offset_at_the_workspace_end", "negative_offset", "lw_63_at_the_pool_end", "absurd_lw",
                                  "h_larger_than_the_hosts", "h_w_far_larger", "h_w_beyond_the_kernels_range"])
@pytest.mark.parametrize("u8", [False, True])
def test_bad_device_descriptor_stays_inside_the_tensors(emu_lib, u8, kind):
    """The kernels range-check what they take from the device copy against the workspace length, the pool length and OH, OW: wrong pixels
    (a row they cannot use gives an all-zero frame), never a store outside the tensors.  Emulation build only."""
    kp, crops, size = lc.small_case()
    idx = list(lc.REFUSAL_FRAMES)
    c = lc.CCall(emu_lib, "cpu", kp[idx], crops[idx], size, 1, u8)
    assert c() == 0
    good_l, good_b = c.cls.clone(), c.box.clone()
    c.reset()
    wild = c.desc.copy()
    frame, rejected = _wild(kind, wild, c)
    c.desc_d = torch.from_numpy(wild)
    assert c() == 0
    assert c.sentinels_intact(), kind
    if rejected:
        keep = [f for f in range(len(idx)) if f != frame]
        assert torch.equal(c.cls[keep], good_l[keep]) and torch.equal(c.box[keep], good_b[keep]), kind
        assert int(c.cls[frame].sum()) == 0 and int(c.box[frame].sum()) == 0, kind
    assert set(np.unique(c.cls.numpy()).tolist()) <= {0, 1} and set(np.unique(c.box.numpy()).tolist()) <= {0, 1}


def test_pool_and_workspace_are_reused_and_grow(emu_lib):
    kp, crops, size = lc.small_case()
    rs = raster.FaceRasteriser("cpu", lib=emu_lib)
    few, more = [0, 6, 2], [0, 6, 2, 3, 1]
    a = rs.clip_labels(list(kp[few]), size=size, crop=crops[few], relative=True, compact=True, bw=1)
    pool, ws, n = rs._wpool, rs._ws, len(rs._wpool_host)
    b = rs.clip_labels(list(kp[few]), size=size, crop=crops[few], relative=True, compact=True, bw=1)      # every size is pooled, the workspace suffices
    assert rs._wpool is pool and rs._ws is ws and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = rs.clip_labels(list(kp[more]), size=size, crop=crops[more], relative=True, compact=True, bw=1)    # new sizes, a longer clip: both are replaced
    assert rs._wpool is not pool and rs._ws is not ws and len(rs._wpool_host) > n and rs._ws.numel() > ws.numel()
    held = rs._held["clip_labels"]
    assert held["old_pool"] is pool and held["old_workspace"] is ws                                       # kept for what may still read them
    pool, ws = rs._wpool, rs._ws
    d = rs.clip_labels(list(kp[few]), size=size, crop=crops[few], relative=True, compact=True, bw=1)      # a smaller clip again: nothing shrinks
    assert rs._wpool is pool and rs._ws is ws and torch.equal(d[0], a[0]) and torch.equal(d[1], a[1])
    want_l, want_b = lc.truth(emu_lib, "cpu", "small", kp, crops, size, 1, True, True)
    assert torch.equal(c[0], want_l[more]) and torch.equal(c[1], want_b[more]) and torch.equal(a[0], want_l[few])


def test_value_errors(emu_lib):
    kp, crops, size = lc.small_case()
    rs = raster.FaceRasteriser("cpu", lib=emu_lib)
    empty = crops.copy(); empty[2, 1] = empty[2, 0]
    for bad in (crops[:7], crops[:, :3], empty):
        with pytest.raises(ValueError):
            rs.clip_labels(list(kp), size=size, crop=bad, relative=True)
    with pytest.raises(RuntimeError, match="face_labels_boxes: bw"):         # the library's refusal comes up
        rs.clip_labels(list(kp), size=size, crop=crops, relative=True, bw=0)
