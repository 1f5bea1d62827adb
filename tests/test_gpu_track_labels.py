"""GPU tier of the face labels with a crop per frame (tsnet_face_labels_boxes[_u8], FaceRasteriser.clip_labels with (F,4) crops): the cases of
track_labels_cases.py through the HIP library -- the C entries between sentinels, the small case in both forms and both brushes, one frame, the
real-size case, the refusals -- equal to the single-crop path frame by frame; then the stream-order properties: back-to-back calls on a busy side
stream with a workspace that grows, and labels consumed by the clip harness on the same stream with no synchronisation in between."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import track_labels_cases as lc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_library_exports_the_entries():
    """fails without the feature: the symbols exist in the built library"""
    from wacv23_tsnet_amd import _lib
    lib = _lib.load()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (tsnet_[a-z0-9_]+)", out))
    for s in ("tsnet_face_labels_boxes", "tsnet_face_labels_boxes_u8"):
        assert s in exported and s in _lib.ABI_SYMBOLS and hasattr(lib, s)


def test_c_entries_gpu():
    """fails without the feature: both entries return 0 on the small case (and give the truth's values between intact sentinels)"""
    from wacv23_tsnet_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    rep = [lc.check_c_entries(lib, dev, "small", bw) for bw in (1, 2)]
    print("[track_labels] " + json.dumps(rep))


def test_small_case_gpu():
    from wacv23_tsnet_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    kp, crops, size = lc.small_case()
    for bw in (1, 2):
        for compact in (False, True):
            lbl, box = lc.check_clip(lib, dev, "small", lc.small_case(), bw, compact, True)
        want_l, want_b = lc.oracle_labels(kp, crops, size, bw)       # oracle/raster_oracle.py + oracle/skimage_resize.py on the host, directly
        assert torch.equal(lbl.cpu(), want_l) and torch.equal(box.cpu(), want_b), bw
    for compact in (False, True):
        lc.check_clip(lib, dev, "small", lc.small_case(), 1, compact, True, frames=[lc.BIG])          # F = 1


def test_real_size_gpu():
    from wacv23_tsnet_amd import _lib
    lc.check_clip(_lib.load(), torch.device("cuda", 0), "real", lc.real_case(), None, True, False)


def test_refusals_gpu():
    """every cause through the HIP library: refused on the host copy before anything is enqueued"""
    from wacv23_tsnet_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    rep = [lc.check_refusal(lib, dev, u8, cause) for u8 in (False, True) for cause in lc.REFUSALS]
    print("[track_labels] " + json.dumps(rep))


def test_back_to_back_calls_are_stream_ordered():
    """Three clips one after the other on a busy side stream with no synchronisation in between -- the second needs a larger workspace and new
    half-kernels, the third a smaller workspace again -- give what a synchronisation after every call gives, which is the per-frame truth."""
    from wacv23_tsnet_amd import _lib, raster
    lib, dev = _lib.load(), torch.device("cuda", 0)
    skp, scrops, ssize = lc.small_case()
    rkp, rcrops, rsize = lc.real_case()
    few, rest = [0, 6, 2], [3, 1, 5, 7]
    calls = [dict(keypoints=list(skp[few]), size=ssize, crop=scrops[few], relative=True, compact=True, bw=1),
             dict(keypoints=list(rkp), size=rsize, crop=rcrops, compact=True),
             dict(keypoints=list(skp[rest]), size=ssize, crop=scrops[rest], relative=True, compact=True, bw=1)]
    ref = raster.FaceRasteriser(dev)
    want = []
    for kw in calls:
        l, b, _ = ref.clip_labels(**kw)
        torch.cuda.synchronize()
        want.append((l.clone(), b.clone()))
    rs = raster.FaceRasteriser(dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    seen = []
    with torch.cuda.stream(stream):
        junk = torch.empty((64, 1024, 1024), device=dev).normal_()          # work in front of the kernels: the stream is busy when they are enqueued
        got = []
        for kw in calls:
            l, b, _ = rs.clip_labels(**kw)
            got.append((l, b))
            seen.append((rs._wpool, rs._ws))
    stream.synchronize()
    assert seen[1][1] is not seen[0][1] and seen[1][0] is not seen[0][0]        # the second clip replaced both ...
    assert seen[2][1] is seen[1][1] and seen[2][0] is not None                  # ... and the third, smaller one reuses the workspace
    for (l, b), (wl, wb) in zip(got, want):
        assert torch.equal(l, wl) and torch.equal(b, wb)
    tl, tb = lc.truth(lib, dev, "small", skp, scrops, ssize, 1, True, True)
    assert torch.equal(got[0][0].cpu(), tl[few]) and torch.equal(got[2][0].cpu(), tl[rest]) and torch.equal(got[2][1].cpu(), tb[rest])
    tl, tb = lc.truth(lib, dev, "real", rkp, rcrops, rsize, 1, True, False)
    assert torch.equal(got[1][0].cpu(), tl) and torch.equal(got[1][1].cpu(), tb)
    del junk


def test_labels_feed_the_clip_harness_on_the_same_stream():
    """clip_labels with a crop per frame followed directly by ClipRunner on the same stream (the tiny face model, 3 sources, 5 driving frames of
    several sizes, batch 4): the frames are the bytes obtained with a synchronisation between the two."""
    import demo_clip
    from wacv23_tsnet_amd import demo, raster
    from wacv23_tsnet_amd.model import TSNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = TSNet(is_train=False, label_nc=2, n_blocks=1, n_downsampling=3, n_source=3).cuda()
    K, F = 3, 5
    kp = demo_clip.synthetic_face_keypoints(K + F)
    for f in range(K + F):                                               # the face grows a little from frame to frame: the crops take several sizes
        kp[f] = np.round((kp[f] - kp[f].mean(0)) * (1.0 + 0.03 * f) + kp[f].mean(0))
    crops = raster.crop_coords_clip(kp)
    assert len({(int(c[1] - c[0]), int(c[3] - c[2])) for c in crops}) >= 4
    g = torch.Generator().manual_seed(1)
    src_img = [(torch.rand((1, 3, 256, 256), generator=g) * 255.0 - torch.from_numpy(demo.IMG_MEAN).view(1, 3, 1, 1)) for _ in range(K)]
    rs = raster.FaceRasteriser(dev)
    lbl, box, _ = rs.clip_labels(list(kp), crop=crops)
    torch.cuda.synchronize()
    with demo.ClipRunner(model, src_img, [lbl[i:i + 1] for i in range(K)], [box[i:i + 1] for i in range(K)], batch=4) as runner:
        want = runner.run(lbl[K:], box[K:])
        lbl2, box2, _ = rs.clip_labels(list(kp[K:]), crop=crops[K:], bw=1)       # enqueued, and consumed at once
        got = runner.run(lbl2, box2)
    assert got.shape == (F, 256, 256, 3) and np.array_equal(got, want)
    assert torch.equal(lbl2, lbl[K:]) and torch.equal(box2, box[K:])
