"""Tracking crops: a box per frame through frame loading, labels and paste-back (tsnet_prepare_frames_boxes[_u8], tsnet_paste_frames_boxes, the
(F,4) forms of FrameLoader / FaceRasteriser / face_driving_keypoints) -- CPU-emulation tier.  Everything is EQUALITY:
  * live Pillow equals the numpy restatement on every case (if not, the case list or the restatement is wrong, not the kernel);
  * every case through the C entries between sentinels, through FrameLoader, and against the single-box entry frame by frame;
  * one refusal test per cause, the bad frame in the middle, nothing written for any frame;
  * a DEVICE descriptor that points past the pool while the host copy is valid writes nothing outside the tensors (emulation only);
  * the Python layer: the six FrameLoader methods, the table pool, labels of 8 real frames with their own crops, the cross-identity key points.
The GPU tier (test_gpu_track_crop.py) runs the same cases through the HIP library."""
import numpy as np
import pytest
import torch

import paste_cases as pc
import track_crop_cases as tc
from wacv23_tsnet_amd import frames, raster

PREPARE_IDS = [v[0] for v in tc.PREPARE_VARIANTS] + ["prepare_face_real"]
PASTE_IDS = [v[0] for v in tc.PASTE_VARIANTS]


@pytest.mark.parametrize("vid", PREPARE_IDS)
def test_prepare_pillow_equals_the_restatement(vid):
    e = tc.prepare_expected(vid)
    got = tc.expect_prepare_pillow(np.array(e["fr"]), e["boxes"], e["size"], e["square"])
    assert np.array_equal(got, e["want"]), (vid, int((got != e["want"]).sum()), pc.PIL_NOTE)


@pytest.mark.parametrize("vid", PASTE_IDS)
def test_paste_pillow_equals_the_restatement(vid):
    e = tc.paste_expected(vid)
    got = tc.expect_paste_pillow(np.array(e["fr"]), np.array(e["gen"]), e["boxes"], e["src_box"], None if e["mask"] is None else np.array(e["mask"]))
    assert np.array_equal(got, e["want"]), (vid, int((got != e["want"]).sum()), pc.PIL_NOTE)
    assert np.array_equal(e["want"], e["fr"]) == (vid == "paste_all_outside")


@pytest.mark.parametrize("vid", PREPARE_IDS)
def test_prepare_cases_emulated(emu_lib, vid):
    tc.check_prepare(emu_lib, "cpu", frames.FrameLoader("cpu", lib=emu_lib), vid)


@pytest.mark.parametrize("vid", PASTE_IDS)
def test_paste_cases_emulated(emu_lib, vid):
    tc.check_paste(emu_lib, "cpu", frames.FrameLoader("cpu", lib=emu_lib), vid)


@pytest.mark.parametrize("cause", list(tc.REFUSALS))
@pytest.mark.parametrize("which", ["prepare", "prepare_u8", "paste"])
def test_refusals_write_nothing(emu_lib, which, cause):
    tc.check_refusal(emu_lib, "cpu", frames.FrameLoader("cpu", lib=emu_lib), which, cause)


BAD_DEVICE_ROWS = {                      # what the DEVICE copy of frame 2 says while the host copy is valid
    "offsets_past_the_pool": {4: 10 ** 9, 6: 2 ** 31 - 1},
    "table_ends_past_the_pool": {4: lambda n: n - 3, 6: lambda n: n - 1},
    "negative_offsets": {4: -7, 6: -(2 ** 31)},
    "absurd_taps": {5: 2 ** 31 - 1, 7: -3},
    "absurd_box": {0: -(2 ** 31), 1: 2 ** 31 - 1, 2: 2 ** 31 - 1, 3: -(2 ** 31)},
    "huge_box_and_taps": {2: 2 ** 24 + 100, 3: 2 ** 30, 5: 2 ** 20, 7: 2 ** 20},
}


@pytest.mark.parametrize("kind", list(BAD_DEVICE_ROWS))
def test_bad_device_descriptor_stays_inside_the_tensors(emu_lib, kind):
    """The device copy is trusted as the tables are, but the kernel range-checks what it takes from it: wrong pixels (unspecified), never a store
    outside the tensors.  Emulation build only: a wild access is not something to try on a device."""
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    rng = np.random.default_rng(12)
    fr = rng.integers(0, 256, (5, 48, 56, 3), dtype=np.uint8)
    # prepare
    boxes, size = tc.REFUSAL_BOXES_PREPARE, (24, 20)
    desc, desc_d, pool = tc.prepare_descriptors(ld, boxes, size)
    wild = desc.copy()
    for col, v in BAD_DEVICE_ROWS[kind].items():
        wild[tc.BAD, col] = np.int64(v(pool.numel()) if callable(v) else v).astype(np.int32)
    wild_d = torch.from_numpy(wild)
    good = ld.prepare(fr, boxes, size, as_bytes=True)
    buf, out = tc.guarded_out((5, 3, 20, 24), torch.uint8, "cpu")
    assert tc.prepare_c(emu_lib, torch.from_numpy(fr), desc, wild_d, pool, size, False, out) == 0
    assert pc.sentinels_intact(buf)
    keep = [f for f in range(5) if f != tc.BAD]
    assert torch.equal(out[keep], good[keep])                        # the other frames are right; frame 2 is unspecified
    # paste
    gen = torch.from_numpy(rng.integers(0, 256, (5, 24, 20, 3), dtype=np.uint8))
    boxes = tc.REFUSAL_BOXES_PASTE
    desc, desc_d, pool = tc.paste_descriptors(ld, boxes, (20, 24))
    wild = desc.copy()
    for col, v in BAD_DEVICE_ROWS[kind].items():
        wild[tc.BAD, col] = np.int64(v(pool.numel()) if callable(v) else v).astype(np.int32)
    good = ld.paste(gen, fr, boxes)
    buf, view = pc.guarded(fr, "cpu")
    assert tc.paste_c(emu_lib, gen, None, view, desc, torch.from_numpy(wild), pool, None) == 0
    assert pc.sentinels_intact(buf)
    assert torch.equal(view[keep], good[keep])


# ------------------------------------------------------------------------------------------------------------------------- the Python layer
def _clip(F=5):
    rng = np.random.default_rng(21)
    fr = rng.integers(0, 256, (F, 60, 90, 3), dtype=np.uint8)
    boxes = np.array([(5, 6, 45, 50), (7, 4, 47, 48), (-3, 8, 39, 50), (30, 20, 95, 70), (7, 4, 47, 48)][:F])     # two frames share sizes; one pair repeats
    return fr, boxes


def _yx(boxes):
    return np.asarray(boxes)[:, [1, 3, 0, 2]]                        # (x0, y0, x1, y1) -> [min_y, max_y, min_x, max_x]


def test_loader_forms_equal_the_per_frame_loop(emu_lib):
    ld, one = frames.FrameLoader("cpu", lib=emu_lib), frames.FrameLoader("cpu", lib=emu_lib)
    fr, boxes = _clip()
    F = len(boxes)
    loop = lambda fn: torch.cat([fn(f) for f in range(F)])
    for as_bytes in (False, True):
        want = loop(lambda f: one.prepare(fr[f:f + 1], boxes[f], (32, 28), as_bytes=as_bytes))
        assert torch.equal(ld.prepare(fr, boxes, (32, 28), as_bytes=as_bytes), want)
        assert torch.equal(ld.prepare(torch.from_numpy(fr), boxes.tolist(), (32, 28), as_bytes=as_bytes), want)       # tensors, lists
        assert torch.equal(ld.face(fr, _yx(boxes), (32, 28), as_bytes=as_bytes), want)
        assert torch.equal(ld.face(fr, _yx(boxes), (32, 28), as_bytes=as_bytes), loop(lambda f: one.face(fr[f:f + 1], _yx(boxes)[f], (32, 28), as_bytes=as_bytes)))
        assert torch.equal(ld.pose(fr, boxes, (16, 32), as_bytes=as_bytes), loop(lambda f: one.pose(fr[f:f + 1], boxes[f], (16, 32), as_bytes=as_bytes)))
    gen = np.random.default_rng(22).integers(0, 256, (F, 32, 32, 3), dtype=np.uint8)
    mask = pc.make_mask("loader", "bands", F, 32, 32)
    for m in (None, mask):
        mf = lambda f: None if m is None else m[f:f + 1]
        want = loop(lambda f: one.paste(gen[f:f + 1], fr[f:f + 1], boxes[f], mask=mf(f)))
        assert torch.equal(ld.paste(gen, fr, boxes, mask=m), want) and not torch.equal(want, torch.from_numpy(fr))
        assert torch.equal(ld.paste(torch.from_numpy(gen), torch.from_numpy(fr), torch.from_numpy(boxes), mask=None if m is None else torch.from_numpy(m)), want)
        assert torch.equal(ld.paste_face(gen, fr, _yx(boxes), mask=m), want)
        assert torch.equal(ld.paste_face(gen, fr, _yx(boxes), mask=m), loop(lambda f: one.paste_face(gen[f:f + 1], fr[f:f + 1], _yx(boxes)[f], mask=mf(f))))
        assert torch.equal(ld.paste_pose(gen, fr, boxes, img_size=(16, 32), mask=m),
                           loop(lambda f: one.paste_pose(gen[f:f + 1], fr[f:f + 1], boxes[f], img_size=(16, 32), mask=mf(f))))
        assert torch.equal(ld.paste(gen, fr, boxes, src_box=(3, 2, 30, 29), mask=m), loop(lambda f: one.paste(gen[f:f + 1], fr[f:f + 1], boxes[f], src_box=(3, 2, 30, 29), mask=mf(f))))


def test_inplace_against_the_clone(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr, boxes = _clip()
    gen = torch.from_numpy(np.random.default_rng(23).integers(0, 256, (len(boxes), 24, 20, 3), dtype=np.uint8))
    t = torch.from_numpy(fr.copy())
    out = ld.paste(gen, t, boxes)
    assert out.data_ptr() != t.data_ptr() and torch.equal(t, torch.from_numpy(fr)) and not torch.equal(out, t)
    out2 = ld.paste(gen, t, boxes, inplace=True)
    assert out2.data_ptr() == t.data_ptr() and torch.equal(t, out)
    assert np.array_equal(out.numpy(), tc.expect_paste_numpy(fr, gen.numpy(), [tuple(b) for b in boxes.tolist()]))


def test_pool_is_reused_and_grows(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr, boxes = _clip()
    a = ld.prepare(fr, boxes, (32, 28), as_bytes=True)
    n, pool = len(ld._pool_host), ld._pool
    b = ld.prepare(fr, boxes, (32, 28), as_bytes=True)               # every size is pooled: the same pool, the same bytes
    assert len(ld._pool_host) == n and ld._pool is pool and torch.equal(a, b)
    more = boxes.copy(); more[1] = (2, 3, 51, 57); more[3] = (1, 1, 80, 59)
    c = ld.prepare(fr, more, (32, 28), as_bytes=True)                # new sizes: the pool grows, the old one is kept for what may still read it
    assert len(ld._pool_host) > n and ld._pool is not pool and ld._held["prepare"]["old_pool"] is pool
    assert torch.equal(c, frames.FrameLoader("cpu", lib=emu_lib).prepare(fr, more, (32, 28), as_bytes=True))
    assert torch.equal(ld.prepare(fr, boxes, (32, 28), as_bytes=True), a)
    assert np.array_equal(c.numpy(), tc.expect_prepare_numpy(fr, [tuple(r) for r in more.tolist()], (32, 28), False))


def test_value_errors(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr, boxes = _clip()
    gen = np.zeros((len(boxes), 24, 20, 3), np.uint8)
    empty = boxes.copy(); empty[2, 2] = empty[2, 0]
    for bad in (boxes[:4], boxes[:, :3], np.concatenate([boxes, boxes]), empty):
        with pytest.raises(ValueError):
            ld.prepare(fr, bad, (32, 28))
        with pytest.raises(ValueError):
            ld.paste(gen, fr, bad)
    with pytest.raises(ValueError):
        ld.face(fr, _yx(boxes)[:3])
    with pytest.raises(ValueError):
        ld.paste(gen, fr, boxes, src_box=(0, 0, 21, 24))
    with pytest.raises(RuntimeError, match="frame 1: .*steep"):      # the library's refusal comes up with its frame
        steep = boxes.copy(); steep[1] = (0, 0, 40, 900)
        ld.prepare(fr, steep, (32, 28))


# ------------------------------------------------------------------------------------------------------------------------- labels
LABEL_FRAMES = (0, 2, 13, 8, 3, 17, 9, 1)                            # of test114: crops of 244, 246, 244, 248, 246, 250, 248, 244 pixels -- interleaved


@pytest.fixture(scope="module")
def face_clip():
    import sys
    sys.path.insert(0, tc.os.path.join(tc.ROOT, "tools"))
    import demo_clip
    kp = demo_clip.clip_keypoints("test114")[0][list(LABEL_FRAMES)]
    crops = raster.crop_coords_clip(kp)
    assert [int(c[1] - c[0]) for c in crops] == [244, 246, 244, 248, 246, 250, 248, 244]
    return kp, crops


def test_crop_coords_clip(face_clip):
    kp, crops = face_clip
    assert crops.shape == (8, 4) and [tuple(c) for c in crops.tolist()] == [tuple(raster.crop_coords(k)) for k in kp]


def test_rasterise_with_a_crop_per_frame(emu_lib, face_clip):
    from oracle import raster_oracle as RO
    kp, crops = face_clip
    rs = raster.FaceRasteriser("cpu", lib=emu_lib)
    edges, bbox, got_crops, bw = rs.rasterise(list(kp), crops)
    assert bw == 1 and np.array_equal(got_crops, crops) and len(edges) == len(bbox) == 8
    for f in range(8):
        h, w = int(crops[f, 1] - crops[f, 0]), int(crops[f, 3] - crops[f, 2])
        assert tuple(edges[f].shape) == tuple(bbox[f].shape) == (h, w)
        e1, b1, _, _ = rs.rasterise([kp[f]], tuple(int(v) for v in crops[f]), bw=bw)
        assert torch.equal(edges[f], e1[0]) and torch.equal(bbox[f], b1[0]), f
        rel = RO.crop_keypoints(kp[f], crops[f])
        assert np.array_equal(edges[f].numpy(), RO.face_edge_map(rel, (w, h), bw)), f
        assert np.array_equal(bbox[f].numpy(), RO.bbox_mask(rel, (w, h))), f
    rel = kp - crops[:, None, [2, 0]]                                # relative=True takes the points as they are
    e2, b2, _, _ = rs.rasterise(list(rel), crops, relative=True)
    assert all(torch.equal(a, b) for a, b in zip(e2, edges)) and all(torch.equal(a, b) for a, b in zip(b2, bbox))
    with pytest.raises(ValueError):
        rs.rasterise(list(kp), crops[:7])


def test_clip_labels_with_a_crop_per_frame(emu_lib, face_clip):
    kp, crops = face_clip
    rs = raster.FaceRasteriser("cpu", lib=emu_lib)
    for compact in (False, True):
        lbl, box, got_crops = rs.clip_labels(list(kp), crop=crops, compact=compact)
        assert tuple(lbl.shape) == ((8, 256, 256) if compact else (8, 2, 256, 256)) and tuple(box.shape) == (8, 256, 256)
        assert lbl.dtype == box.dtype == (torch.uint8 if compact else torch.float32) and np.array_equal(got_crops, crops)
        for f in range(8):
            l1, b1, _ = rs.clip_labels([kp[f]], crop=tuple(int(v) for v in crops[f]), compact=compact)
            assert torch.equal(lbl[f], l1[0]) and torch.equal(box[f], b1[0]), (compact, f)


def test_brush_is_the_first_frames(emu_lib, face_clip):
    """The reference computes the brush once per clip, from the first frame's crop (:302, :347): a first frame whose crop is >= 512 pixels high
    gives bw = 2 for every frame, the smaller ones included."""
    kp, crops = face_clip
    kp = kp[:4].copy()
    kp[0] = (kp[0] - kp[0].mean(0)) * 2.2 + kp[0].mean(0)             # the first frame's face, larger
    kp[0] = np.round(kp[0])
    crops = raster.crop_coords_clip(kp)
    assert crops[0, 1] - crops[0, 0] >= 512 and all(c[1] - c[0] < 512 for c in crops[1:])
    rs = raster.FaceRasteriser("cpu", lib=emu_lib)
    edges, bbox, _, bw = rs.rasterise(list(kp), crops)
    assert bw == 2
    for f in range(4):
        e2, b2, _, _ = rs.rasterise([kp[f]], tuple(int(v) for v in crops[f]), bw=2)
        assert torch.equal(edges[f], e2[0]) and torch.equal(bbox[f], b2[0]), f
    thin, _, _, bw1 = rs.rasterise([kp[1]], tuple(int(v) for v in crops[1]))
    assert bw1 == 1 and not torch.equal(thin[0], edges[1])           # the frame's own size would have drawn a thinner line


def test_face_driving_keypoints_with_tracking_crops(emu_lib):
    import sys
    sys.path.insert(0, tc.os.path.join(tc.ROOT, "tools"))
    import demo_clip
    sub, drv = demo_clip.clip_keypoints("test114")[0], demo_clip.clip_keypoints("val024")[0]
    pts, crops, bw = raster.face_driving_keypoints(sub, drv, lib=emu_lib, fix_crop_pos=False)
    assert np.array_equal(crops, raster.crop_coords_clip(drv)) and crops.shape == (len(drv), 4) and bw == max(1, int(crops[0, 1] - crops[0, 0]) // 256)
    rel = lambda kp: kp - raster.crop_coords_clip(kp)[:, None, [2, 0]]
    want = raster.smooth_keypoints(raster.FaceAdapter(emu_lib).fit(rel(sub)).apply(rel(drv)), emu_lib)
    assert pts.dtype == np.float64 and np.array_equal(pts, want)
    fixed = raster.face_driving_keypoints(sub, drv, lib=emu_lib)
    assert not np.array_equal(pts, fixed[0])                         # the crops do move on these clips
    # every frame given the first frame's landmarks: every crop is the first frame's, and the two modes agree
    sub0, drv0 = np.repeat(sub[:1], 7, 0), np.repeat(drv[:1], 6, 0)
    a = raster.face_driving_keypoints(sub0, drv0, lib=emu_lib, fix_crop_pos=False)
    b = raster.face_driving_keypoints(sub0, drv0, lib=emu_lib)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] and all(tuple(c) == tuple(b[1]) for c in a[1].tolist())
