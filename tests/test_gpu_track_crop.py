"""GPU tier of the tracking crops (tsnet_prepare_frames_boxes[_u8], tsnet_paste_frames_boxes, the (F,4) forms of FrameLoader,
ClipRunner.run(paste_boxes=...)): the cases of track_crop_cases.py through the HIP library -- the C entries between sentinels, FrameLoader, and the
single-box entry frame by frame -- equal to the numpy restatement byte for byte; the refusals; the stream-order property; the clip harness."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import paste_cases as pc
import track_crop_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_cases_gpu():
    from wacv23_tsnet_amd import _lib, frames
    lib, dev = _lib.load(), torch.device("cuda", 0)
    ld = frames.FrameLoader(dev)
    rep = [tc.check_prepare(lib, dev, ld, v[0]) for v in tc.PREPARE_VARIANTS] + [tc.check_prepare(lib, dev, ld, "prepare_face_real")]
    rep += [tc.check_paste(lib, dev, ld, v[0]) for v in tc.PASTE_VARIANTS]
    print("[track_crop] " + json.dumps(rep))


def test_refusals_gpu():
    """every cause through the HIP library: refused on the host copy before anything is launched"""
    from wacv23_tsnet_amd import _lib, frames
    lib, dev = _lib.load(), torch.device("cuda", 0)
    rep = [tc.check_refusal(lib, dev, frames.FrameLoader(dev), which, cause) for which in ("prepare", "prepare_u8", "paste") for cause in tc.REFUSALS]
    print("[track_crop] " + json.dumps(rep))


def test_loader_on_device_tensors():
    """(F,4) forms on device tensors: equal to the per-frame loop, inplace against the clone, a second call on pooled sizes, a call that grows the pool"""
    from wacv23_tsnet_amd import frames
    dev = torch.device("cuda", 0)
    ld, one = frames.FrameLoader(dev), frames.FrameLoader(dev)
    e = tc.paste_expected("paste_mixed-mask_bands")
    fr, gen, mask = (torch.from_numpy(np.array(e[k])).to(dev) for k in ("fr", "gen", "mask"))
    boxes, F = e["boxes"], len(e["boxes"])
    want = torch.from_numpy(np.array(e["want"])).to(dev)
    t = fr.clone()
    out = ld.paste(gen, t, boxes, mask=mask)
    assert out.data_ptr() != t.data_ptr() and torch.equal(t, fr) and torch.equal(out, want)
    out2 = ld.paste(gen, t, boxes, mask=mask, inplace=True)
    assert out2.data_ptr() == t.data_ptr() and torch.equal(t, want)
    crops = np.asarray(boxes)[:, [1, 3, 0, 2]]
    assert torch.equal(ld.paste_face(gen, fr, crops, mask=mask), want)
    pool = ld._pool
    assert torch.equal(ld.paste(gen, fr, boxes, mask=mask), want) and ld._pool is pool               # pooled sizes: descriptors + one launch
    p = tc.prepare_expected("prepare_mixed")
    pfr = torch.from_numpy(np.array(p["fr"])).to(dev)
    got = ld.prepare(pfr, p["boxes"], p["size"], as_bytes=True)                                      # new sizes: the pool grows
    assert ld._pool is not pool and torch.equal(got.cpu(), torch.from_numpy(np.array(p["want"])))
    assert torch.equal(ld.face(pfr, np.asarray(p["boxes"])[:, [1, 3, 0, 2]], p["size"]).cpu(), torch.from_numpy(tc.widen(p["want"])))
    assert torch.equal(ld.pose(pfr, p["boxes"], (40, 72), as_bytes=True),
                       torch.cat([one.pose(pfr[f:f + 1], p["boxes"][f], (40, 72), as_bytes=True) for f in range(len(p["boxes"]))]))
    assert torch.equal(ld.paste_pose(gen[:, :64], fr, boxes, img_size=(32, 64), mask=mask[:, :64]),
                       torch.cat([one.paste_pose(gen[f:f + 1, :64], fr[f:f + 1], boxes[f], img_size=(32, 64), mask=mask[f:f + 1, :64]) for f in range(F)]))
    assert torch.equal(ld.paste(gen, fr, boxes, mask=mask), want)                                    # after the growth, the same bytes


def test_prepare_and_paste_are_stream_ordered():
    """prepare -> (identity) -> paste with a box per frame, enqueued back to back on a busy side stream with no synchronisation in between, gives
    the frames obtained with a synchronisation after every call."""
    from wacv23_tsnet_amd import frames
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    video = torch.from_numpy(rng.integers(0, 256, (3, 480, 640, 3), dtype=np.uint8)).to(dev)
    back = torch.from_numpy(rng.integers(0, 256, (3, 480, 640, 3), dtype=np.uint8)).to(dev)
    mask = torch.from_numpy(pc.make_mask("stream", "bands", 3, 256, 256)).to(dev)
    boxes = [(-21, 17, 253, 291), (200, 100, 470, 370), (380, 230, 652, 502)]
    ld = frames.FrameLoader(dev)

    def chain():
        planes = ld.prepare(video, boxes, (256, 256), as_bytes=True)                                  # (F,3,256,256) B, G, R
        gen = planes.flip(1).permute(0, 2, 3, 1).contiguous()                                         # the generator's place: RGB bytes again
        return ld.paste(gen, back, boxes, mask=mask), gen

    # with a synchronisation after every call (this also fills the pool, so the second round is enqueue-only)
    planes = ld.prepare(video, boxes, (256, 256), as_bytes=True); torch.cuda.synchronize()
    gen = planes.flip(1).permute(0, 2, 3, 1).contiguous(); torch.cuda.synchronize()
    want = ld.paste(gen, back, boxes, mask=mask); torch.cuda.synchronize()
    assert np.array_equal(want.cpu().numpy(), tc.expect_paste_numpy(back.cpu().numpy(), gen.cpu().numpy(), boxes, None, mask.cpu().numpy()))
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        junk = torch.empty((64, 1024, 1024), device=dev).normal_()          # work in front of the kernels: the stream is busy when they are enqueued
        got, _ = chain()
    stream.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, back)
    del junk


def test_clip_runner_pastes_with_a_box_per_frame():
    """ClipRunner.run(paste_boxes=...) on the tiny face model: 6 driving frames at batch 4 (a ragged last group), boxes that move by a few pixels
    and take two sizes.  The full frames equal the numpy restatement applied per frame to the runner's own 256 x 256 bytes."""
    import demo_clip
    from wacv23_tsnet_amd import demo, raster
    from wacv23_tsnet_amd.model import TSNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = TSNet(is_train=False, label_nc=2, n_blocks=1, n_downsampling=3, n_source=3).cuda()
    K, F = 3, 6
    kp = demo_clip.synthetic_face_keypoints(K + F)
    rs = raster.FaceRasteriser(dev)
    edges, bbox, crop, bw = rs.rasterise(list(kp))
    lbl, box = rs.vl2ch(demo.resize_label(edges), 2), demo.resize_label(bbox)
    g = torch.Generator().manual_seed(1)
    src_img = [(torch.rand((1, 3, 256, 256), generator=g) * 255.0 - torch.from_numpy(demo.IMG_MEAN).view(1, 3, 1, 1)) for _ in range(K)]
    video = np.random.default_rng(8).integers(0, 256, (F, 200, 300, 3), dtype=np.uint8)
    pboxes = [(170, -40, 370, 160), (172, -38, 372, 162), (169, -41, 373, 163), (165, -36, 369, 168), (171, -42, 371, 158), (168, -39, 372, 165)]
    assert len({(b[2] - b[0], b[3] - b[1]) for b in pboxes}) == 2
    with demo.ClipRunner(model, src_img, [lbl[i:i + 1] for i in range(K)], [box[i:i + 1] for i in range(K)], batch=4) as runner:
        small = runner.run(lbl[K:], box[K:])
        keep = video.copy()
        full = runner.run(lbl[K:], box[K:], paste_into=video, paste_boxes=pboxes)
        full_d = runner.run(lbl[K:], box[K:], paste_into=torch.from_numpy(video).to(dev), paste_boxes=np.asarray(pboxes))
        with pytest.raises(ValueError):
            runner.run(lbl[K:], box[K:], paste_into=video, paste_box=pboxes[0], paste_boxes=pboxes)
        with pytest.raises(ValueError):
            runner.run(lbl[K:], box[K:], paste_into=video, paste_boxes=pboxes[:5])
    assert small.shape == (F, 256, 256, 3) and full.shape == video.shape and full.dtype == np.uint8
    assert np.array_equal(video, keep)                                      # paste_into is left as it is
    want = tc.expect_paste_numpy(video, small, pboxes)
    assert np.array_equal(full, want) and np.array_equal(full_d, want) and not np.array_equal(want, video)
