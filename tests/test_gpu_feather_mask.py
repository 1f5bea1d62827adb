"""GPU tier of the feathered paste masks (tsnet_blur_mask, FrameLoader.feather_mask, ClipRunner.run(paste_feather=...)): the cases of
feather_cases.py through the HIP library, equal to the numpy restatement byte for byte with the sentinels around output and intermediate
intact; the stream-order property; and the clip harness feathering its own paste.  There is one route (rows kernel, then columns kernel), so
the selector's values 0 and 1 are held equal and nothing else."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import feather_cases as fc
import paste_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_cases_gpu():
    from wacv23_tsnet_amd import _lib, frames
    lib, dev = _lib.load(), torch.device("cuda", 0)
    ld = frames.FrameLoader(dev)
    rep = [fc.check_case(lib, dev, ld, cid, routes=(0, 1)) for cid in fc.IDS]
    print("[feather] " + json.dumps(rep))
    out_dir = os.environ.get("TSNET_REPORT_DIR")                     # where the caller collects reports, if anywhere
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "feather_report.json"), "w") as f:
            json.dump(rep, f)


def test_refusals_write_nothing_gpu():
    from wacv23_tsnet_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    shape = (2, 20, 30)
    src = torch.from_numpy(fc.make_input("errors", shape, "random")).to(dev)
    obuf, out = fc.guarded(shape, dev)
    tbuf, tmp = fc.guarded(shape, dev)
    for over in (dict(H=fc.MAX_SIDE + 1), dict(rx=-1.0), dict(tmp=None), dict(src=None, rect=None), dict(flags=3 << 8)):
        assert fc.blur_c(lib, src, shape, None, 2.0, 0, out, tmp, **over) == -1, over
        assert lib.tsnet_op_last_error().decode().startswith("blur_mask")
    torch.cuda.synchronize()
    assert fc.untouched(obuf) and fc.untouched(tbuf)


def test_blur_is_stream_ordered():
    """a blur enqueued on a busy side stream behind the kernel that writes its input, no synchronisation in between, sees that input"""
    from wacv23_tsnet_amd import frames
    dev = torch.device("cuda", 0)
    ld = frames.FrameLoader(dev)
    m = fc.make_input("stream", (4, 256, 256), "random")
    want = torch.from_numpy(fc.expect_numpy(m, 8))
    src = torch.from_numpy(m).to(dev)
    assert torch.equal(ld.feather_mask(src, 8).cpu(), want)                  # with a synchronisation; the workspace is allocated here
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        junk = torch.empty((64, 1024, 1024), device=dev).normal_()          # work in front: the stream is busy when the kernels are enqueued
        late = torch.zeros_like(src)
        late.copy_(src)                                                     # the kernel that writes the blur's input
        got = ld.feather_mask(late, 8)
        late2 = (late != 0).to(torch.uint8)                                 # ... and a 0 / 1 form made on the stream, taken as binary
        got2 = ld.feather_mask(late2, 8, binary=True)
    stream.synchronize()
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got2.cpu(), torch.from_numpy(fc.expect_numpy(m, 8, binary=True)))
    del junk


def test_clip_runner_feathers_its_paste():
    """ClipRunner.run(paste_into=..., paste_feather=...) on the tiny face model: 6 driving frames at batch 4 (a ragged last group), a box
    leaving the frame; "box" and "bbox".  The full frames equal the CPU-tier sequence -- the numpy restatements of the blur and of the paste --
    applied to the runner's own 256 x 256 bytes from a run without paste_into."""
    import demo_clip
    from wacv23_tsnet_amd import demo, frames, raster
    from wacv23_tsnet_amd.model import TSNet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = TSNet(is_train=False, label_nc=2, n_blocks=1, n_downsampling=3, n_source=3).cuda()
    K, F, r = 3, 6, 8
    kp = demo_clip.synthetic_face_keypoints(K + F)
    rs = raster.FaceRasteriser(dev)
    edges, bbox, crop, bw = rs.rasterise(list(kp))
    lbl, box = rs.vl2ch(demo.resize_label(edges), 2), demo.resize_label(bbox)
    g = torch.Generator().manual_seed(1)
    src_img = [(torch.rand((1, 3, 256, 256), generator=g) * 255.0 - torch.from_numpy(demo.IMG_MEAN).view(1, 3, 1, 1)) for _ in range(K)]
    video = np.random.default_rng(8).integers(0, 256, (F, 200, 300, 3), dtype=np.uint8)
    pbox = (170, -40, 370, 160)
    with demo.ClipRunner(model, src_img, [lbl[i:i + 1] for i in range(K)], [box[i:i + 1] for i in range(K)], batch=4) as runner:
        small = runner.run(lbl[K:], box[K:])
        full_box = runner.run(lbl[K:], box[K:], paste_into=video, paste_box=pbox, paste_feather=r)
        full_bbox = runner.run(lbl[K:], box[K:], paste_into=video, paste_box=pbox, paste_feather=r, paste_feather_from="bbox")
    inset = frames.FrameLoader(dev).feather_inset(r)
    rect = np.zeros((F, 256, 256), np.uint8)
    rect[:, inset:256 - inset, inset:256 - inset] = 255
    want = pc.expect_numpy(video, small, pbox, None, fc.expect_numpy(rect, r))
    assert np.array_equal(full_box, want) and not np.array_equal(want, pc.expect_numpy(video, small, pbox))
    tb = (box[K:].cpu().numpy() != 0).astype(np.uint8)
    assert 0 < int(tb.sum()) < tb.size
    want = pc.expect_numpy(video, small, pbox, None, fc.expect_numpy(tb, r, binary=True))
    assert np.array_equal(full_bbox, want) and not np.array_equal(full_bbox, full_box)
