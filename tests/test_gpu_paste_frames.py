"""GPU tier of the paste-back path (tsnet_paste_frames, FrameLoader.paste, ClipRunner.run(paste_into=...)): the cases of paste_cases.py through
the HIP library, equal to the numpy restatement byte for byte with the sentinels around the frames intact; the stream-order property; and the
clip harness pasting its own frames."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import paste_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_cases_gpu():
    from wacv23_tsnet_amd import _lib, frames
    lib, dev = _lib.load(), torch.device("cuda", 0)
    ld = frames.FrameLoader(dev)
    rep = [pc.check_variant(lib, dev, ld, vid) for vid, _, _ in pc.variants()]
    rep.append(pc.check_too_steep(lib, dev, ld))
    print("[paste] " + json.dumps(rep))
    out_dir = os.environ.get("TSNET_REPORT_DIR")                     # where the caller collects reports, if anywhere
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "paste_report.json"), "w") as f:
            json.dump(rep, f)


def test_paste_is_stream_ordered():
    """DemoPostprocessor -> paste enqueued back to back on a busy side stream, no synchronisation in between, gives the frames obtained with
    a synchronisation after every call."""
    from wacv23_tsnet_amd import demo, frames
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    ref = (torch.rand((1, 3, 256, 256), generator=g) * 255.0 - torch.from_numpy(demo.IMG_MEAN).view(1, 3, 1, 1)).to(dev)
    rec = (torch.rand((2, 3, 256, 256), generator=g) * 2.0 - 1.0).to(dev)
    fr = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (2, 480, 640, 3), dtype=np.uint8)).to(dev)
    mask = torch.from_numpy(pc.make_mask("stream", "bands", 2, 256, 256)).to(dev)
    box = (-21, 17, 253, 291)
    post, ld = demo.DemoPostprocessor(ref), frames.FrameLoader(dev)
    # with a synchronisation after every call (this also uploads the tables, so the second round is enqueue-only)
    gen = post(rec); torch.cuda.synchronize()
    want = ld.paste(gen, fr, box, mask=mask); torch.cuda.synchronize()
    assert np.array_equal(want.cpu().numpy(), pc.expect_numpy(fr.cpu().numpy(), gen.cpu().numpy(), box, None, mask.cpu().numpy()))
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        junk = torch.empty((64, 1024, 1024), device=dev).normal_()          # work in front of the kernels: the stream is busy when they are enqueued
        got = ld.paste(post(rec), fr, box, mask=mask)
    stream.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, fr)
    del junk


def test_clip_runner_pastes_its_frames(tmp_path):
    """ClipRunner.run(paste_into=...) on the tiny face model: 6 driving frames at batch 4 (a ragged last group), a box leaving the frame.  The
    full frames equal the numpy restatement applied to the runner's own 256 x 256 bytes from a run without paste_into."""
    import demo_clip
    from PIL import Image
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
    pbox = (170, -40, 370, 160)                                             # 256 -> 200 both ways; leaves the frame at the top and the right
    with demo.ClipRunner(model, src_img, [lbl[i:i + 1] for i in range(K)], [box[i:i + 1] for i in range(K)], batch=4) as runner:
        small = runner.run(lbl[K:], box[K:])
        keep = video.copy()
        full = runner.run(lbl[K:], box[K:], out_dir=str(tmp_path / "out"), name="t", paste_into=video, paste_box=pbox)
        full_d = runner.run(lbl[K:], box[K:], paste_into=torch.from_numpy(video).to(dev), paste_box=pbox)
    assert small.shape == (F, 256, 256, 3) and full.shape == video.shape and full.dtype == np.uint8
    assert np.array_equal(video, keep)                                      # paste_into is left as it is
    want = pc.expect_numpy(video, small, pbox)
    assert np.array_equal(full, want) and np.array_equal(full_d, want) and not np.array_equal(want, video)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "000005_t_full.png").convert("RGB")), want[5])
    strip = np.asarray(Image.open(tmp_path / "out" / "000004_t.png").convert("RGB"))
    assert strip.shape == (256, 768, 3) and np.array_equal(strip[:, 512:], small[4])
    assert Image.open(tmp_path / "out" / "t.gif").n_frames == F
