"""GPU tier of the YUV 4:2:0 conversions (tsnet_rgb_to_yuv420, tsnet_yuv420_to_rgb, FrameLoader.to_yuv420 / from_yuv420,
ClipRunner.run(y4m=...), tools/demo_clip.py --y4m): the cases of yuv_cases.py through the HIP library, equal to the numpy restatement byte for
byte with the sentinels around every output intact; the two large frames with the round-trip bound; refusals that write nothing; the
stream-order property; the clip harness and the demo tool writing a Y4M file."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import yuv_cases as yc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_cases_gpu():
    from wacv23_tsnet_amd import _lib, frames
    lib, dev = _lib.load(), torch.device("cuda", 0)
    ld = frames.FrameLoader(dev)
    rep = [yc.check_case(lib, dev, ld, cid) for cid in yc.IDS]
    print("[yuv] " + json.dumps(rep))
    out_dir = os.environ.get("TSNET_REPORT_DIR")                     # where the caller collects reports, if anywhere
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "yuv_report.json"), "w") as f:
            json.dump(rep, f)


def test_large_frames_gpu():
    """(1, 4096, 4096): every colour once -- luma exhaustive, chroma on mixed blocks; (1, 1024, 1024): constant blocks over the lattice, and
    rgb -> yuv -> rgb within 1 per byte (full range) and 2 (limited)"""
    from wacv23_tsnet_amd import frames
    print("[yuv] round trip worst per table: " + json.dumps(yc.check_large(frames.FrameLoader(torch.device("cuda", 0)))))


def test_refusals_write_nothing_gpu():
    from wacv23_tsnet_amd import _lib
    lib, dev = _lib.load(), torch.device("cuda", 0)
    for cause in yc.ARG_ERRORS:
        yc.check_refusal(lib, dev, cause)
    torch.cuda.synchronize()


def test_conversion_is_stream_ordered():
    """a conversion enqueued on a busy side stream behind the kernel that writes its input, no synchronisation in between, sees that input"""
    from wacv23_tsnet_amd import frames
    dev = torch.device("cuda", 0)
    ld = frames.FrameLoader(dev)
    rgb = yc.make_rgb("stream", (4, 270, 482), "random")
    fwd, inv = yc.derive("bt709", False)
    want = yc.rgb_to_yuv(rgb, fwd, "nv12")
    want_back = torch.from_numpy(yc.yuv_to_rgb(want, 270, 482, inv, "nv12"))
    src = torch.from_numpy(rgb).to(dev)
    assert torch.equal(ld.to_yuv420(src, "nv12", "bt709", False).cpu(), torch.from_numpy(want))     # with a synchronisation; the tables are made here
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        junk = torch.empty((64, 1024, 1024), device=dev).normal_()          # work in front: the stream is busy when the kernels are enqueued
        late = torch.zeros_like(src)
        late.copy_(src)                                                     # the kernel that writes the conversion's input
        got = ld.to_yuv420(late, "nv12", "bt709", False)
        back = ld.from_yuv420(got, (270, 482), "nv12", "bt709", False)      # ... and the inverse behind the forward that writes ITS input
    stream.synchronize()
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert torch.equal(back.cpu(), want_back)
    del junk


def test_clip_runner_writes_y4m(tmp_path):
    """ClipRunner.run(y4m=...) on the tiny face model: 6 driving frames at batch 4 (a ragged last group), generated frames and full frames
    pasted at a box leaving the frame"""
    import demo_clip
    from wacv23_tsnet_amd import demo, frames, raster
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
    video = np.random.default_rng(8).integers(0, 256, (F, 201, 301, 3), dtype=np.uint8)
    with demo.ClipRunner(model, src_img, [lbl[i:i + 1] for i in range(K)], [box[i:i + 1] for i in range(K)], batch=4) as runner:
        small, full = yc.check_clip_runner(runner, frames.FrameLoader(dev), (lbl[K:], box[K:]), video, (170, -40, 370, 160), tmp_path)
    assert small.shape == (F, 256, 256, 3) and full.shape == video.shape


def test_demo_clip_writes_y4m(tmp_path, monkeypatch, capsys):
    """tools/demo_clip.py --paste-back --y4m: the header and the frame count are right, and the file's frames equal the restatement of the
    full frames the same run wrote as PNGs"""
    import demo_clip
    from PIL import Image
    out, path = str(tmp_path / "demo"), str(tmp_path / "out.y4m")
    monkeypatch.setattr(sys, "argv", ["demo_clip.py", "--out", out, "--frames", "5", "--batch", "2", "--n-blocks", "1", "--timing-frames", "4",
                                      "--paste-back", "--y4m", path])
    demo_clip.main()
    assert "--y4m: 5 frames of 640 x 480" in capsys.readouterr().out
    rd, got = yc.read_y4m(path)
    assert (rd.width, rd.height, rd.fps, rd.colourspace, rd.full_range) == (640, 480, (25, 1), "420jpeg", True) and got.shape == (5, 640 * 480 * 3 // 2)
    pngs = np.stack([np.asarray(Image.open(os.path.join(out, f"{i:06d}_synthetic_face_full.png")).convert("RGB")) for i in range(5)])
    assert np.array_equal(got, yc.rgb_to_yuv(pngs, yc.derive("bt601", True)[0], "i420"))
