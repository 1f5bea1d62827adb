"""The image side of the loaders on the device (wacv23_tsnet_amd/frames.py, csrc/frames.hpp): decoded frames -> crop -> Pillow's bicubic resize ->
(pose: black bars to 256 x 256) -> BGR - IMG_MEAN.  Everything here is EQUALITY: Pillow's 8-bit resampler is integer arithmetic on coefficient
tables, the tables are restated in its operation order, and the kernel does the integer work.
  * the tables (Python restatement and the C entry) applied by a few lines of numpy reproduce Image.resize on random images;
  * the kernel on the g11_frames_* fixtures (the cropped regions of the reference's demo frames) reproduces the `in_src_bgr` bytes stored with
    the g10 goldens -- what the reference loader's own statements produced (oracle/capture_demo_input_goldens.py) -- on all 12 frames;
  * the kernel against live Pillow on random frames: up / down scaling, a skipped pass, boxes leaving the frame, 1-pixel boxes, batches,
    sizes that are not multiples of the tile;
  * argument errors; and on the GPU the same checks through the HIP library, the end-to-end forward and the stream-order property.
The fixtures are the contract.  A live-Pillow case that disagrees under another Pillow version while the fixture test passes points at that
version's resampler, not at the kernel."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import helpers as Hh
from wacv23_tsnet_amd import demo, frames

SHAPES = [(244, 256), (274, 256), (390, 128), (780, 256), (370, 128), (742, 256), (256, 256), (31, 256), (1024, 64), (77, 512)]
PAIRS = {"test114": ("g10_face_test114_to_val024_b1", "face"), "val024": ("g10_face_val024_to_test114_b2", "face"),
         "00110": ("g10_pose_00110_to_00164_b1", "pose"), "00164": ("g10_pose_00164_to_00110_b2", "pose")}
PIL_NOTE = "live Pillow %s disagrees; if test_kernel_on_fixtures_emulated passes, the fixtures (the contract) hold and this Pillow's resampler differs" % Image.__version__


def _apply(a, axis, table):
    """one pass of Pillow's 8-bit resampler along `axis` of a uint8 (h, w, 3) array, in numpy"""
    first, count, coef = table
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((len(first),) + a.shape[1:], np.uint8)
    for o in range(len(first)):
        acc = (1 << 21) + np.tensordot(coef[o, :count[o]].astype(np.int64), a[first[o]:first[o] + count[o]], axes=1)
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def _fixture(clip):
    z = np.load(os.path.join(Hh.GOLD, f"g11_frames_{clip}.npz"))
    return json.loads(str(z["meta"])), z["crops"]


def _expected(clip):
    z = np.load(os.path.join(Hh.GOLD, PAIRS[clip][0] + ".npz"))
    meta = json.loads(str(z["meta"]))
    assert meta["source"][0] == clip
    mean = np.asarray(meta["img_mean_bgr"], dtype=np.float32)
    assert np.array_equal(mean, demo.IMG_MEAN)
    return meta, torch.from_numpy(z["in_src_bgr"].astype(np.float32) - mean).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("n_in,n_out", SHAPES)
def test_tables_reproduce_pillow(emu_lib, n_in, n_out):
    tp = frames.bicubic_table(n_in, n_out)
    tc = frames.bicubic_table_c(emu_lib, n_in, n_out)
    for a, b in zip(tp, tc):
        assert a.dtype == np.int32 and np.array_equal(a, b)                 # the Python restatement == the C entry
    taps = 2 * int(np.ceil(2 * max(n_in / n_out, 1.0))) + 1
    assert tp[2].shape == (n_out, taps) and emu_lib.tsnet_bicubic_taps(n_in, n_out) == taps == frames.bicubic_taps(n_in, n_out)
    assert tp[1].max() <= taps and tp[0].min() >= 0 and (tp[0] + tp[1]).max() <= n_in
    rng = np.random.default_rng(n_in * 1000 + n_out)
    other = 37
    for axis in (0, 1):                                                     # the table drives the vertical and the horizontal pass alike
        shape = (n_in, other, 3) if axis == 0 else (other, n_in, 3)
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        size = (other, n_out) if axis == 0 else (n_out, other)              # PIL (w, h); the other axis keeps its size: that pass is skipped
        want = np.asarray(Image.fromarray(img).resize(size))
        got = _apply(img, axis, tp) if n_in != n_out else img
        assert np.array_equal(got, want), (n_in, n_out, axis, PIL_NOTE)


def _check_fixtures(lib, dev):
    ld = frames.FrameLoader(dev, lib=lib)
    report = {}
    for clip, (gold, model) in PAIRS.items():
        meta, crops = _fixture(clip)
        _, want = _expected(clip)
        x0, y0, x1, y1 = meta["box"]
        assert crops.shape == (3, y1 - y0, x1 - x0, 3)
        if model == "face":
            got = ld.face(crops, [0, y1 - y0, 0, x1 - x0])
        else:
            got = ld.pose(crops, (0, 0, x1 - x0, y1 - y0))
        got = got.cpu()
        report[clip] = dict(frames=int(crops.shape[0]), differing=int((got != want).sum()))
        assert got.dtype == torch.float32 and torch.equal(got, want), report
        # the same region inside a full frame, addressed by the clip's own crop box (the pixels around it must not matter: noise there)
        W, H = meta["frame_size"]
        full = np.random.default_rng(1).integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        ys, ye, xs, xe = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
        full[:, ys:ye, xs:xe] = crops[:, ys - y0:ye - y0, xs - x0:xe - x0]
        got2 = (ld.face(full, [y0, y1, x0, x1]) if model == "face" else ld.pose(full, (x0, y0, x1, y1))).cpu()
        report[clip]["differing_in_frame"] = int((got2 != want).sum())
        assert torch.equal(got2, want), report
        if model == "pose":                                                # resize_square's bars: byte 0 -> -mean
            bars = torch.from_numpy(-demo.IMG_MEAN).view(1, 3, 1, 1).expand(3, 3, 256, 64)
            assert torch.equal(got[:, :, :, :64], bars) and torch.equal(got[:, :, :, 192:], bars)
    return report


def _pil(frame, box, size, square=False):
    im = Image.fromarray(frame).crop(box).resize(size)
    a = np.asarray(im)
    if square:
        S = max(size)
        full = np.zeros((S, S, 3), np.uint8)
        py, px = (S - size[1]) // 2, (S - size[0]) // 2
        full[py:py + size[1], px:px + size[0]] = a
        a = full
    return torch.from_numpy(a[:, :, ::-1].astype(np.float32) - demo.IMG_MEAN).permute(2, 0, 1)


# (frame (h, w), F, box, size (ow, oh), square)
LIVE = [((480, 640), 1, (121, 17, 365, 261), (256, 256), False),           # upscale, the face shape
        ((480, 640), 3, (100, 40, 500, 440), (100, 120), False),           # downscale 4x / 3.3x, F > 1, sizes off the 64 x 32 tile
        ((300, 200), 2, (10, 20, 170, 280), (48, 260), False),             # 3.3x down horizontally, vertical pass skipped (260 -> 260)
        ((300, 200), 1, (10, 20, 170, 280), (160, 97), False),             # horizontal pass skipped
        ((300, 200), 2, (30, 50, 130, 200), (100, 150), False),            # both skipped: a plain crop
        ((480, 640), 2, (-20, -31, 250, 239), (256, 256), False),          # leaves the frame at the left and the top
        ((480, 640), 2, (500, 300, 700, 520), (77, 131), False),           # ... at the right and the bottom
        ((480, 640), 1, (-30, -30, 670, 510), (90, 70), False),            # ... on all four sides
        ((480, 640), 2, (320, 100, 321, 300), (40, 50), False),            # a 1-pixel-wide box
        ((480, 640), 1, (100, 240, 300, 241), (64, 32), False),            # a 1-pixel-high box
        ((1080, 1920), 2, (841, 206, 1231, 986), (128, 256), True),        # the pose shape with its bars
        ((200, 500), 2, (0, 0, 500, 200), (130, 40), True),                # bars above and below (odd split)
        ((900, 90), 1, (5, 0, 85, 900), (33, 40), False)]                  # 22.5x down vertically: the tile height shrinks


def _check_live(lib, dev, cases=LIVE):
    ld = frames.FrameLoader(dev, lib=lib)
    rng = np.random.default_rng(11)
    report = []
    for (h, w), F, box, size, square in cases:
        fr = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
        fr[:, ::7, ::5] = 255; fr[:, 3::11, 2::9] = 0                      # hard edges: the negative lobes clip at both ends
        got = ld.prepare(fr if F == 1 else torch.from_numpy(fr), box, size, square=square).cpu()
        want = torch.stack([_pil(fr[f], box, size, square) for f in range(F)])
        report.append(dict(frame=[h, w], F=F, box=list(box), size=list(size), differing=int((got != want).sum())))
        assert got.shape == want.shape and torch.equal(got, want), (report[-1], PIL_NOTE)
        if F > 1:
            assert not torch.equal(got[0], got[1])
    return report


def _device_check(lib, dev):
    return dict(fixtures=_check_fixtures(lib, dev), live=_check_live(lib, dev))


def test_kernel_on_fixtures_emulated(emu_lib):
    _check_fixtures(emu_lib, "cpu")


def test_kernel_vs_live_pillow_emulated(emu_lib):
    _check_live(emu_lib, "cpu")


def test_custom_mean_and_spellings(emu_lib):
    ld = frames.FrameLoader("cpu", lib=emu_lib)
    fr = np.random.default_rng(2).integers(0, 256, (1, 60, 80, 3), dtype=np.uint8)
    a = ld.prepare(fr, (5, 6, 70, 50), (32, 24), mean=(1.0, 2.0, 3.0))
    b = ld.prepare(fr, (5, 6, 70, 50), (32, 24), mean=(0.0, 0.0, 0.0))
    assert torch.equal(a, b - torch.tensor([1.0, 2.0, 3.0]).view(1, 3, 1, 1))
    assert torch.equal(ld.face(fr, [6, 50, 5, 70], size=(32, 24)), ld.prepare(fr, (5, 6, 70, 50), (32, 24)))
    assert ld.pose(fr, (5, 6, 70, 50)).shape == (1, 3, 256, 256)
    with pytest.raises(ValueError):
        ld.prepare(fr[0], (0, 0, 4, 4), (4, 4))
    with pytest.raises(ValueError):
        ld.prepare(fr.astype(np.float32), (0, 0, 4, 4), (4, 4))


def test_argument_errors_write_nothing(emu_lib):
    lib = emu_lib
    fr = torch.zeros((1, 20, 30, 3), dtype=torch.uint8)
    out = torch.full((1, 3, 16, 16), 7.0)
    mean = (frames.C.c_float * 3)(0.0, 0.0, 0.0)
    tx = [torch.from_numpy(np.ascontiguousarray(t)) for t in frames.bicubic_table(10, 16)]
    taps = frames.bicubic_taps(10, 16)

    def call(box=(0, 0, 10, 10), xt=taps, yt=taps, oh=16, ow=16, pt=0, pl=0, OH=16, OW=16, F=1, frames_ptr=fr.data_ptr(), tabs=True):
        p = [t.data_ptr() if tabs else None for t in tx]
        return lib.tsnet_prepare_frames(frames_ptr, F, 20, 30, *box, p[0], p[1], p[2], xt, p[0], p[1], p[2], yt, oh, ow, pt, pl, OH, OW, mean,
                                        out.data_ptr(), None)

    assert call() == 0 and not torch.equal(out, torch.full_like(out, 7.0))
    out.fill_(7.0)
    bad = [dict(box=(5, 0, 5, 10)), dict(box=(0, 9, 10, 3)),                # empty boxes
           dict(xt=taps - 2), dict(yt=taps + 2),                            # a table narrower / wider than the size ratio's: count > taps
           dict(pt=1), dict(pl=-1), dict(OH=15), dict(OW=8),                # padding that does not fit
           dict(F=0), dict(frames_ptr=None), dict(tabs=False), dict(oh=0)]
    for kw in bad:
        assert call(**kw) == -1, kw                                         # TSNET_ERR_ARG
        assert lib.tsnet_op_last_error().decode(), kw
        assert torch.equal(out, torch.full_like(out, 7.0)), kw
    assert lib.tsnet_bicubic_taps(0, 5) == -1 and lib.tsnet_bicubic_table(4, 0, None, None, None) == -1


# ------------------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_kernel_gpu():
    rep = _device_check(None, "cuda")
    print("[frames] " + json.dumps(rep))
    out_dir = os.environ.get("TSNET_REPORT_DIR")                     # where the caller collects reports, if anywhere
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "frames_report.json"), "w") as f:
            json.dump(rep, f)


def _prepared_sources(ld, clip, B):
    meta, crops = _fixture(clip)
    x0, y0, x1, y1 = meta["box"]
    box = (0, 0, x1 - x0, y1 - y0)
    img = ld.pose(torch.from_numpy(crops), box) if PAIRS[clip][1] == "pose" else ld.prepare(torch.from_numpy(crops), box, (256, 256))
    return [img[k:k + 1].repeat(B, 1, 1, 1) for k in range(img.shape[0])]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", ["test114", "00110"])
def test_end_to_end_forward_on_loaded_frames(clip):
    """The sources prepared on the device from the fixture ARE the golden's src_img; the forward on them meets the golden's gates (those of
    tests/test_gpu_seed_sweep.py against the stored fp32 reference: 1e-3 on crops / lattice, W x 1e-3 on the row sums, 1e-4 on the flows)."""
    name = PAIRS[clip][0]
    meta, z, cfg, sd, inputs = Hh.golden_case(name)
    ld = frames.FrameLoader("cuda")
    src = _prepared_sources(ld, clip, meta["B"])
    for k in range(cfg.n_source):
        assert torch.equal(src[k].cpu(), inputs[0][k]), (clip, k)
    eng = Hh.make_engine(cfg, sd, meta["H"], meta["W"], meta["B"], "cuda")
    has_flow = meta.get("has_flow", True)
    rec, flows = Hh.run_engine(eng, (src,) + tuple(inputs[1:]), "cuda", return_flow=has_flow)
    eng.close()
    views = {"c": (slice(96, 128), slice(96, 128)), "tl": (slice(0, 16), slice(0, 16)), "br": (slice(meta["H"] - 16, meta["H"]), slice(meta["W"] - 16, meta["W"]))}
    if "rec32_sub4" in z.files:
        views["sub4"] = (slice(None, None, 4), slice(None, None, 4))
    d_gold = max(float(np.abs(rec[:, :, ys, xs].numpy() - z[f"rec32_{tag}"]).max()) for tag, (ys, xs) in views.items())
    d_rows = float(np.abs(rec.double().sum(dim=3).numpy() - z["rec32_rowsum"]).max())
    d_flow = max(float(np.abs(flows[i].numpy() - z[f"flow32_{i}"]).max()) for i in range(cfg.n_source)) if has_flow else 0.0
    print(f"[frames-e2e] {name}: rec {d_gold:.3e} rowsum {d_rows:.3e} flow {d_flow:.3e}")
    assert d_gold <= 1e-3 and d_rows <= meta["W"] * 1e-3 and d_flow <= 1e-4


@pytest.mark.gpu
def test_prepare_is_stream_ordered():
    """prepare -> set_sources -> forward_target enqueued back to back on one stream, no synchronisation in between, gives the frame obtained
    with a synchronisation after every call."""
    clip = "test114"
    meta, z, cfg, sd, inputs = Hh.golden_case(PAIRS[clip][0])
    dev = torch.device("cuda", 0)
    eng = Hh.make_engine(cfg, sd, meta["H"], meta["W"], meta["B"], "cuda")
    ld = frames.FrameLoader(dev)
    lbl, box = [t.cuda() for t in inputs[1]], [t.cuda() for t in inputs[2]]
    tl, tb = inputs[3].cuda(), inputs[4].cuda()
    fmeta, crops = _fixture(clip)
    crops_d = torch.from_numpy(crops).cuda()
    cbox = (0, 0, crops.shape[2], crops.shape[1])
    # with a synchronisation after every call (this also uploads the tables, so the second round is enqueue-only)
    img = ld.prepare(crops_d, cbox, (256, 256)); torch.cuda.synchronize()
    eng.set_sources([img[k:k + 1].repeat(meta["B"], 1, 1, 1) for k in range(3)], lbl, box); torch.cuda.synchronize()
    want, _ = eng.forward_target(tl, tb); torch.cuda.synchronize()
    want = want.clone()
    # sources that differ, so that a stale source set would show
    eng.set_sources([torch.zeros_like(img[:1]).repeat(meta["B"], 1, 1, 1) for _ in range(3)], lbl, box); torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        junk = torch.empty((64, 1024, 1024), device=dev).normal_()          # work in front of the kernel: the stream is busy when it is enqueued
        img2 = ld.prepare(crops_d, cbox, (256, 256))
        eng.set_sources([img2[k:k + 1].repeat(meta["B"], 1, 1, 1) for k in range(3)], lbl, box)
        got, _ = eng.forward_target(tl, tb)
    stream.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(img2, img)
    del junk
    eng.close()
