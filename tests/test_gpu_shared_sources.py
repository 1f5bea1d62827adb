"""GPU tier: clip mode with ONE source set shared by a batch of driving frames (tsnet_set_sources_shared) at the reference width.  The
shared cache holds K encoded images; forward_target on B driving frames must give, bit for bit, the one-shot forward on the same sources
replicated B times -- at every B up to max_batch against one cache -- and demo.ClipRunner(batch=4) the bytes of ClipRunner(batch=1)."""
import os
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
from oracle import tsnet_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _case(cfg, B, H, W, wseed, iseed, mask="box", bias_std=0.02):
    """(weights, one source set of batch 1, B driving frames)"""
    sd = O.synth_state_dict(cfg, seed=wseed, bias_std=bias_std)
    src = O.synth_inputs(cfg, 1, H, W, seed=iseed, mask_mode=mask)[:3]
    drv = O.synth_inputs(cfg, B, H, W, seed=iseed + 1, mask_mode=mask)[3:]
    return sd, src, drv


def _rep(src, n):
    return tuple([x.repeat(n, *([1] * (x.dim() - 1))) for x in part] for part in src)


def _shared(eng, src, tar_lbl, tar_bbox, return_flow=True, set_sources=True):
    if set_sources:
        eng.set_sources(*[[t.to(DEV) for t in part] for part in src], shared=True)
    rec, flows = eng.forward_target(tar_lbl.to(DEV), tar_bbox.to(DEV), return_flow=return_flow)
    torch.cuda.synchronize()
    return rec.cpu(), ([f.cpu() for f in flows] if flows is not None else None)


def test_full_size_shared_equals_replicated():
    """cfg1 shape (256 x 256, K = 3, ngf 64), n_blocks = 4, max_batch = 4."""
    cfg = O.TSNetConfig(label_nc=2, n_blocks=4, n_source=3)
    sd, src, (tl, tb) = _case(cfg, 4, 256, 256, 21, 22)
    eng = Hh.make_engine(cfg, sd, 256, 256, 4, DEV)
    ref_rec, ref_flows = Hh.run_engine(eng, (*_rep(src, 4), tl, tb), DEV)
    rec, flows = _shared(eng, src, tl, tb)
    assert torch.equal(rec, ref_rec) and all(torch.equal(a, b) for a, b in zip(flows, ref_flows))
    assert eng.stage("src_fea", DEV).shape[0] == 3
    # every smaller batch, anywhere in the clip, against the SAME cache
    for lo, hi in ((0, 1), (3, 4), (0, 2), (2, 4), (1, 4), (0, 3)):
        r, f = _shared(eng, src, tl[lo:hi], tb[lo:hi], set_sources=False)
        assert torch.equal(r, ref_rec[lo:hi]), (lo, hi)
        assert all(torch.equal(a, b[lo:hi]) for a, b in zip(f, ref_flows)), (lo, hi)
    # the per-batch cache keeps its rule
    eng.set_sources(*[[t.to(DEV) for t in part] for part in _rep(src, 4)])
    with pytest.raises(RuntimeError, match="batch differs from the cached sources"):
        eng.forward_target(tl[:2].to(DEV), tb[:2].to(DEV))
    eng.close()


def test_large_map_shared_equals_replicated():
    """configs[4] shape: 512 x 512, K = 5, bf16 operands, max_batch = 2 -- 4096 positions: flow_kernel_p."""
    cfg = O.TSNetConfig(label_nc=2, n_blocks=0, n_source=5)
    sd, src, (tl, tb) = _case(cfg, 2, 512, 512, 25, 26, mask="bernoulli")
    eng = Hh.make_engine(cfg, sd, 512, 512, 2, DEV, operands="bf16")
    assert eng.lib.tsnet_flow_plan(2, 64, 64, 512) >= 1
    ref_rec, ref_flows = Hh.run_engine(eng, (*_rep(src, 2), tl, tb), DEV)
    rec, flows = _shared(eng, src, tl, tb)
    assert torch.equal(rec, ref_rec) and all(torch.equal(a, b) for a, b in zip(flows, ref_flows))
    r1, f1 = _shared(eng, src, tl[1:2], tb[1:2], set_sources=False)
    assert torch.equal(r1, ref_rec[1:2]) and all(torch.equal(a, b[1:2]) for a, b in zip(f1, ref_flows))
    eng.close()


def test_pose_shared():
    """The pose model: 25 labels, fixed-background composite, B = 4."""
    cfg = O.TSNetConfig(label_nc=25, n_blocks=4, n_source=3, pose=True)
    sd, src, (tl, tb) = _case(cfg, 4, 256, 256, 23, 24)
    eng = Hh.make_engine(cfg, sd, 256, 256, 4, DEV)
    ref_rec, ref_flows = Hh.run_engine(eng, (*_rep(src, 4), tl, tb), DEV)
    rec, flows = _shared(eng, src, tl, tb)
    assert torch.equal(rec, ref_rec) and all(torch.equal(a, b) for a, b in zip(flows, ref_flows))
    r, _ = _shared(eng, src, tl[1:4], tb[1:4], return_flow=False, set_sources=False)
    assert torch.equal(r, ref_rec[1:4])
    eng.close()


def test_clip_runner_batches(tmp_path):
    """ClipRunner(batch=4) on F = 6 driving frames (groups 4 + 2) writes the bytes of ClipRunner(batch=1)."""
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
    src = (src_img, [lbl[i:i + 1] for i in range(K)], [box[i:i + 1] for i in range(K)])
    with demo.ClipRunner(model, *src) as r1:
        want = r1.run(lbl[K:], box[K:], out_dir=str(tmp_path / "b1"), name="t")
    with demo.ClipRunner(model, *src, batch=4) as r4:
        got = r4.run(lbl[K:], box[K:], out_dir=str(tmp_path / "b4"), name="t")
        one = r4.frame(lbl[K + 4:K + 5], box[K + 4:K + 5]).cpu().numpy()           # frame() keeps working on the batched runner
        with pytest.raises(ValueError, match="batch 4"):
            r4.frames(lbl[K:K + 5], box[K:K + 5])
    assert want.shape == (F, 256, 256, 3) and want.dtype == np.uint8
    assert np.array_equal(got, want) and np.array_equal(one, want[4])
    assert len({want[i].tobytes() for i in range(F)}) == F                          # six different frames: a group mix-up would show
    for i in range(F):
        a = np.asarray(Image.open(tmp_path / "b1" / f"{i:06d}_t.png").convert("RGB"))
        b = np.asarray(Image.open(tmp_path / "b4" / f"{i:06d}_t.png").convert("RGB"))
        assert a.shape == (256, 768, 3) and np.array_equal(a, b)
    assert Image.open(tmp_path / "b4" / "t.gif").n_frames == F == Image.open(tmp_path / "b1" / "t.gif").n_frames


def test_shared_is_stream_ordered():
    """set_sources(shared=True) and two forward_target calls enqueued back to back on one stream, no synchronisation in between, give the
    frames obtained with a synchronisation after every call."""
    cfg = O.TSNetConfig(label_nc=2, n_blocks=1, n_source=3)
    sd, src, (tl, tb) = _case(cfg, 4, 256, 256, 27, 28)
    dev = torch.device("cuda", 0)
    eng = Hh.make_engine(cfg, sd, 256, 256, 4, DEV)
    srcd = [[t.to(dev) for t in part] for part in src]
    tl, tb = tl.to(dev), tb.to(dev)
    eng.set_sources(*srcd, shared=True); torch.cuda.synchronize()
    want4, _ = eng.forward_target(tl, tb); torch.cuda.synchronize()
    want2, _ = eng.forward_target(tl[1:3], tb[1:3]); torch.cuda.synchronize()
    want4, want2 = want4.clone(), want2.clone()
    assert torch.equal(want2, want4[1:3])
    # sources that differ, so that a stale source set would show
    eng.set_sources([torch.zeros_like(t) for t in srcd[0]], srcd[1], srcd[2], shared=True); torch.cuda.synchronize()
    stale, _ = eng.forward_target(tl, tb); torch.cuda.synchronize()
    assert not torch.equal(stale, want4)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        junk = torch.empty((64, 1024, 1024), device=dev).normal_()          # work in front of the kernels: the stream is busy when they are enqueued
        eng.set_sources(*srcd, shared=True)
        got4, _ = eng.forward_target(tl, tb)
        got2, _ = eng.forward_target(tl[1:3], tb[1:3])
    stream.synchronize()
    assert torch.equal(got4, want4) and torch.equal(got2, want2)
    del junk
    eng.close()
