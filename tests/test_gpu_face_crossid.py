"""GPU tier of the cross-identity face path (tests/test_face_crossid.py is the CPU tier): the HIP library draws the reference's maps from
FRACTIONAL landmarks -- the device kernels were pinned on integer landmarks only (tests/test_raster.py) -- and the labels made from
face_driving_keypoints drive the generator through ClipRunner with the bits of the one-shot forward."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as Hh

pytestmark = pytest.mark.gpu


def _gold():
    z12 = np.load(os.path.join(Hh.GOLD, "g12_face_crossid.npz"))
    z7 = np.load(os.path.join(Hh.GOLD, "g7_raster_face.npz"))
    return json.loads(str(z12["meta"]))["pairs"], z12, z7, json.loads(str(z7["meta"]))["clips"]


def _frame_coords(kp_rel, crop):
    kp = kp_rel.copy()                                   # integer landmarks: adding the crop back is exact
    kp[:, :, 0] += crop[2]
    kp[:, :, 1] += crop[0]
    return kp


def test_device_maps_from_fractional_landmarks_equal_the_reference():
    """rasterise(relative=True) of the reference's adapted and smoothed points on the HIP library: its edge maps and box masks, byte for
    byte, on the 38 frames at 274 x 274 and the 40 frames at 244 x 244."""
    from wacv23_tsnet_amd import _lib, raster
    meta, z12, _, _ = _gold()
    r = raster.FaceRasteriser("cuda", lib=_lib.load())
    frames = 0
    for name, m in meta.items():
        w, h = m["size"]
        want_e = (np.unpackbits(z12[f"{name}_edges"], axis=-1)[:, :, :w] * 255).astype(np.uint8)
        want_b = (np.unpackbits(z12[f"{name}_bbox"], axis=-1)[:, :, :w] * 255).astype(np.uint8)
        edges, bbox, crop, bw = r.rasterise(list(z12[f"{name}_smoothed"]), tuple(m["crop"]), relative=True)
        torch.cuda.synchronize()
        got_e, got_b = edges.cpu().numpy(), bbox.cpu().numpy()
        ham = (got_e != want_e).reshape(got_e.shape[0], -1).sum(axis=1)
        print(f"[face_crossid gpu] {name}: {got_e.shape[0]} frames of {h} x {w}, {int((ham > 0).sum())} differ, hamming {int(ham.sum())}")
        assert bw == m["bw"] and got_e.shape == (m["frames"], h, w)
        assert np.array_equal(got_e, want_e), (name, ham.tolist())
        assert np.array_equal(got_b, want_b), name
        frames += got_e.shape[0]
    assert frames == 78


def test_crossid_labels_through_clip_runner_carry_the_forward_bits():
    """The smallest model of the goldens (64 x 64 frames, K = 3, n_blocks = 0, as g3_face_64_*): subject test114 driven by val024.  Labels from
    face_driving_keypoints -> rasterise(relative=True) -> resize_label(size=(64, 64)) -> vl2ch; ClipRunner(batch=4) on 6 driving frames
    (groups of 4 and 2) returns the bits of tsnet_forward on the same tensors, and the frames it writes are their post-processing."""
    from wacv23_tsnet_amd import demo, raster
    from wacv23_tsnet_amd.model import TSNet
    meta, z12, z7, clips = _gold()
    m = meta["test114_to_val024"]
    dev = torch.device("cuda", 0)
    K, F, S = 3, 6, (64, 64)
    sub = _frame_coords(z7["test114_keypoints"], clips["test114"]["crop"])
    drv = _frame_coords(z7["val024_keypoints"], clips["val024"]["crop"])
    rs = raster.FaceRasteriser(dev)
    pts, crop, bw = raster.face_driving_keypoints(list(sub), list(drv))
    assert list(crop) == m["crop"] and bw == m["bw"] and np.array_equal(pts, z12["test114_to_val024_smoothed"])
    edges, bbox, _, _ = rs.rasterise(list(pts[:F]), crop, relative=True)
    tar_lbl, tar_box = rs.vl2ch(demo.resize_label(edges, size=S), 2), demo.resize_label(bbox, size=S)
    raw_e, raw_b, _, _ = rs.rasterise(list(drv[:F]))                                       # the driver's own face: what the labels were before
    raw_lbl = rs.vl2ch(demo.resize_label(raw_e, size=S), 2)
    se, sb, _, _ = rs.rasterise(list(sub[[0, 13, 26]]))
    src_lbl, src_box = rs.vl2ch(demo.resize_label(se, size=S), 2), demo.resize_label(sb, size=S)
    assert tar_lbl.shape == (F, 2, 64, 64) and torch.equal(tar_lbl.sum(dim=1), torch.ones_like(tar_lbl[:, 0]))
    assert (tar_lbl[:, 1].flatten(1).sum(dim=1) > 0).all() and (tar_box.flatten(1).sum(dim=1) > 0).all()      # thin at 64 x 64 (a dozen edge pixels), not empty
    assert all(not torch.equal(tar_lbl[i], raw_lbl[i]) for i in range(F))                  # every driving label changed, at 64 x 64 too
    torch.manual_seed(0)
    model = TSNet(is_train=False, label_nc=2, n_blocks=0, n_downsampling=3, n_source=K, height=64, width=64).cuda()
    g = torch.Generator().manual_seed(1)
    src_img = [(torch.rand((1, 3, 64, 64), generator=g) * 255.0 - torch.from_numpy(demo.IMG_MEAN).view(1, 3, 1, 1)) for _ in range(K)]
    src = (src_img, [src_lbl[i:i + 1] for i in range(K)], [src_box[i:i + 1] for i in range(K)])
    with demo.ClipRunner(model, *src, batch=4) as runner:
        recs = []
        for lo, hi in ((0, 4), (4, 6)):                                                    # the groups run() makes of 6 frames
            rec, _ = runner.eng.forward_target(tar_lbl[lo:hi], tar_box[lo:hi])
            recs.append(rec.clone())
        frames = runner.run(tar_lbl, tar_box)
        want_rec = []
        for lo, hi in ((0, 4), (4, 6)):                                                    # tsnet_forward: the sources of every batch element given
            n = hi - lo
            model.set_test_input([x.repeat(n, 1, 1, 1) for x in src[0]], [x.repeat(n, 1, 1, 1) for x in src[1]], [x.repeat(n, 1, 1) for x in src[2]],
                                 tar_lbl[lo:hi], tar_box[lo:hi])
            model.forward()
            want_rec.append(model.rec_tar_img.clone())
        torch.cuda.synchronize()
        got, want = torch.cat(recs).cpu(), torch.cat(want_rec).cpu()
        assert got.shape == (F, 3, 64, 64) and torch.isfinite(want).all()
        assert torch.equal(got, want)                                                      # bits
        assert frames.shape == (F, 64, 64, 3) and np.array_equal(frames, runner.post(torch.cat(want_rec)).cpu().numpy())
        assert len({frames[i].tobytes() for i in range(F)}) == F                           # six different frames: a group mix-up would show
