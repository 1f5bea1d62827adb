"""Cross-identity face driving: the loader's key-point preparation of the driving clip (FaceDatasetTest.normalize_faces,
dataset/dataset_video_face.py:411-454, and the five-frame moving average, :357-379) as host code of the library (csrc/face_adapt.hpp), and
the label maps drawn from its FRACTIONAL points.  tests/golden/g12_face_crossid.npz holds what the imported reference computes on its two demo
pairs (tools/capture_face_crossid_fixtures.py): the 77 statistics, the adapted and the smoothed points as float64, edge maps and box masks.

  * statistics, adapted and smoothed points EQUAL the reference's doubles (== : bit for bit).  The library restates the reference's
    operations in their order -- sequential sums, sum / n, sqrt(dx*dx + dy*dy), two divisions, left-to-right evaluation -- so there is no
    rounding to allow for;
  * rasterise(relative=True) of the reference's smoothed points gives its edge maps and box masks byte for byte on all 78 frames, and the host
    fit on the fractional pieces equals scipy's curve_fit bit for bit (the rasteriser was pinned on integer landmarks only, tests/test_raster.py);
  * a clip adapted to itself stays where it is: the scales are 1 up to rounding.  Coordinates are below 512, where an ulp is 1.1e-13; a
    point goes through five roundings of that size and two scales within a few ulp of 1 applied to offsets below 512 -- 1e-10 leaves three
    orders of magnitude to spare and is far below anything a wrong scale or centre would give (the adaptation moves points by up to 12 px);
  * the smallest clips (F = 5, 6), where the head and tail formulas of the moving average meet, against a literal cumsum evaluation;
  * what is refused: F = 4, a driving clip without width, non-finite points, relative=True without a crop."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import helpers as Hh
from oracle import raster_oracle as RO
from wacv23_tsnet_amd import raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def gold():
    z12 = np.load(os.path.join(Hh.GOLD, "g12_face_crossid.npz"))
    z7 = np.load(os.path.join(Hh.GOLD, "g7_raster_face.npz"))
    meta = json.loads(str(z12["meta"]))["pairs"]
    assert sorted(meta) == ["test114_to_val024", "val024_to_test114"]
    assert sum(m["frames"] for m in meta.values()) == 78
    return meta, z12, z7


def _maps(z, name, w):
    return (np.unpackbits(z[f"{name}_edges"], axis=-1)[:, :, :w] * 255).astype(np.uint8), (np.unpackbits(z[f"{name}_bbox"], axis=-1)[:, :, :w] * 255).astype(np.uint8)


def _frame_coords(kp_rel, crop):
    """g7 stores the clips' INTEGER landmarks relative to the crop: adding the crop back is exact"""
    kp = kp_rel.copy()
    assert np.array_equal(kp, np.floor(kp))
    kp[:, :, 0] += crop[2]
    kp[:, :, 1] += crop[0]
    return kp


def test_adaptation_and_smoothing_equal_the_reference_bit_for_bit(emu_lib, gold):
    meta, z12, z7 = gold
    for name, m in meta.items():
        sub, drv = z7[f"{m['subject']}_keypoints"], z7[f"{m['driver']}_keypoints"]
        sub0, drv0 = sub.copy(), drv.copy()
        ad = raster.FaceAdapter(lib=emu_lib).fit(sub)
        assert ad.stats.shape == (77,) and ad.stats.dtype == np.float64
        assert np.array_equal(ad.stats, z12[f"{name}_stats"]), (name, np.abs(ad.stats - z12[f"{name}_stats"]).max())
        adapted = ad.apply(drv)
        assert adapted.dtype == np.float64 and np.array_equal(adapted, z12[f"{name}_adapted"]), (name, np.abs(adapted - z12[f"{name}_adapted"]).max())
        smoothed = raster.smooth_keypoints(adapted, lib=emu_lib)
        assert smoothed.dtype == np.float64 and np.array_equal(smoothed, z12[f"{name}_smoothed"]), (name, np.abs(smoothed - z12[f"{name}_smoothed"]).max())
        assert np.array_equal(sub, sub0) and np.array_equal(drv, drv0)                    # the caller's arrays are left alone
        assert np.abs(adapted - drv).max() == m["max_shift_px"] > 10                      # the adaptation is no small correction
        assert (smoothed != np.floor(smoothed)).mean() > 0.999                            # and its points are fractional


def test_relative_rasterise_equals_the_reference_maps(emu_lib, gold):
    meta, z12, _ = gold
    r = raster.FaceRasteriser("cpu", lib=emu_lib)
    for name, m in meta.items():
        w, h = m["size"]
        want_e, want_b = _maps(z12, name, w)
        pts = z12[f"{name}_smoothed"]
        keep = pts.copy()
        edges, bbox, crop, bw = r.rasterise(list(pts), tuple(m["crop"]), relative=True)
        assert tuple(crop) == tuple(m["crop"]) and bw == m["bw"] and edges.shape == (m["frames"], h, w)
        assert np.array_equal(pts, keep)
        ham = (edges.numpy() != want_e).reshape(m["frames"], -1).sum(axis=1)
        print(f"[face_crossid] {name}: {m['frames']} frames, {int((ham > 0).sum())} differ, hamming {int(ham.sum())}")
        assert np.array_equal(edges.numpy(), want_e), (name, ham.tolist())
        assert np.array_equal(bbox.numpy(), want_b), name
        # the default path subtracts the crop: relative points handed to it as frame coordinates draw another picture
        other, _, _, _ = r.rasterise(list(pts[:1]), tuple(m["crop"]))
        assert not np.array_equal(other.numpy(), want_e[:1])


def test_host_fit_on_fractional_pieces_equals_curve_fit(emu_lib, gold):
    """tsnet_fit_face_curves against scipy's curve_fit called as utils/keypoint2img.py:319-337 calls it (the way of
    tests/test_raster.py::test_host_fit_equals_curve_fit_bit_for_bit), on the fractional pieces of every third frame of both pairs."""
    import warnings
    from scipy.optimize import curve_fit
    meta, z12, _ = gold
    n_fits = n_fractional = 0
    for name in meta:
        kps = np.ascontiguousarray(z12[f"{name}_smoothed"][::3])
        F = kps.shape[0]
        rec = np.full((F, 34, 8), np.nan)
        assert emu_lib.tsnet_fit_face_curves(kps.ctypes.data, F, rec.ctypes.data) == 0
        for f in range(F):
            for e, se in enumerate(RO.sub_edges()):
                x, y = kps[f][se, 0], kps[f][se, 1]
                n_fractional += bool((x != np.floor(x)).any())
                swap = abs(x[:-1] - x[1:]).max() < abs(y[:-1] - y[1:]).max()
                if swap:
                    x, y = y, x
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    popt, _ = curve_fit(RO._linear if len(x) < 3 else RO._quadratic, x, y)
                n_fits += 1
                if len(x) == 3 and abs(popt[0]) > 1:
                    assert rec[f, e, 0] == 0
                    continue
                assert rec[f, e, 0] == 1 + 2 * swap + 4 * (len(x) == 3)
                want = [0.0, popt[0], popt[1]] if len(x) < 3 else list(popt)
                assert [float(v) for v in rec[f, e, 1:4]] == [float(v) for v in want], (name, f, e, rec[f, e], popt)      # == on doubles: bit for bit
                assert rec[f, e, 4] == min(x[0], x[-1]) and rec[f, e, 5] == max(x[0], x[-1])
    assert n_fits == 34 * (13 + 14) and n_fractional > 0.9 * n_fits


def test_a_clip_adapted_to_itself_does_not_move(emu_lib, gold):
    meta, z12, z7 = gold
    clips = {c: z7[f"{c}_keypoints"] for c in ("test114", "val024")}                     # integer landmarks
    clips.update({n: z12[f"{n}_smoothed"] for n in meta})                                  # fractional ones
    for clip, kp in clips.items():
        moved = raster.FaceAdapter(lib=emu_lib).fit(kp).apply(kp)
        assert kp.max() < 512
        d = np.abs(moved - kp).max()
        print(f"[face_crossid] {clip} adapted to itself: max shift {d:.3e}")
        assert d <= 1e-10


def _literal_moving_average(x):
    """dataset_video_face.py:357-379 on (F,P,2), evaluated with numpy's cumsum"""
    c = np.cumsum(x, axis=0)
    F = x.shape[0]
    out = np.zeros_like(x)
    out[0] = c[0]
    out[1] = c[2] / 3
    out[2] = c[4] / 5
    for i in range(3, F - 2):
        out[i] = (c[i + 2] - c[i - 3]) / 5
    out[F - 2] = (c[-1] - c[-4]) / 3
    out[F - 1] = x[-1]
    return out


@pytest.mark.parametrize("F", [5, 6, 9])
def test_smoothing_of_short_clips(emu_lib, F):
    """F = 5: no interior frame, head and tail formulas side by side; F = 6: one interior frame, (c[5] - c[0]) / 5; F = 9: several."""
    x = np.random.default_rng(F).uniform(0.0, 300.0, size=(F, 68, 2))
    got = raster.smooth_keypoints(x, lib=emu_lib)
    assert np.array_equal(got, _literal_moving_average(x))
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[-1], x[-1])
    one = raster.smooth_keypoints(x[:, :1], lib=emu_lib)                                  # P = 1: a view, made contiguous by the shell
    assert np.array_equal(one, got[:, :1])
    # in place at the C entry point
    y = np.ascontiguousarray(x.copy())
    assert emu_lib.tsnet_smooth_keypoints(y.ctypes.data, F, 68, y.ctypes.data) == 0
    assert np.array_equal(y, got)


def test_refusals(emu_lib, gold):
    meta, z12, z7 = gold
    kp = z7["val024_keypoints"]
    with pytest.raises(RuntimeError, match="five frames"):
        raster.smooth_keypoints(kp[:4], lib=emu_lib)
    out = np.full((4, 68, 2), -7.0)
    four = np.ascontiguousarray(kp[:4])
    assert emu_lib.tsnet_smooth_keypoints(four.ctypes.data, 4, 68, out.ctypes.data) == -1 and (out == -7.0).all()      # TSNET_ERR_ARG, nothing written
    ad = raster.FaceAdapter(lib=emu_lib)
    with pytest.raises(RuntimeError, match="fit"):
        ad.apply(kp)
    with pytest.raises(RuntimeError, match="fit"):
        ad.stats
    ad.fit(z7["test114_keypoints"])
    flat = kp.copy()
    flat[0, :, 0] = 100.0                                                                 # first frame without width
    with pytest.raises(RuntimeError, match="no width"):
        ad.apply(flat)
    bad = kp.copy()
    bad[3, 40, 1] = np.nan
    with pytest.raises(RuntimeError, match="non-finite"):
        ad.apply(bad)
    with pytest.raises(RuntimeError, match="non-finite"):
        raster.FaceAdapter(lib=emu_lib).fit(bad)
    stats = ad.stats
    assert emu_lib.tsnet_face_adapt_apply(stats.ctypes.data, np.ascontiguousarray(kp).ctypes.data, 0) == -1
    assert b"at least one frame" in emu_lib.tsnet_op_last_error()
    with pytest.raises(ValueError, match="68 x 2"):
        ad.apply(kp[:, :60])
    r = raster.FaceRasteriser("cpu", lib=emu_lib)
    with pytest.raises(ValueError, match="crop"):
        r.rasterise(list(z12["test114_to_val024_smoothed"][:2]), relative=True)


def test_face_driving_keypoints_from_frame_coordinates(emu_lib, gold):
    """The convenience takes what read_keypoints returns -- frame coordinates -- crops each clip by its own first frame's crop and runs the
    loader's order.  The demo clips' landmarks are integers, so cropping is exact and the points are again the reference's bits."""
    meta, z12, z7 = gold
    clips = json.loads(str(z7["meta"]))["clips"]
    for name, m in meta.items():
        sub = _frame_coords(z7[f"{m['subject']}_keypoints"], clips[m["subject"]]["crop"])
        drv = _frame_coords(z7[f"{m['driver']}_keypoints"], clips[m["driver"]]["crop"])
        pts, crop, bw = raster.face_driving_keypoints(list(sub), list(drv), lib=emu_lib)
        assert list(crop) == m["crop"] == clips[m["driver"]]["crop"] and bw == m["bw"]
        assert m["subject_crop"] == clips[m["subject"]]["crop"] == list(raster.crop_coords(sub[0]))
        assert pts.shape == (m["frames"], 68, 2) and np.array_equal(pts, z12[f"{name}_smoothed"])


def test_demo_tool_label_path_on_the_emulator(emu_lib, gold):
    """tools/demo_clip.py --drive: face_driving_keypoints -> rasterise(relative=True) -> resize_label -> vl2ch, here at F = 8 driving frames on the
    emulation build, against the same steps on the golden points."""
    import demo_clip
    from wacv23_tsnet_amd import demo
    meta, z12, z7 = gold
    m = meta["val024_to_test114"]
    sub, _ = demo_clip.clip_keypoints("val024")
    drv, dm = demo_clip.clip_keypoints("test114")
    F = 8
    r = raster.FaceRasteriser("cpu", lib=emu_lib)
    lbl, box, crop, bw = demo_clip.crossid_labels(r, sub, drv[:F])
    assert list(crop) == dm["crop"] == m["crop"] and bw == m["bw"]
    assert lbl.shape == (F, 2, 256, 256) and box.shape == (F, 256, 256)
    assert torch.equal(lbl.sum(dim=1), torch.ones_like(lbl[:, 0])) and lbl[:, 1].sum() > 1000
    # an 8-frame driving clip is smoothed over 8 frames, not 40: its own chain, step by step
    pts = raster.smooth_keypoints(raster.FaceAdapter(lib=emu_lib).fit(z7["val024_keypoints"]).apply(z7["test114_keypoints"][:F]), lib=emu_lib)
    edges, bbox, _, _ = r.rasterise(list(pts), tuple(m["crop"]), relative=True)
    assert torch.equal(lbl, r.vl2ch(demo.resize_label(edges, lib=emu_lib), 2)) and torch.equal(box, demo.resize_label(bbox, lib=emu_lib))
