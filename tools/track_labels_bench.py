"""GPU box: the face labels of a clip with a crop per frame -- FaceRasteriser.clip_labels(crop=(F,4), compact=True), one call of
tsnet_face_labels_boxes_u8 -- against what the previous commit did for the same input, at 256 x 256 and F = 1, 4 and 32, for two inputs:

    val024    the clip's own per-frame crops (268 .. 274 pixels), key points and crops repeated cyclically to F
    distinct  F distinct sizes: val024's first frame scaled by 1 + 0.015 f per frame (274 .. 400 pixels at F = 32)

in one process, steady state, median of --reps repetitions after warm-up with the 10th and 90th percentile beside it.  A repetition starts from
host key points and ends with a synchronisation:
  (a) the single call;
  (b) the previous commit's clip_labels on the same input, restated here (`groups_clip_labels`: the frames of every crop size through
      tsnet_raster_face and tsnet_resize_label, twice, and back into frame order) on the library given with --lib2 -- a build of the previous
      commit; without --lib2 this tree's library, whose single-size entries are the same code;
  (c) the fixed-crop clip_labels at the same F (one crop for the clip, the first frame's): the floor.
The host's curve fits (tsnet_fit_face_curves), which every side pays, are timed alone as well.  The outputs of (a) and (b) are checked equal before
anything is timed.  Nothing here is an acceptance gate.

    python tools/track_labels_bench.py [--lib2 path/to/the/previous/libtsnet_hip.so] > profiles/track_labels.txt
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import demo_clip
from wacv23_tsnet_amd import _lib, raster
from wacv23_tsnet_amd.demo import resize_label

ap = argparse.ArgumentParser()
ap.add_argument("--lib2", default=None)
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
args = ap.parse_args()
torch.set_num_threads(1)
dev = torch.device("cuda", 0)
lib = _lib.load()
lib2 = _lib.bind(C.CDLL(os.path.abspath(args.lib2))) if args.lib2 else lib
SIZE = (256, 256)


def groups_clip_labels(rs, kp, crops):
    """the previous commit's FaceRasteriser.clip_labels(crop=(F,4), compact=True)"""
    edges, bbox, crops, _ = rs.rasterise(kp, crops)
    cls = torch.empty((len(edges),) + SIZE, dtype=torch.float32, device=rs.device)
    box = torch.empty_like(cls)
    for idx in rs._size_groups(crops).values():
        cls[idx] = resize_label(torch.stack([edges[f] for f in idx]), SIZE, lib=rs.lib)
        box[idx] = resize_label(torch.stack([bbox[f] for f in idx]), SIZE, lib=rs.lib)
    return cls.to(torch.uint8), box.to(torch.uint8)


def spread(ts):
    ts = sorted(ts)
    return [round(v, 4) for v in (statistics.median(ts), ts[len(ts) // 10], ts[len(ts) * 9 // 10])]


def timed(fn, sync=True):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def run(name, kp, crops):
    F = len(kp)
    kps = list(kp)
    rs, rs2 = raster.FaceRasteriser(dev), raster.FaceRasteriser(dev, lib=lib2)
    fixed = tuple(int(v) for v in crops[0])
    a = lambda: rs.clip_labels(kps, SIZE, crop=crops, compact=True)
    b = lambda: groups_clip_labels(rs2, kps, crops)
    c = lambda: rs.clip_labels(kps, SIZE, crop=fixed, compact=True)
    la, ba, _ = a()
    lb, bb = b()
    assert torch.equal(la, lb) and torch.equal(ba, bb) and int(la.sum()) > 0
    rel = np.ascontiguousarray(kp - crops[:, None, [2, 0]], dtype=np.float64)
    curves = np.empty((F, 34, 8))
    fits = timed(lambda: lib.tsnet_fit_face_curves(rel.ctypes.data, F, curves.ctypes.data), sync=False)
    ta, tb, tc = timed(a), timed(b), timed(c)
    sizes = sorted({(int(r[1] - r[0]), int(r[3] - r[2])) for r in crops})
    print(json.dumps({"case": name, "F": F, "size_groups": len(sizes), "crop_heights": [min(s[0] for s in sizes), max(s[0] for s in sizes)],
                      "a_single_call_ms_median_p10_p90": ta, "b_previous_groups_ms_median_p10_p90": tb, "c_fixed_crop_ms_median_p10_p90": tc,
                      "host_fits_ms_median_p10_p90": fits, "b_over_a": round(tb[0] / ta[0], 2), "a_over_c": round(ta[0] / tc[0], 3),
                      "a_minus_b_ms": round(ta[0] - tb[0], 4), "b_spread_p90_minus_p10_ms": round(tb[2] - tb[1], 4)}), flush=True)


print(f"# track_labels_bench: torch threads 1, reps {args.reps} (median, 10th and 90th percentile), warm-up {args.warmup}; {torch.cuda.get_device_name(0)}")
print(f"# a = clip_labels(crop=(F,4), compact=True), one call of tsnet_face_labels_boxes_u8 (at most six kernels, four when no frame takes a Gaussian pass); "
      f"b = the previous commit's size-group loop on {'the library ' + os.path.basename(args.lib2) if args.lib2 else 'this library (no --lib2)'}; "
      "c = the fixed-crop clip_labels; wall clock from host key points to the end of a synchronisation, fits and uploads included, ms per CALL")
val = demo_clip.clip_keypoints("val024")[0]
for F in (1, 4, 32):
    kp = val[np.arange(F) % len(val)]
    run("val024's own crops", kp, raster.crop_coords_clip(kp))
    kp = np.stack([np.round((val[0] - val[0].mean(0)) * (1.0 + 0.015 * f) + val[0].mean(0)) for f in range(F)])
    crops = raster.crop_coords_clip(kp)
    assert len({(int(r[1] - r[0]), int(r[3] - r[2])) for r in crops}) == F, "the scaled frames do not have F distinct sizes"
    run("F distinct sizes", kp, crops)
