"""GPU box: a box per frame (FrameLoader.prepare / paste with (F,4) boxes; tsnet_prepare_frames_boxes_u8, tsnet_paste_frames_boxes) against what a
caller could do without it, for the two real shapes of paste_bench.py:

    face  640 x 480 frame <-> 256 x 256, boxes = val024's per-frame crops (268 .. 274 pixels), repeated cyclically to F
    pose  1920 x 1080 frame <-> the 128 x 256 picture of a 256 x 256 square, the fixed box (841, 206, 1231, 986) moved by the same offsets

each at F = 1, 4 and 32, for the prepare (byte form) and for the paste, in one process, steady state, median of --reps repetitions after warm-up
with the 10th and 90th percentile beside it.  Everything starts and stays on the device; a repetition ends with a synchronisation:
  (a) one call with a box per frame -- descriptor upload included;
  (b) a loop of F single-box calls with the same boxes: what a caller had before;
  (c) one single-box call at the same F with one fixed box: the floor -- what the per-frame indirection and the launch-wide tile height cost.
The outputs of (a) and (b) are checked equal before anything is timed.  Nothing here is an acceptance gate.

    python tools/track_crop_bench.py > profiles/track_crop.txt
"""
import argparse
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
from wacv23_tsnet_amd import frames, raster

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
torch.set_num_threads(1)
dev = torch.device("cuda", 0)
ld = frames.FrameLoader(dev)

crops = raster.crop_coords_clip(demo_clip.clip_keypoints("val024")[0])
FACE = crops[:, [2, 0, 3, 1]]                                        # (x0, y0, x1, y1)
POSE = np.array((841, 206, 1231, 986)) + (FACE - FACE[0])


def spread(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[len(ts) // 10], ts[len(ts) * 9 // 10]


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def kernel_alone(op, video, gen, boxes, fixed, size, square, src_box):
    """the C entries of (a) and (c) between two HIP events, their arguments laid out once: the interval holds the launch and the kernel, not the
    loader's Python nor the descriptor upload -> (a, c) in microseconds, median with 10th / 90th percentile"""
    lib, stream = ld.lib, torch.cuda.current_stream(dev).cuda_stream
    F, h, w, _ = video.shape
    ow, oh = size
    S = max(ow, oh)
    OH, OW = (S, S) if square else (oh, ow)
    geom = (oh, ow, (OH - oh) // 2, (OW - ow) // 2, OH, OW)
    x0, y0, x1, y1 = fixed
    tab = lambda n_in, n_out: (lambda t, taps: (t.data_ptr(), t.data_ptr() + 4 * n_out, t.data_ptr() + 8 * n_out, taps))(*ld._axis(n_in, n_out))
    if op == "prepare":
        out = torch.empty((F, 3, OH, OW), dtype=torch.uint8, device=dev)
        d, dd, pool, _ = ld._descriptors(np.asarray(boxes, np.int64), lambda b: ((b[2] - b[0], ow), (b[3] - b[1], oh)))
        call_a = lambda: lib.tsnet_prepare_frames_boxes_u8(video.data_ptr(), F, h, w, d.ctypes.data, dd.data_ptr(), pool.data_ptr(), pool.numel(), *geom, out.data_ptr(), stream)
        call_c = lambda: lib.tsnet_prepare_frames_u8(video.data_ptr(), F, h, w, x0, y0, x1, y1, *tab(x1 - x0, ow), *tab(y1 - y0, oh), *geom, out.data_ptr(), stream)
    else:
        sx0, sy0, sx1, sy1 = src_box if src_box is not None else (0, 0, 256, 256)
        d, dd, pool, _ = ld._descriptors(np.asarray(boxes, np.int64), lambda b: ((sx1 - sx0, b[2] - b[0]), (sy1 - sy0, b[3] - b[1])))
        call_a = lambda: lib.tsnet_paste_frames_boxes(gen.data_ptr(), None, F, 256, 256, sx0, sy0, sx1, sy1, d.ctypes.data, dd.data_ptr(), pool.data_ptr(), pool.numel(),
                                                      video.data_ptr(), h, w, stream)
        call_c = lambda: lib.tsnet_paste_frames(gen.data_ptr(), None, F, 256, 256, sx0, sy0, sx1, sy1, *tab(sx1 - sx0, x1 - x0), *tab(sy1 - sy0, y1 - y0),
                                                video.data_ptr(), h, w, x0, y0, x1, y1, stream)
    res = []
    for call in (call_a, call_c):
        for _ in range(args.warmup):
            assert call() == 0
        ev = []
        for _ in range(args.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); call(); e.record()
            ev.append((s, e))
        torch.cuda.synchronize()
        res.append(spread([s.elapsed_time(e) * 1e3 for s, e in ev]))
    return res


def run(name, hw, size, square, src_box, track, F):
    h, w = hw
    rng = np.random.default_rng(F)
    boxes = track[np.arange(F) % len(track)]
    video = torch.from_numpy(rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)).to(dev)
    gen = torch.from_numpy(rng.integers(0, 256, (F, 256, 256, 3), dtype=np.uint8)).to(dev)
    fixed = tuple(int(v) for v in boxes[0])
    rows = [tuple(int(v) for v in b) for b in boxes]
    ops = {
        "prepare": (lambda: ld.prepare(video, boxes, size, square=square, as_bytes=True),
                    lambda: [ld.prepare(video[f:f + 1], rows[f], size, square=square, as_bytes=True) for f in range(F)],
                    lambda: ld.prepare(video, fixed, size, square=square, as_bytes=True)),
        "paste": (lambda: ld.paste(gen, video, boxes, src_box=src_box, inplace=True),
                  lambda: [ld.paste(gen[f:f + 1], video[f:f + 1], rows[f], src_box=src_box, inplace=True) for f in range(F)],
                  lambda: ld.paste(gen, video, fixed, src_box=src_box, inplace=True)),
    }
    for op, (a, b, c) in ops.items():
        if op == "prepare":
            assert torch.equal(a(), torch.cat(b()))
        else:
            keep = video.clone()
            got = a().clone(); video.copy_(keep); b()
            assert torch.equal(got, video) and not torch.equal(got, keep)
        ta, tb, tc = timed(a), timed(b), timed(c)
        ka, kc = kernel_alone(op, video, gen, boxes, fixed, size, square, src_box)
        r = lambda t: [round(v / F, 4) for v in t]
        print(json.dumps({"case": name, "op": op, "F": F, "sizes": sorted({int(x[2] - x[0]) for x in boxes}),
                          "a_boxes_ms_per_frame_median_p10_p90": r(ta), "b_loop_ms_per_frame_median_p10_p90": r(tb), "c_fixed_ms_per_frame_median_p10_p90": r(tc),
                          "a_over_c": round(ta[0] / tc[0], 3), "b_over_a": round(tb[0] / ta[0], 2),
                          "a_minus_c_us_per_call": round((ta[0] - tc[0]) * 1e3, 1),
                          "kernel_alone_a_us_median_p10_p90": [round(v, 1) for v in ka], "kernel_alone_c_us_median_p10_p90": [round(v, 1) for v in kc]}), flush=True)


print(f"# track_crop_bench: torch threads 1, reps {args.reps} (median, 10th and 90th percentile), warm-up {args.warmup}; {torch.cuda.get_device_name(0)}")
print("# a = one call with a box per frame (descriptor upload included); b = a loop of F single-box calls; c = one single-box call with a fixed box; "
      "wall clock of enqueue + synchronisation, everything on the device")
for F in (1, 4, 32):
    run("face 640x480 <-> 256x256, val024's crops", (480, 640), (256, 256), False, None, FACE, F)
    run("pose 1920x1080 <-> 128x256 of 256x256, the pose box moved by val024's offsets", (1080, 1920), (128, 256), True, (64, 0, 192, 256), POSE, F)
