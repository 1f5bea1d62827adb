"""GPU box: feathered paste masks on the device (FrameLoader.feather_mask, csrc/mask_blur.hpp) against the host path they replace, r = 8, at
256 x 256 and 512 x 512, F = 1, 4 and 32, in one process, steady state, median of --reps repetitions after warm-up with the spread of the
repetitions (10th and 90th percentile) beside it.  The 0 / 1 bbox masks start on the device (where the rasteriser leaves them) and the feathered
mask is wanted on the device (where the paste reads it):
  (a) the host path, single thread: download the masks, per frame Image.filter(ImageFilter.GaussianBlur(r)), upload from pinned memory;
  (b) the device call: the C entry on the masks in place (flags bit 0) + a synchronisation, by the host clock;
  (c) the same call between two HIP events (the interval holds the two launches themselves);
  (d) the box-mask form (in = NULL: the indicator of a rectangle, nothing read) between two HIP events, beside (c).
The outputs of (a), (b) and (d) are checked equal to Pillow before anything is timed.  Nothing here is an acceptance gate: the figures are
recorded as they come.

    python tools/feather_bench.py > profiles/feather_mask.txt
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageFilter

from wacv23_tsnet_amd import frames

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--radius", type=float, default=8.0)
args = ap.parse_args()
torch.set_num_threads(1)
dev = torch.device("cuda", 0)
ld = frames.FrameLoader(dev)
R = args.radius


def spread(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[len(ts) // 10], ts[len(ts) * 9 // 10]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def events(fn, reps, warmup):
    for _ in range(warmup):
        assert fn() == 0
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return spread([a.elapsed_time(b) for a, b in ev])


def run(S, F):
    rng = np.random.default_rng(F + S)
    m = np.zeros((F, S, S), np.uint8)                                       # a 0 / 1 box per frame, as the rasteriser's bbox masks are
    for f in range(F):
        x0, y0 = rng.integers(S // 8, S // 3, 2)
        m[f, y0:y0 + S // 2, x0:x0 + S // 2] = 1
    m_d = torch.from_numpy(m).to(dev)
    pinned = torch.empty(m.shape, dtype=torch.uint8).pin_memory()
    out_h = torch.empty_like(m_d)

    def host_path():
        a = m_d.cpu().numpy()
        p = pinned.numpy()
        for f in range(F):
            p[f] = np.asarray(Image.fromarray(a[f] * 255, "L").filter(ImageFilter.GaussianBlur(R)))
        out_h.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize()

    host_path()
    want = out_h.clone()
    assert torch.equal(ld.feather_mask(m_d, R, binary=True), want)
    inset = ld.feather_inset(R)
    rect = (inset, inset, S - inset, S - inset)
    ref = np.zeros((S, S), np.uint8); ref[rect[1]:rect[3], rect[0]:rect[2]] = 255
    box_want = torch.from_numpy(np.asarray(Image.fromarray(ref, "L").filter(ImageFilter.GaussianBlur(R)))).to(dev)
    box_got = ld.feather_mask(None, R, size=(F, S, S), rect=rect)
    assert all(torch.equal(box_got[f], box_want) for f in range(F))
    out, tmp = torch.empty_like(m_d), torch.empty_like(m_d)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rect_c = (C.c_int * 4)(*rect)
    call_in = lambda: ld.lib.tsnet_blur_mask(m_d.data_ptr(), F, S, S, None, R, R, 1, out.data_ptr(), tmp.data_ptr(), stream)
    call_box = lambda: ld.lib.tsnet_blur_mask(None, F, S, S, rect_c, R, R, 0, out.data_ptr(), tmp.data_ptr(), stream)

    def device_call():
        call_in()
        torch.cuda.synchronize()

    t_host = timed(host_path, args.reps, args.warmup)
    t_dev = timed(device_call, args.reps, args.warmup)
    assert torch.equal(out, want)
    t_in = events(call_in, args.reps, args.warmup)
    t_box = events(call_box, args.reps, args.warmup)
    assert all(torch.equal(out[f], box_want) for f in range(F))
    r4 = lambda t, d=1.0: [round(v / d, 4) for v in t]
    us = lambda t, d=1.0: [round(v * 1e3 / d, 2) for v in t]
    print(json.dumps({"size": f"{S}x{S}", "F": F, "radius": R, "host_ms_per_frame_median_p10_p90": r4(t_host, F),
                      "device_call_sync_ms_per_frame_median_p10_p90": r4(t_dev, F), "device_over_host_speedup": round(t_host[0] / t_dev[0], 2),
                      "device_events_us_median_p10_p90": us(t_in), "device_events_us_per_frame": round(t_in[0] * 1e3 / F, 2),
                      "box_form_events_us_median_p10_p90": us(t_box), "box_form_events_us_per_frame": round(t_box[0] * 1e3 / F, 2),
                      "MB_read_plus_written_input_form": round(4 * m.size / 1e6, 3)}), flush=True)


print(f"# feather_bench: Pillow {Image.__version__}, torch threads 1, radius {R}, reps {args.reps} (median, 10th and 90th percentile), warm-up {args.warmup}; "
      f"{torch.cuda.get_device_name(0)}")
print("# host = download of the 0/1 masks + Image.filter(GaussianBlur) per frame + upload from pinned memory; device = tsnet_blur_mask (rows kernel, "
      "columns kernel) + synchronise by the host clock, and between HIP events; box form = in NULL, the indicator of a rectangle")
for S in (256, 512):
    for F in (1, 4, 32):
        run(S, F)
