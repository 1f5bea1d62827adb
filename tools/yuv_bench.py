"""GPU box: frames across PCIe as YUV 4:2:0 (FrameLoader.to_yuv420 / from_yuv420, csrc/yuv_frames.hpp) against packed RGB, for

    640 x 480 and 1920 x 1080 frames at F = 1, 4 and 32

in one process, steady state, median of --reps repetitions after warm-up with the spread of the repetitions (10th and 90th percentile).
The way out -- the frames are on the device (where the paste leaves them) and wanted on the host:
  (a) today's exit: the RGB frames downloaded with .cpu(), as ClipRunner.run does, and into pinned memory, as tools/paste_bench.py does;
  (b) to_yuv420 + the download of the I420 frames into pinned memory (half the bytes);
  (c) the kernel alone between two HIP events around the C entry (the interval still holds the launch itself), with the bytes it reads plus
      writes per second, beside a device-to-device copy of the same number of bytes timed the same way: the ceiling the kernel is compared with.
The way in -- decoded frames are on the host (pinned) and wanted on the device as RGB: the RGB upload against the I420 upload + from_yuv420,
and the inverse kernel alone as in (c).
Frames are random bytes.  The device results are checked against the numpy restatement (tests/yuv_cases.py) at F = 1 before anything is
timed.  Nothing here is an acceptance gate: the figures are recorded as they come, the conversion losing included.

    python tools/yuv_bench.py > profiles/yuv_frames.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import yuv_cases as yc
from wacv23_tsnet_amd import frames

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
torch.set_num_threads(1)
dev = torch.device("cuda", 0)
ld = frames.FrameLoader(dev)
TABLE = ("bt601", True)


def spread(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[len(ts) // 10], ts[len(ts) * 9 // 10]


def timed(fn):
    for _ in range(args.warmup):
        fn()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return spread(ts)


def events(fn):
    """fn enqueues on the current stream; the time between two HIP events around it, ms"""
    for _ in range(args.warmup):
        fn()
    ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return spread([a.elapsed_time(b) for a, b in ev])


def run(h, w, F):
    rng = np.random.default_rng(F)
    rgb = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    fwd, inv = ld.yuv_tables(*TABLE)
    nb = yc.frame_bytes(h, w)
    rgb_d = torch.from_numpy(rgb).to(dev)
    yuv_d = torch.empty((F, nb), dtype=torch.uint8, device=dev)
    back_d = torch.empty_like(rgb_d)
    pin_rgb = torch.empty(rgb.shape, dtype=torch.uint8).pin_memory()
    pin_yuv = torch.empty((F, nb), dtype=torch.uint8).pin_memory()
    if F == 1:
        want = yc.rgb_to_yuv(rgb, fwd)
        assert np.array_equal(ld.to_yuv420(rgb_d, out=yuv_d).cpu().numpy(), want)
        assert np.array_equal(ld.from_yuv420(yuv_d, (h, w), out=back_d).cpu().numpy(), yc.yuv_to_rgb(want, h, w, inv))

    def out_rgb_cpu():
        rgb_d.cpu()

    def out_rgb_pinned():
        pin_rgb.copy_(rgb_d, non_blocking=True)
        torch.cuda.synchronize()

    def out_yuv():
        ld.to_yuv420(rgb_d, out=yuv_d)
        pin_yuv.copy_(yuv_d, non_blocking=True)
        torch.cuda.synchronize()

    def in_rgb():
        back_d.copy_(pin_rgb, non_blocking=True)
        torch.cuda.synchronize()

    def in_yuv():
        yuv_d.copy_(pin_yuv, non_blocking=True)
        ld.from_yuv420(yuv_d, (h, w), out=back_d)
        torch.cuda.synchronize()

    t_cpu, t_pin, t_yuv = timed(out_rgb_cpu), timed(out_rgb_pinned), timed(out_yuv)
    t_in_rgb, t_in_yuv = timed(in_rgb), timed(in_yuv)
    s = torch.cuda.current_stream(dev).cuda_stream
    moved = F * (3 * h * w + nb)                                      # either direction reads one form and writes the other
    k_fwd = events(lambda: ld.lib.tsnet_rgb_to_yuv420(rgb_d.data_ptr(), F, h, w, fwd.ctypes.data, 0, yuv_d.data_ptr(), s))
    k_inv = events(lambda: ld.lib.tsnet_yuv420_to_rgb(yuv_d.data_ptr(), F, h, w, inv.ctypes.data, 0, back_d.data_ptr(), s))
    a, b = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    k_copy = events(lambda: b.copy_(a))                               # reads moved / 2 bytes and writes as many
    per = lambda t: [round(v / F, 4) for v in t]
    us = lambda t: [round(v * 1e3, 1) for v in t]
    gbs = lambda t: round(moved / t[0] / 1e6, 1)
    print(json.dumps({
        "frame": f"{w}x{h}", "F": F, "rgb_MB": round(rgb.nbytes / 1e6, 2), "i420_MB": round(F * nb / 1e6, 2),
        "out_rgb_cpu_ms_per_frame_median_p10_p90": per(t_cpu), "out_rgb_pinned_ms_per_frame_median_p10_p90": per(t_pin),
        "out_to_yuv420_plus_i420_pinned_ms_per_frame_median_p10_p90": per(t_yuv),
        "out_yuv_over_rgb_pinned": round(t_yuv[0] / t_pin[0], 3), "out_yuv_over_rgb_cpu": round(t_yuv[0] / t_cpu[0], 3),
        "out_expected_half_rgb_pinned_plus_kernel_ms_per_frame": round((t_pin[0] / 2 + k_fwd[0]) / F, 4),
        "in_rgb_pinned_upload_ms_per_frame_median_p10_p90": per(t_in_rgb), "in_i420_upload_plus_from_yuv420_ms_per_frame_median_p10_p90": per(t_in_yuv),
        "in_yuv_over_rgb": round(t_in_yuv[0] / t_in_rgb[0], 3),
        "kernel_to_yuv_us_median_p10_p90": us(k_fwd), "kernel_to_rgb_us_median_p10_p90": us(k_inv), "copy_same_bytes_us_median_p10_p90": us(k_copy),
        "kernel_MB_read_plus_written": round(moved / 1e6, 3), "kernel_to_yuv_GB_per_s": gbs(k_fwd), "kernel_to_rgb_GB_per_s": gbs(k_inv),
        "copy_GB_per_s": gbs(k_copy), "to_yuv_over_copy_rate": round(k_copy[0] / k_fwd[0], 3), "to_rgb_over_copy_rate": round(k_copy[0] / k_inv[0], 3)}), flush=True)


print(f"# yuv_bench: torch threads 1, reps {args.reps} (median, 10th and 90th percentile), warm-up {args.warmup}; {torch.cuda.get_device_name(0)}; "
      f"table {TABLE[0]} {'full' if TABLE[1] else 'limited'} range, I420")
print("# out: RGB frames on the device -> host: .cpu() | pinned copy | to_yuv420 + pinned copy of the I420 frames.  in: pinned host frames -> RGB on the "
      "device: RGB upload | I420 upload + from_yuv420.  kernels and a device-to-device copy of the same bytes by HIP events around the call")
for F in (1, 4, 32):
    for h, w in ((480, 640), (1080, 1920)):
        run(h, w, F)
