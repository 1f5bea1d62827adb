"""GPU box: the frame loader (wacv23_tsnet_amd/frames.py, csrc/frames.hpp) against the reference's host path, for the two real shapes:

    face  640 x 480 frame, 244 x 244 crop -> 256 x 256
    pose  1920 x 1080 frame, 390 x 780 crop -> 128 x 256, padded to 256 x 256

each at F = 1 and F = 32, steady state, median of --reps repetitions after warm-up:
  (a) the reference's way on this host, single thread: Image.crop().resize(), channel reversal, - IMG_MEAN, upload of the fp32 tensor;
  (b) this build: upload of the uint8 crop rows (the rows of the frame the box covers) + the kernel; and the kernel alone between two HIP
      events, with the bytes it reads (the crop's pixels) and writes (the fp32 planes) per second.
Frames are random bytes.  The outputs of (a) and (b) are checked equal before anything is timed.

    python tools/frames_bench.py > profiles/frames_prepare.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from wacv23_tsnet_amd import demo, frames

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
assert args.reps >= 50
torch.set_num_threads(1)
dev = torch.device("cuda", 0)
ld = frames.FrameLoader(dev)
MEAN = demo.IMG_MEAN


def reference(fr, box, size, square):
    """the loaders' statements per frame, then one upload of the fp32 batch"""
    out = []
    for f in fr:
        im = Image.fromarray(f).crop(box).resize(size)
        a = np.asarray(im)
        if square:
            S = max(size)
            full = np.zeros((S, S, 3), np.uint8)
            full[(S - size[1]) // 2:(S - size[1]) // 2 + size[1], (S - size[0]) // 2:(S - size[0]) // 2 + size[0]] = a
            a = full
        out.append((a[:, :, ::-1].astype(np.float32) - MEAN).transpose(2, 0, 1))
    t = torch.from_numpy(np.ascontiguousarray(np.stack(out))).to(dev)
    torch.cuda.synchronize()
    return t


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def run(name, hw, box, size, square, F):
    h, w = hw
    x0, y0, x1, y1 = box
    rng = np.random.default_rng(F)
    fr = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    rows = np.ascontiguousarray(fr[:, y0:y1])                        # what has to cross PCIe: the frame rows the box covers, contiguous
    rbox = (x0, 0, x1, y1 - y0)
    assert torch.equal(ld.prepare(rows, rbox, size, square=square), reference(fr, box, size, square))

    def ours():
        ld.prepare(torch.from_numpy(rows), rbox, size, square=square)
        torch.cuda.synchronize()

    t_ref = median_ms(lambda: reference(fr, box, size, square), args.reps, args.warmup)
    t_ours = median_ms(ours, args.reps, args.warmup)
    rows_d = torch.from_numpy(rows).to(dev)
    for _ in range(args.warmup):
        ld.prepare(rows_d, rbox, size, square=square)
    ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); ld.prepare(rows_d, rbox, size, square=square); b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    t_k = statistics.median(a.elapsed_time(b) for a, b in ev)
    S = max(size)
    OH, OW = (S, S) if square else (size[1], size[0])
    nbytes = F * ((y1 - y0) * (x1 - x0) * 3 + 3 * OH * OW * 4)
    print(json.dumps({"case": name, "F": F, "reference_host_ms_per_frame": round(t_ref / F, 4), "upload_u8_plus_kernel_ms_per_frame": round(t_ours / F, 4),
                      "speedup_incl_upload": round(t_ref / t_ours, 2), "kernel_alone_us": round(t_k * 1e3, 1), "kernel_alone_us_per_frame": round(t_k * 1e3 / F, 2),
                      "kernel_MB_read_plus_written": round(nbytes / 1e6, 2), "kernel_GB_per_s": round(nbytes / t_k / 1e6, 1),
                      "uploaded_MB_u8": round(rows.nbytes / 1e6, 2), "reference_uploaded_MB_fp32": round(F * 3 * OH * OW * 4 / 1e6, 2)}), flush=True)
    return t_ref / t_ours


print(f"# frames_bench: Pillow {Image.__version__}, torch threads 1, reps {args.reps} (median), warm-up {args.warmup}; {torch.cuda.get_device_name(0)}")
ok = True
for F in (1, 32):
    r1 = run("face 640x480, crop 244x244 -> 256x256", (480, 640), (121, 17, 365, 261), (256, 256), False, F)
    r2 = run("pose 1920x1080, crop 390x780 -> 128x256 + bars", (1080, 1920), (841, 206, 1231, 986), (128, 256), True, F)
    if F == 32:
        ok = r1 > 1.0 and r2 > 1.0
print(f"# acceptance (upload + kernel faster than the reference's host path per frame at F = 32, both shapes): {'PASS' if ok else 'FAIL'}")
sys.exit(0 if ok else 1)
