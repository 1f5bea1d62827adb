"""Record conv_w1's output BITS on the cases of tests/w1_pair_cases.py with the CPU-emulation build of the tree this is run in:
    python tools/probes/w1_capture_bits.py          (writes tests/golden/w1_parent_bits.npz and, to keep every file under 1 MiB, .part2.npz ...)
Run at the commit BEFORE a change to the producers (the lane mapping, the item shape, the LDS pads), the file is what
tests/test_emu_w1_pair_lanes.py holds the changed kernel to, value for value: the transform, the split and the product order are meant to be
untouched by such a change, and the emulator runs the kernel sources as they are.  Our own kernels' outputs, fp32 NHWC."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conftest                      # noqa: E402  (tests/conftest.py: the emulation build)
import op_cases as oc                # noqa: E402
import w1_pair_cases as wc           # noqa: E402
from wacv23_tsnet_amd import _lib    # noqa: E402


def main():
    lib = _lib.bind(ctypes.CDLL(conftest.build_emu_lib()))
    rec = {}
    for name, args, kw, chunks, _ in wc.CASES:
        ys = wc.outputs(oc, lib, "cpu", name, args, kw, chunks)
        y = ys[chunks[0]]
        assert all(torch.equal(y, o) for o in ys.values()), (name, "chunk sizes differ in this tree")
        rec[name] = y.numpy()
        print(f"{name:24s} chunks {chunks}  {tuple(y.shape)}  max|y| {float(y.abs().max()):.4g}")
    parts, size = [{}], 0                # greedy, in case order: a part is closed before it would pass the limit (fp32 noise barely compresses)
    for name, y in rec.items():
        if parts[-1] and size + y.nbytes > wc.LIMIT:
            parts.append({}); size = 0
        parts[-1][name] = y; size += y.nbytes
    for i, p in enumerate(parts):
        np.savez_compressed(wc.part_path(i), **p)
        print(f"{wc.part_path(i)}: {sorted(p)}  {os.path.getsize(wc.part_path(i))} bytes")


if __name__ == "__main__":
    main()
