"""Record the output BITS of every case of tests/one_table_cases.py with the CPU-emulation build of the tree this is run in:
    python tools/probes/one_table_capture_bits.py     (writes tests/golden/one_table_parent_bits.npz, in parts if it would pass 1 MiB)
Run at the commit BEFORE a change to how the kernels of the transformation and synthesis branches find a source image (the slot table,
the mask layout, the operator entry points' spellings), the file is what tests/test_one_table.py holds the changed tree to, value for value:
such a change moves addresses, not arithmetic, and the emulator runs the kernel sources as they are.  Our own kernels' outputs, fp32."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conftest                      # noqa: E402  (tests/conftest.py: the emulation build)
import one_table_cases as tc         # noqa: E402
from wacv23_tsnet_amd import _lib    # noqa: E402


def main():
    lib = _lib.bind(ctypes.CDLL(conftest.build_emu_lib()))
    rec = {"forward." + k: v for k, v in tc.forward_outputs(lib).items()}
    rec.update({"op." + k: v for k, v in tc.op_outputs(lib).items()})
    parts, size = [{}], 0                # greedy, in case order: a part is closed before it would pass the limit
    for name, t in rec.items():
        y = t.contiguous().numpy()
        assert np.isfinite(y).all(), name
        if parts[-1] and size + y.nbytes > tc.LIMIT:
            parts.append({}); size = 0
        parts[-1][name] = y; size += y.nbytes
        print(f"{name:36s} {tuple(y.shape)}  max|y| {float(np.abs(y).max()):.4g}")
    for i, p in enumerate(parts):
        np.savez_compressed(tc.part_path(i), **p)
        print(f"{tc.part_path(i)}: {len(p)} arrays, {os.path.getsize(tc.part_path(i))} bytes")


if __name__ == "__main__":
    main()
