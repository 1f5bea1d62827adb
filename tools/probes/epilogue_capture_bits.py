"""Record the convolutions' epilogue BITS on the cases of tests/epilogue_bits_cases.py:
    python tools/probes/epilogue_capture_bits.py                       the CPU-emulation build of the tree this is run in
                                                                       -> tests/golden/epilogue_parent_bits.npz, .part2.npz ... each under 1 MiB
    python tools/probes/epilogue_capture_bits.py --gpu LIB [--out DIR] LIB = a libtsnet_hip.so (the parent commit's, built in a checkout of its own),
                                                                       on an MI355X -> epilogue_parent_bits_gpu.npz ... in tests/golden or DIR
Run with the code of the commit BEFORE a change to conv_epilogue's index arithmetic or to a patch tile's staging, the files are what
tests/test_emu_epilogue_parent_bits.py and its GPU twin hold the changed kernels to, word for word: y, the fp64 statistics partials, alpha, beta
and amax_out through tsnet_op_conv2d_epi.  The emulator runs the kernel sources as they are; the device's MFMA sums a k-step in an order of
its own, so the GPU tier needs the second record.  Our own kernels' outputs."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import conftest                      # noqa: E402  (tests/conftest.py: the emulation build)
import epilogue_bits_cases as bc     # noqa: E402
from wacv23_tsnet_amd import _lib    # noqa: E402


def main():
    gpu = "--gpu" in sys.argv
    if gpu:
        import torch
        assert torch.cuda.is_available()
        lib, dev = _lib.bind(ctypes.CDLL(os.path.abspath(sys.argv[sys.argv.index("--gpu") + 1]))), "cuda"
    else:
        lib, dev = _lib.bind(ctypes.CDLL(conftest.build_emu_lib())), "cpu"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.dirname(bc.GOLDEN)
    os.makedirs(out, exist_ok=True)
    parts, size = [{}], 0                # greedy, in case order: a part is closed before it would pass the limit (fp32 noise barely compresses)
    for case in bc.CASES:
        w = {f"{case[0]}/{k}": v.numpy() for k, v in bc.words(lib, dev, case).items()}
        n = sum(v.nbytes for v in w.values())
        print(f"{case[0]:28s} {case[1]:6s} info {w[case[0] + '/info'].tolist()}  {sorted(k.split('/')[1] for k in w)}  {n} bytes")
        if parts[-1] and size + n > bc.LIMIT:
            parts.append({}); size = 0
        parts[-1].update(w); size += n
    for i, p in enumerate(parts):
        path = os.path.join(out, os.path.basename(bc.part_path(i, gpu)))
        np.savez_compressed(path, **p)
        print(f"{path}: {len(p)} arrays  {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
