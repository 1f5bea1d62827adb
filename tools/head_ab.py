"""GPU box: the RGB head alone (tsnet_op_head at the forward's shape, 64 channels, 256 x 256, batch 4 and 1) with every tile height and the
launcher's choice, on this tree's library and on another build of the same ABI (--lib2, e.g. the previous commit's).  The operator call
allocates and packs, so the kernel's own time comes from a kernel trace around this script:
    rocprofv3 --kernel-trace -f csv -d OUT -o t -- python tools/head_ab.py --lib2 PATH
    python tools/head_ab.py --summarise OUT/.../t_kernel_trace.csv"""
import argparse, collections, csv, ctypes, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib2", default=None)
ap.add_argument("--summarise", default=None, metavar="CSV")
a = ap.parse_args()
if a.summarise:
    agg = collections.OrderedDict()
    for r in csv.DictReader(open(a.summarise)):
        n = r["Kernel_Name"]
        if "head_" not in n or "pack" in n:
            continue
        k = (re.sub(r"\(.*", "", n).replace("void tsnet::", ""), r.get("Grid_Size_Y", ""))
        agg.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, v in agg.items():
        v = sorted(v)
        print("%-28s batch=%-3s n=%2d  median %7.1f us  min %7.1f" % (k[0], k[1], len(v), v[len(v) // 2], v[0]))
    sys.exit(0)
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: F401
from wacv23_tsnet_amd import _lib
import head_mfma_cases as hc
libs = {"this tree": _lib.load()}
if a.lib2:
    libs[os.path.basename(a.lib2)] = _lib.bind(ctypes.CDLL(a.lib2))
for N in (4, 1):
    x, al, be, w, b = hc.inputs(N, 256, 256, 64)
    for name, lib in libs.items():
        for rows in (8, 16, 32, 0):
            for _ in range(3):
                hc.run(lib, "cuda", x, al, be, w, b, rows=rows)
print("done")
