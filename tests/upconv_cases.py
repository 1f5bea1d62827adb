"""The decoder's up-convolution as one operator (tsnet_op_upconv2d): nn.Upsample(x2, bilinear) + ReflectionPad2d(1) + Conv2d(3 x 3) on the
LOW-resolution map, shared by the CPU-emulation tier (test_emu_upconv.py) and the GPU tier (test_gpu_upconv.py).  kernel 0 forms the upsampled
patch while the patch kernel stages it (conv_h2.hpp UP2); kernel 1 runs upsample2x into a scratch tensor and then the convolution on the same
tile.  Every case asserts BOTH that the two routes give the same bits and that the result matches the fp64 reference."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from op_cases import _p, _rand, _sync, nchw, nhwc

# (name, N, low-res H, low-res W, Cin, Cout, tile, input transform: "in_relu" | "in" | "raw")
CASES = [
    ("a", 2, 2, 16, 16, 64, 0, "in_relu"),     # one tile touching all four borders: clamp and reflection on every side; the table per image
    ("b", 1, 4, 32, 32, 64, 0, "in_relu"),     # 2 x 2 tiles: seams in both directions, both upsample phases at a seam; two slabs
    ("c", 1, 6, 16, 48, 128, 128, "raw"),      # a tile row without an image border; odd slab count (the unroll-by-two tail); the wide tile
    ("d", 3, 2, 32, 16, 64, 0, "in"),          # batch and table per image, IN without ReLU
]


def make(case, seed=0):
    """inputs with both signs (the ReLU matters), alpha / beta distinct per image and channel; the fp64 reference"""
    _, N, H, W, Cin, Cout, _, tr = case
    x = _rand(seed, "x", (N, Cin, H, W))       # op_cases.conv_case's operands: what its tolerance was set on
    w = _rand(seed, "w", (Cout, Cin, 3, 3)) * (2.0 / (Cin * 9) ** 0.5)
    b = _rand(seed, "b", (Cout,))
    al = be = None
    xin = x
    if tr != "raw":                            # the transformed operand in fp32, as op_cases.conv_case forms it
        al = _rand(seed, "al", (N, Cin), 0.5, 1.5)
        be = _rand(seed, "be", (N, Cin), -0.3, 0.3)
        xin = x * al[:, :, None, None] + be[:, :, None, None]
        if tr == "in_relu":
            xin = F.relu(xin)
    up = F.interpolate(xin.double(), scale_factor=2, mode="bilinear", align_corners=False)
    ref = F.conv2d(F.pad(up, (1,) * 4, mode="reflect"), w.double(), b.double())
    bound = float(xin.abs().max()) * 1.0001 + 1e-30
    return x, w, b, al, be, ref, bound


def run(lib, dev, case, tensors, kernel, ksize=3, stride=1, pad=1, pad_mode=1, nprod=3, tile=None):
    """tsnet_op_upconv2d on a NaN-filled output; returns (rc, NHWC output on the CPU)"""
    _, N, H, W, Cin, Cout, ctile, tr = case
    x, w, b, al, be, _, bound = tensors
    xd, wd, bd = nhwc(x).to(dev), w.to(dev), b.to(dev)
    ald = al.contiguous().to(dev) if al is not None else None
    bed = be.contiguous().to(dev) if be is not None else None
    y = torch.full((N, 2 * H, 2 * W, Cout), float("nan"), device=dev)
    rc = lib.tsnet_op_upconv2d(xd.data_ptr(), N, H, W, Cin, wd.data_ptr(), bd.data_ptr(), Cout, ksize, stride, pad, pad_mode,
                               _p(ald), _p(bed), int(tr == "in_relu"), bound, nprod, kernel, ctile if tile is None else tile, y.data_ptr(), None)
    _sync(dev)
    return rc, y.cpu()


def check_case(lib, dev, case, rel):
    t = make(case)
    rc0, y0 = run(lib, dev, case, t, 0)
    assert rc0 == 0, lib.tsnet_op_last_error().decode()
    rc1, y1 = run(lib, dev, case, t, 1)
    assert rc1 == 0, lib.tsnet_op_last_error().decode()
    ref = t[5]
    e0 = ((nchw(y0).double() - ref).abs().max() / ref.abs().max()).item()
    e1 = ((nchw(y1).double() - ref).abs().max() / ref.abs().max()).item()
    print(f"upconv case {case[0]}: fused {e0:.3e}  two launches {e1:.3e}  equal bits {torch.equal(y0, y1)}")
    assert torch.equal(y0, y1), (case[0], (y0 - y1).abs().max().item())
    assert e0 < rel, (case[0], e0)


# what neither route takes: (keyword overrides of run) -- TSNET_ERR_ARG (-1) and an untouched output.  bf16 storage exists with bf16 operands
# (nprod = 1) alone, so the operand kind is what the operator can be asked for.
REFUSALS = [dict(pad_mode=0), dict(stride=2), dict(ksize=1, pad=0), dict(nprod=1), dict(tile=32), dict(tile=2128)]


def check_refusals(lib, dev):
    case = CASES[1]
    t = make(case)
    for kw in REFUSALS:
        for kernel in (0, 1):
            rc, y = run(lib, dev, case, t, kernel, **kw)
            assert rc == -1, (kw, kernel, rc)
            assert lib.tsnet_op_last_error()
            assert torch.isnan(y).all(), (kw, kernel)
    # a frame that does not split into 4 x 32 tiles (2W = 48)
    odd = ("odd", 1, 4, 24, 16, 64, 0, "raw")
    rc, y = run(lib, dev, odd, make(odd), 0)
    assert rc == -1 and torch.isnan(y).all()
