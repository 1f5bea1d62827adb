"""Cases of the RGB head's folded MFMA form (csrc/head_mfma.hpp), shared by the CPU-emulation tier (tests/test_emu_head_mfma.py) and the GPU
tier (tests/test_gpu_head_mfma.py).  tsnet_op_head takes the folded kernel when C % 16 == 0 and the InstanceNorm transform is present, so
every case here passes (alpha, beta).  References are plain PyTorch CPU ops (fp32, and fp64 for the error comparison)."""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F

import op_cases as oc

# the smallest legal frame, odd heights, widths not divisible by 4, frames narrower than a tile, tiles hanging over both edges, a full-width row of tiles
SHAPES = [(1, 4, 4), (3, 6, 5), (1, 9, 7), (2, 10, 12), (1, 40, 36), (2, 32, 256)]
RAGGED = SHAPES[:5]
ONE_HOT = [(0, 0, 0, 0), (1, 5, 6, 6), (2, 15, 3, 3), (0, 7, 0, 6), (1, 9, 6, 0)]
BG = [0.25, -0.5, 0.75]


def inputs(N, H, W, C, seed=0):
    """x, alpha, beta, w, bias as op_cases.head_case draws them"""
    x = oc._rand(seed, "x", (N, C, H, W))
    w = oc._rand(seed, "w", (3, C, 7, 7)) * (2.0 / (C * 49) ** 0.5)
    b = oc._rand(seed, "b", (3,))
    al = oc._rand(seed, "al", (N, C), 0.5, 1.5)
    be = oc._rand(seed, "be", (N, C), -0.3, 0.3)
    return x, al, be, w, b


def activation(x, al, be):
    return F.relu(x * al[:, :, None, None] + be[:, :, None, None])


def run(lib, dev, x, al, be, w, b, composite=False, rows=0):
    """tsnet_op_head on relu(x * alpha + beta): (N, 3, H, W) on the CPU"""
    N, C, H, W = x.shape
    y = torch.full((N, 3, H, W), float("nan"), device=dev)
    xd, wd, bd = oc.nhwc(x).to(dev), w.contiguous().to(dev), b.to(dev)
    ald, bed = al.contiguous().to(dev), be.contiguous().to(dev)
    rc = lib.tsnet_op_head(xd.data_ptr(), N, H, W, C, ald.data_ptr(), bed.data_ptr(), wd.data_ptr(), bd.data_ptr(), int(composite) | (rows << 8),
                           (ctypes.c_float * 3)(*BG), y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    oc._sync(dev)
    return y.cpu()


def rows_give_equal_bits(lib, dev, N, H, W, C=64):
    x, al, be, w, b = inputs(N, H, W, C)
    ys = [run(lib, dev, x, al, be, w, b, rows=r) for r in (8, 16, 32, 0)]
    return all(torch.equal(ys[0], y) for y in ys[1:]) and bool(torch.isfinite(ys[0]).all())


def batch_gives_equal_bits(lib, dev, H, W, C=64):
    """image i of an N = 4 call against the N = 1 call on that image"""
    x, al, be, w, b = inputs(4, H, W, C)
    y4 = run(lib, dev, x, al, be, w, b)
    return all(torch.equal(y4[i:i + 1], run(lib, dev, x[i:i + 1], al[i:i + 1], be[i:i + 1], w, b)) for i in range(4))


def one_hot_case(lib, dev, H, W, o, c, ky, kx, C=16):
    """a filter with a single 1: output channel o is tanh(activation of channel c shifted by (ky - 3, kx - 3), reflected, + bias[o]), the other
    two are tanh(bias).  Returns max|d|."""
    x, al, be, _, b = inputs(1, H, W, C)
    w = torch.zeros(3, C, 7, 7)
    w[o, c, ky, kx] = 1.0
    xp = F.pad(activation(x, al, be), (3,) * 4, mode="reflect")
    ref = torch.tanh(b)[None, :, None, None].expand(1, 3, H, W).clone()
    ref[0, o] = torch.tanh(xp[0, c, ky:ky + H, kx:kx + W] + b[o])
    return (run(lib, dev, x, al, be, w, b) - ref).abs().max().item()


def fp64_errors(lib, dev, N, H, W, C):
    """(max error of the folded head, max error of PyTorch's fp32 CPU evaluation), both against the fp64 evaluation"""
    x, al, be, w, b = inputs(N, H, W, C)
    xin = activation(x, al, be)
    ref64 = torch.tanh(F.conv2d(F.pad(xin.double(), (3,) * 4, mode="reflect"), w.double(), b.double()))
    ref32 = torch.tanh(F.conv2d(F.pad(xin, (3,) * 4, mode="reflect"), w, b))
    y = run(lib, dev, x, al, be, w, b)
    return (y.double() - ref64).abs().max().item(), (ref32.double() - ref64).abs().max().item()
