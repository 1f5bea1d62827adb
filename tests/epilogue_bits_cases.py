"""The cases that pin conv_epilogue's index arithmetic (csrc/conv_common.hpp: the row map once per row group, 32-bit output offsets, the addend's
image taken per tile) to the BITS of the commit before it: shared by tools/probes/epilogue_capture_bits.py (which recorded
tests/golden/epilogue_parent_bits*.npz with that commit's emulation build and epilogue_parent_bits_gpu*.npz with its device library on an
MI355X), the CPU tier (tests/test_emu_epilogue_parent_bits.py) and the GPU tier (tests/test_gpu_epilogue_parent_bits.py).  The values, their order of summation and the stores are meant to be untouched by such a change, so
every word -- y, the fp64 partials, alpha, beta, amax_out -- is held with torch.equal.

One case = (name, family, shape of epilogue_cases, kernel, tile, nprod, options).  Options: stats (0 / 1 = in_finalize2 launch / 2 = the plan's
route, with the arrival counters), amax (amax_out), add_nmod (an addend of add_nmod images), in_pair (the operand scale from a published max |x|,
epilogue_cases.AMAX_PAIRS), bound (a fixed operand bound).  The smallest shapes at which a rewritten index map can go wrong:
  rows past the end of an image (m = -1): the row-tile families at 156 = 128 + 28 and 80 = 64 + 16 positions;
  Cout below the tile width and no multiple of 32 (nok false on whole lanes): 16, 24, 40, 72 and 96 channels;
  the addend with add_nmod < N and = N; two or three images, so that the tile -> image map matters;
  one tile per image, 2 - 32 (in-kernel finalize) and 33 (in_finalize2 route: a patch and a row-tile family); amax_out on and off;
  conv_w1 with chunks of two tiles at one tile per image (every chunk crosses into the next image);
  the stem at its own geometry: a 4 x 32 and an 8 x 64 frame of 8 channels, 7 x 7, reflection, with a derived and a fixed scale."""
import os

import epilogue_cases as ec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epilogue_parent_bits.npz")
# The device's MFMA sums a k-step in an order of its own, so the emulator's y is not the MI355X's (nor was it for the commit before): the GPU
# tier has a record of its own, the same cases through the parent commit's libtsnet_hip.so on the device.
GOLDEN_GPU = GOLDEN.replace(".npz", "_gpu.npz")
LIMIT = 900 * 1024           # a committed file stays under 1 MiB: the record is written in parts (.npz, .part2.npz, ...)

R, Z, NORM, RAW = ec.REFL, ec.ZERO, ec.NORM, ec.RAW
# shapes: (N, H, W, Cin, Cout, k, stride, pad, reflect, norm)
_H2_40 = (2, 8, 32, 16, 40, 3, 1, 1, R, NORM)            # two 4 x 32 tiles per image
_H2_72 = (2, 8, 32, 16, 72, 3, 1, 1, R, NORM)
_H2_KG = (2, 8, 32, 32, 40, 3, 1, 1, R, NORM)           # two K groups need an even number of 16-channel slabs
_H2_16 = (2, 4, 32, 16, 16, 3, 1, 1, R, NORM)            # one tile per image, Cout below every tile width
_H2_33 = (1, 132, 32, 16, 16, 3, 1, 1, R, NORM)          # 33 tiles per image: in_finalize2
_H2D = (2, 8, 64, 16, 72, 3, 2, 1, Z, NORM)
_H2D_3 = (3, 16, 64, 16, 72, 3, 2, 1, Z, NORM)           # 8 x 32 outputs: two four-row / four two-row tiles per image
_H2S = (2, 8, 32, 8, 64, 7, 1, 3, R, RAW)
_STEM_A = (2, 4, 32, 8, 64, 7, 1, 3, R, RAW)             # one tile per image: the 3-pixel reflection reaches past the 4-row frame's middle
_STEM_B = (2, 8, 64, 8, 64, 7, 1, 3, R, RAW)             # 2 x 2 tiles per image
_H2S32 = (2, 8, 32, 32, 40, 7, 1, 3, R, RAW)
_H2R_C = (2, 12, 13, 16, 24, 1, 1, 0, Z, NORM)           # 156 positions: 128 + 28 (64-row tile: 64 + 64 + 28)
_H2R_B = (2, 9, 7, 64, 130, 3, 2, 1, Z, NORM)            # 20 positions per image in one ragged tile
_G64_B = (2, 8, 10, 64, 130, 1, 1, 0, Z, NORM)           # 80 positions: 64 + 16
_H2R_33 = (1, 65, 64, 16, 16, 1, 1, 0, Z, NORM)          # 4160 positions = 32 tiles of 128 rows and one of 64: in_finalize2
_W1_16 = (16, 4, 32, 128, 40, 3, 1, 1, R, NORM)          # one tile per image, sixteen in all (eight XCD rows of two): every chunk of two crosses an image
_W1_2 = (2, 8, 32, 128, 40, 3, 1, 1, R, NORM)


def _c(name, family, shape, kernel, tile, nprod, **opt):
    return (name, family, shape, kernel, tile, nprod, opt)


CASES = (
    _c("h2_32_nmod1", "H2", _H2_40, 2, 32, 3, stats=2, amax=True, add_nmod=1),
    _c("h2_64_nmod2", "H2", _H2_72, 2, 64, 3, stats=2, amax=True, add_nmod=2),
    _c("h2_128_launch_noamax", "H2", _H2_72, 2, 128, 3, stats=1),
    _c("h2_2128_plain", "H2", _H2_72, 2, 2128, 3),
    _c("h2_20064", "H2", _H2_KG, 2, 20064, 3, stats=2, amax=True),
    _c("h2_3128_bf16", "H2", _H2_72, 2, 3128, 1, stats=2, amax=True, add_nmod=1),
    _c("h2_one_tile_cout16", "H2", _H2_16, 2, 32, 3, stats=2, amax=True, add_nmod=2),
    _c("h2_33_tiles", "H2", _H2_33, 2, 32, 3, stats=2, amax=True),
    _c("h2d_2128_nmod1", "H2D", _H2D, 2, 2128, 3, stats=2, amax=True, add_nmod=1),
    _c("h2d_64_nmod3", "H2D", _H2D_3, 2, 64, 3, stats=2, amax=True, add_nmod=3),
    _c("h2d_128_noamax", "H2D", _H2D_3, 2, 128, 3, stats=2),
    _c("h2d_12128", "H2D", _H2D, 2, 12128, 3, stats=2, amax=True),
    _c("h2s_nmod2", "H2S", _H2S, 0, 0, 3, stats=2, amax=True, add_nmod=2),
    _c("h2s_nmod1_noamax", "H2S", _H2S, 0, 0, 3, stats=1, add_nmod=1),
    _c("stem_4x32_fixed", "H2S", _STEM_A, 0, 0, 3, stats=2, amax=True),
    _c("stem_4x32_in_amax", "H2S", _STEM_A, 0, 0, 3, stats=2, amax=True, in_pair="binades"),
    _c("stem_4x32_in_amax_edge", "H2S", _STEM_A, 0, 0, 3, stats=2, amax=True, in_pair="edge"),
    _c("stem_4x32_bound300", "H2S", _STEM_A, 0, 0, 3, bound=300.0),
    _c("stem_8x64_fixed", "H2S", _STEM_B, 0, 0, 3, stats=2, amax=True, add_nmod=1),
    _c("stem_8x64_in_amax", "H2S", _STEM_B, 0, 0, 3, stats=2, amax=True, in_pair="binades"),
    _c("stem_4x32_in_amax_f16", "H2S", _STEM_A, 0, 0, 16, stats=2, amax=True, in_pair="binades"),
    _c("stem_4x32_bf16", "H2S", _STEM_A, 0, 0, 1, stats=2, amax=True),
    _c("h2s32_nmod1", "H2S32", _H2S32, 0, 0, 3, stats=2, amax=True, add_nmod=1),
    _c("h2s32_nmod2_noamax", "H2S32", _H2S32, 0, 0, 3, stats=1, add_nmod=2),
    _c("h2r_64_ragged_nmod2", "H2R", _H2R_C, 1, 64, 3, stats=2, amax=True, add_nmod=2),
    _c("h2r_s2_128_nmod1", "H2R", _H2R_B, 1, 128, 3, stats=2, amax=True, add_nmod=1),
    _c("h2r_64_launch_noamax", "H2R", _H2R_C, 1, 64, 3, stats=1, add_nmod=1),
    _c("g64_3064_ragged_nmod2", "G64", _G64_B, 1, 3064, 3, stats=2, amax=True, add_nmod=2),
    _c("g64_3128_ragged_nmod1", "G64", _G64_B, 1, 3128, 3, stats=2, amax=True, add_nmod=1),
    _c("g64_3064_bf16_noamax", "G64", _G64_B, 1, 3064, 1, stats=2),
    _c("h2r_33_tiles", "H2R", _H2R_33, 1, 64, 3, stats=2, amax=True),
    _c("w1_chunk2_nmod4", "W1", _W1_16, 3, 2, 3, stats=2, amax=True, add_nmod=4),
    _c("w1_chunk2_nmod1_noamax", "W1", _W1_16, 3, 2, 3, stats=1, add_nmod=1),
    _c("w1_chunk1", "W1", _W1_2, 3, 1, 3, stats=2, amax=True, add_nmod=2),
)
NAMES = [c[0] for c in CASES]


def part_path(i, gpu=False):
    base = GOLDEN_GPU if gpu else GOLDEN
    return base if i == 0 else base.replace(".npz", f".part{i + 1}.npz")


def load_golden(gpu=False):
    """{case name/word: array} from every part of the record (gpu: the one taken on the device)"""
    import numpy as np
    rec, i = {}, 0
    while os.path.exists(part_path(i, gpu)):
        with np.load(part_path(i, gpu)) as z:
            rec.update({k: z[k] for k in z.files})
        i += 1
    return rec


def words(lib, dev, case):
    """{word: integer tensor of its bits} of one case: y, and where the case asks for them part (the plan's N x tpi x Cout x 2 doubles), alpha, beta,
    amax.  Plus info: (family index, tiles per image, finalize route, chunk, rows, width) -- the plan the record was taken on."""
    import torch
    name, family, shape, kernel, tile, nprod, opt = case
    t = ec.inputs(shape)
    N = shape[0]
    Ho, Wo = ec.shape_out(shape)
    kw = dict(stats=opt.get("stats", 0), amax=opt.get("amax", False))
    if kw["stats"] == 2:
        kw["counters"] = True
    if "add_nmod" in opt:
        kw["addend"] = ec._rand(11, "addend", (opt["add_nmod"], Ho, Wo, shape[4]), -2.0, 2.0)
    if "bound" in opt:
        kw["bound"] = opt["bound"]
    if "in_pair" in opt:                                   # epilogue_cases.check_in_amax's inputs: every image its own maximum, published exactly
        x = t["x"].clone()
        for i in range(N):
            m = ec.AMAX_PAIRS[opt["in_pair"]][i % 2]
            x[i] *= 0.7 * m / float(x[i].abs().max())
            x[i, 1, 2, 3] = -m
        kw.update(x=x, in_amax=x.abs().amax(dim=(1, 2, 3)).view(torch.int32), bound=0.0)
    o = ec.run(lib, dev, shape, kernel, tile, nprod, t, **kw)
    assert o.rc == 0, (name, o.msg)
    assert o.family == family, (name, "the planner runs this case on", o.family, o.info)
    if family == "W1":
        assert o.chunk == tile, (name, o.chunk)
    out = {"y": o.y.view(torch.int32), "info": torch.tensor([o.info[0], o.tpi, o.fin, o.chunk, o.rows, o.width], dtype=torch.int32)}
    assert not torch.isnan(o.y).any(), (name, "an output word was never written")
    if kw["stats"]:
        assert o.fin == int(kw["stats"] == 2 and o.tpi <= ec.FIN_MAX_TILES), (name, o.tpi, o.fin)
        out["part"] = o.part.contiguous().view(torch.int64)
        out["alpha"], out["beta"] = o.alpha.view(torch.int32), o.beta.view(torch.int32)
        if kw["stats"] == 2:
            assert o.nonzero == 0, (name, "arrival counters left non-zero")
    if kw["amax"]:
        out["amax"] = o.amax
    return out


def check_case(lib, dev, case, golden):
    """every word of the case equals the record; returns the words compared"""
    import torch
    got = words(lib, dev, case)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.split("/", 1)[0] == case[0])
    assert keys == sorted(got), (case[0], keys, sorted(got))
    for k in keys:
        want = torch.from_numpy(golden[f"{case[0]}/{k}"])
        assert want.dtype == got[k].dtype and want.shape == got[k].shape, (case[0], k, want.shape, got[k].shape)
        bad = int((want != got[k]).sum())
        assert torch.equal(want, got[k]), (case[0], k, f"{bad} of {want.numel()} words differ from the parent's")
    return keys
