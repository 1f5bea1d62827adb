"""The convolutions' shared epilogue and operand hand-offs one kernel at a time (tsnet_op_conv2d_epi; csrc/conv_common.hpp conv_epilogue), shared by
the CPU-emulation tier (test_emu_conv_epilogue.py) and the GPU tier (test_gpu_conv_epilogue.py).

What a whole forward cannot show at 1e-3 on a stage output is held here word by word: the addend of a split convolution, every fp64 statistics
partial, alpha / beta on both finalize routes (the in_finalize2 launch, and the last-arriving workgroup behind the arrival counters), max |y| per
image, the operand scale derived on the device from a published max |x|, and bf16 storage of x and y.  Every yardstick is the RETURNED y: the
convolution sum itself is test_emu_ops.py's / test_gpu_ops.py's business, and with any epilogue part switched on y must keep the bits
tsnet_op_conv2d gives on the same kernel and tile.

Bounds (none of them measured from the code under test):
  partial (tile t, channel c): |sum - ref| <= n * 2^-52 * sum|v|, |sumsq - ref| <= n * 2^-52 * sum v^2, n = positions of the tile -- the worst case
      of ANY fp64 summation order of n exactly representable terms ((n - 1) * 2^-53 to first order; v^2 of an fp32 v is exact in fp64).
  alpha: 2^-21 relative; beta: 2^-21 |beta_ref| + 2^-40 alpha_ref max|y| -- conv_epilogue's write_ab rounds to fp32 five or six times at <= 2^-24
      each ((float)var, + eps, sqrt, divide, (float)mean, the product: 6 * 2^-24 < 2^-21); the absolute term covers the fp64 summation error of a
      mean near zero.
  everything else is bit equality."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from op_cases import _p, _rand, _sync, bf16_tie_values, nhwc
from wacv23_tsnet_amd._lib import CONV_EPI_INFO, TsnetConvEpi

TSNET_ERR_ARG = -1
FAMILIES = ("H2R", "G64", "H2", "H2S", "H2S32", "H2D", "W1")          # csrc/conv_plan.hpp ConvFamily, in its order
PATCH = ("H2", "H2S", "H2S32", "H2D", "W1")                           # tiles are rows x 32 pixel rectangles, row-major inside an image
FIN_COUNTER_INTS = 65536                                              # conv_plan.hpp kFinCounterInts
FIN_MAX_TILES = 32                                                    # conv_plan.hpp kFinMaxTiles
REFL, ZERO, NORM, RAW = 1, 0, True, False

# shapes: (N, H, W, Cin, Cout, k, stride, pad, reflect, norm)
_H2 = (2, 8, 32, 32, 130, 3, 1, 1, REFL, NORM)          # two 4 x 32 tiles per image; 130 channels: a ragged last channel tile at every width
_H2D = (2, 8, 64, 16, 72, 3, 2, 1, ZERO, NORM)
_H2S = (2, 8, 32, 8, 64, 7, 1, 3, REFL, RAW)
_H2S32 = (2, 8, 32, 32, 40, 7, 1, 3, REFL, RAW)
_H2R_A = (2, 5, 7, 16, 24, 1, 1, 0, ZERO, NORM)         # 35 positions in one tile
_H2R_B = (1, 9, 7, 64, 130, 3, 2, 1, ZERO, NORM)        # 20 positions, three channel tiles of 64 / two of 128 with a ragged last one
_H2R_C = (2, 12, 13, 16, 24, 1, 1, 0, ZERO, NORM)       # 156 positions: a whole 128-row tile and a ragged one of 28 per image
_G64_A = (2, 8, 8, 64, 130, 1, 1, 0, ZERO, NORM)
_G64_B = (2, 8, 10, 64, 130, 1, 1, 0, ZERO, NORM)       # 80 positions: 64 + 16 in the 64-row tile, one ragged 128-row tile
_W1_12 = (12, 8, 32, 128, 96, 3, 1, 1, REFL, NORM)      # two tiles per image: a chunk of three crosses into the next image
_W1_8 = (8, 8, 32, 128, 96, 3, 1, 1, REFL, NORM)


def _tpi_shape(H):
    return (2, H, 32, 16, 64, 3, 1, 1, REFL, NORM)


# rows: name -> (family, shape, kernel, tile, nprod[, expected (w1_chunk, w1_tab2)])
ROWS = {}
for _t in (32, 64, 128, 2128, 20032, 20064):
    ROWS[f"h2_{_t}"] = ("H2", _H2, 2, _t, 3)
ROWS["h2_3128_bf16"] = ("H2", _H2, 2, 3128, 1)
ROWS["h2_64_f16"] = ("H2", _H2, 2, 64, 16)
for _t in (64, 128, 2128, 12128):
    ROWS[f"h2d_{_t}"] = ("H2D", _H2D, 2, _t, 3)
ROWS["h2s"] = ("H2S", _H2S, 0, 0, 3)
ROWS["h2s32"] = ("H2S32", _H2S32, 0, 0, 3)
ROWS["h2r_1x1_64"] = ("H2R", _H2R_A, 1, 64, 3)
ROWS["h2r_s2_128"] = ("H2R", _H2R_B, 1, 128, 3)
ROWS["h2r_two_tiles_64"] = ("H2R", _H2R_C, 1, 64, 3)
ROWS["g64_3064"] = ("G64", _G64_A, 1, 3064, 3)
ROWS["g64_3128"] = ("G64", _G64_A, 1, 3128, 3)
ROWS["g64_ragged_3064"] = ("G64", _G64_B, 1, 3064, 3)
ROWS["g64_ragged_3128"] = ("G64", _G64_B, 1, 3128, 3)
ROWS["w1_chunk1"] = ("W1", _W1_12, 3, 1, 3, (1, 0))
ROWS["w1_chunk3"] = ("W1", _W1_12, 3, 3, 3, (3, 1))
ROWS["w1_chunk2"] = ("W1", _W1_8, 3, 2, 3, (2, 1))
# tiles per image on H2 at 16 -> 64, W = 32: the fold's eight-entry batches with a ragged tail, the kFinMaxTiles boundary, the fall-back to the launch
TPI_ROWS = {1: 4, 7: 28, 8: 32, 9: 36, 32: 128, 33: 132}              # tpi -> H
for _tpi, _h in TPI_ROWS.items():
    ROWS[f"h2_tpi{_tpi}"] = ("H2", _tpi_shape(_h), 2, 64, 3)
# bf16 operands (nprod = 1): the rows of the bf16-storage checks
ROWS["h2r_1x1_64_bf16"] = ("H2R", _H2R_A, 1, 64, 1)
ROWS["g64_ragged_3064_bf16"] = ("G64", _G64_B, 1, 3064, 1)
ROWS["h2d_2128_bf16"] = ("H2D", _H2D, 2, 2128, 1)

STAT_ROWS = [r for r in ROWS]
BF16_ROWS = ["h2_3128_bf16", "h2r_1x1_64_bf16", "g64_ragged_3064_bf16", "h2d_2128_bf16"]
# (row, add_nmod): 1 and N / 2 (rows of two images have both in one)
ADDEND_CASES = [("h2_64", 1), ("h2_20032", 1), ("h2d_2128", 1), ("h2s", 1), ("h2s32", 1), ("h2r_two_tiles_64", 1), ("g64_ragged_3064", 1),
                ("w1_chunk3", 1), ("w1_chunk3", 6), ("w1_chunk2", 4)]
# (row, nprod): the operand scale from a published maximum; conv_w1 has no fp16-operand form
IN_AMAX_CASES = [("h2_64", 3), ("h2_64", 16), ("h2d_2128", 3), ("h2d_2128", 16), ("h2r_1x1_64", 3), ("h2r_1x1_64", 16),
                 ("g64_ragged_3064", 3), ("g64_ragged_3064", 16), ("w1_chunk3", 3), ("h2s", 3), ("h2s", 16)]
_ULP = 2.0 ** -24
AMAX_PAIRS = {"binades": (0.9, 300.0),                                # maxima far apart: every image needs its own scale
              "edge": (0.75 - _ULP, 0.75)}                            # + 0.25: 1 - 2^-24 and 1.0 -- one ulp either side of a power of two
BOUND_ADD = 0.25


def shape_out(shape):
    N, H, W, Cin, Cout, k, stride, pad, reflect, norm = shape
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


_INPUTS = {}


def inputs(shape, seed=0, ties=False):
    """op_cases.conv_case's operands: x in (-1, 1), He-scaled weights, a bias in (-1, 1) (channel means away from zero), per-image alpha / beta
    where the layer has a fused transform (then with ReLU).  ties: a quarter of x from bf16_tie_values, and the first output channels read ONE
    operand through a centre tap of 1.5 without bias -- 1.5 times a bf16 value with an odd significand below 171 / 128 is an exact bf16 tie."""
    key = (shape, seed, ties)
    if key not in _INPUTS:
        N, H, W, Cin, Cout, k, stride, pad, reflect, norm = shape
        x = _rand(seed, "x", (N, Cin, H, W))
        w = _rand(seed, "w", (Cout, Cin, k, k)) * (2.0 / (Cin * k * k) ** 0.5)
        b = _rand(seed, "b", (Cout,))
        if ties:
            t = bf16_tie_values(seed, "xt", (N, Cin, H, W), emin=-2, emax=1)
            x = torch.where(_rand(seed, "xm", (N, Cin, H, W), 0.0, 1.0) < 0.25, t, x)
            nd = min(Cin, Cout) // 2
            w[:nd] = 0.0
            for c in range(nd):
                w[c, c, k // 2, k // 2] = 1.5
            b[:nd] = 0.0
        al = _rand(seed, "al", (N, Cin), 0.5, 1.5) if norm else None
        be = _rand(seed, "be", (N, Cin), -0.3, 0.3) if norm else None
        xin = x if not norm else F.relu(x * al[:, :, None, None] + be[:, :, None, None])
        _INPUTS[key] = dict(x=nhwc(x), w=w, b=b, al=al, be=be, bound=float(xin.abs().max()) * 1.0001 + 1e-30)
    return _INPUTS[key]


def bf16_bits(t):
    """round to nearest even to bf16: the 16-bit patterns"""
    return t.float().to(torch.bfloat16).view(torch.int16)


class Out:
    pass


def run(lib, dev, shape, kernel, tile, nprod, t, *, plain=False, stats=0, counters=False, repeat=1, amax=False, addend=None, in_amax=None,
        x_bf16=False, y_bf16=False, x=None, al=None, be=None, bound=None, part_short=0, null_alpha=False, add_nmod=None):
    """One call on NaN-filled outputs.  plain: tsnet_op_conv2d (the yardstick of y's bits); else tsnet_op_conv2d_epi.  The scratch is sized
    from the shape alone, for the smallest tile a plan can take (64 positions), so that no plan can outgrow it."""
    N, H, W, Cin, Cout, k, stride, pad, reflect, norm = shape
    Ho, Wo = shape_out(shape)
    x = t["x"] if x is None else x
    al = t["al"] if al is None else al
    be = t["be"] if be is None else be
    N = x.shape[0]
    xd = (x.to(torch.bfloat16) if x_bf16 else x).contiguous().to(dev)
    wd, bd = t["w"].to(dev), t["b"].to(dev)
    ald = al.contiguous().to(dev) if norm else None
    bed = be.contiguous().to(dev) if norm else None
    y = torch.full((N, Ho, Wo, Cout), float("nan"), device=dev, dtype=torch.bfloat16 if y_bf16 else torch.float32)
    args = [xd.data_ptr(), N, H, W, Cin, wd.data_ptr(), bd.data_ptr(), Cout, k, stride, pad, int(reflect), _p(ald), _p(bed), int(bool(norm)),
            t["bound"] if bound is None else bound, nprod, kernel, tile, y.data_ptr()]
    o = Out()
    if plain:
        o.rc = lib.tsnet_op_conv2d(*args, None)
        o.msg = lib.tsnet_op_last_error().decode() if o.rc else ""
        _sync(dev)
        o.y = y.cpu()
        return o
    e = TsnetConvEpi()
    e.stats, e.repeat = stats, repeat
    info = (C.c_int * CONV_EPI_INFO)(*([-1] * CONV_EPI_INFO))
    nz = C.c_int(-1)
    e.info_out = C.cast(info, C.POINTER(C.c_int))
    keep = []
    if stats:
        cap = N * ((Ho * Wo + 63) // 64) * Cout * 2
        part = torch.zeros(cap, dtype=torch.float64, device=dev)
        alpha = torch.full((N, Cout), float("nan"), device=dev)
        beta = torch.full((N, Cout), float("nan"), device=dev)
        e.part, e.part_capacity = part.data_ptr(), cap
        e.alpha, e.beta = (None if null_alpha else alpha.data_ptr()), beta.data_ptr()
    if counters:
        cnt = torch.zeros(FIN_COUNTER_INTS, dtype=torch.int32, device=dev)
        e.counters = cnt.data_ptr()
        e.counters_nonzero_out = C.pointer(nz)
    if amax:
        am = torch.full((N,), -1, dtype=torch.int32, device=dev)          # the op zeroes it
        e.amax_out = am.data_ptr()
    if addend is not None:
        ad = addend.contiguous().to(dev)
        keep.append(ad)
        e.addend, e.add_nmod = ad.data_ptr(), addend.shape[0] if add_nmod is None else add_nmod
    if in_amax is not None:
        ia = in_amax.contiguous().to(dev)
        keep.append(ia)
        e.in_amax, e.bound_add = ia.data_ptr(), BOUND_ADD
    e.x_bf16, e.y_bf16 = int(x_bf16), int(y_bf16)
    if part_short:                                                        # the plan's need is known from a first call: one double short of it
        e.part_capacity = part_short
    o.rc = lib.tsnet_op_conv2d_epi(*args, C.byref(e), None)
    o.msg = lib.tsnet_op_last_error().decode() if o.rc else ""
    _sync(dev)
    o.y = y.cpu()
    o.info = list(info)
    o.family = FAMILIES[info[0]] if 0 <= info[0] < len(FAMILIES) else None
    o.tpi, o.fin, o.chunk, o.tab2, o.rows, o.width, o.tiles_n = info[1:8]
    if stats:
        o.part_all = part.cpu()
        o.part = o.part_all[:N * max(o.tpi, 0) * Cout * 2].view(N, max(o.tpi, 0), Cout, 2) if o.rc == 0 else None
        o.alpha, o.beta = alpha.cpu(), beta.cpu()
    if counters:
        o.nonzero = nz.value
    if amax:
        o.amax = am.cpu()
    return o


def _ok(o):
    assert o.rc == 0, o.msg
    return o


_PLAIN = {}


def plain_y(lib, dev, name):
    """tsnet_op_conv2d's output of a row, computed once per library"""
    key = (id(lib), name)
    if key not in _PLAIN:
        family, shape, kernel, tile, nprod = ROWS[name][:5]
        _PLAIN[key] = _ok(run(lib, dev, shape, kernel, tile, nprod, inputs(shape), plain=True)).y
    return _PLAIN[key]


def tile_sums(y, o):
    """fp64 (sum, sum of squares, sum of |v|, positions) of the returned y per (image, tile, channel), by the plan's tile map"""
    N, Ho, Wo, Cc = y.shape
    v = y.double()
    if o.family in PATCH:
        assert Ho % o.rows == 0 and Wo % 32 == 0 and o.tpi == (Ho // o.rows) * (Wo // 32), (o.family, o.info)
        g = v.view(N, Ho // o.rows, o.rows, Wo // 32, 32, Cc)
        red = lambda u: u.sum(dim=(2, 4)).reshape(N, o.tpi, Cc)
        n = torch.full((o.tpi,), o.rows * 32.0, dtype=torch.float64)
    else:
        hw = Ho * Wo
        assert o.tpi == (hw + o.rows - 1) // o.rows, (o.family, o.info)
        g = F.pad(v.view(N, hw, Cc), (0, 0, 0, o.tpi * o.rows - hw)).view(N, o.tpi, o.rows, Cc)
        red = lambda u: u.sum(dim=2)
        n = torch.tensor([min(o.rows, hw - i * o.rows) for i in range(o.tpi)], dtype=torch.float64)
    return red(g), red(g * g), red(g.abs()), n[None, :, None]


def check_partials(y, o):
    """every double finite and within the reassociation bound of the returned y's tile; returns the worst error as a fraction of its bound"""
    assert torch.isfinite(o.part).all(), "a partial was never written (NaN-primed) or is not finite"
    s, q, a, n = tile_sums(y, o)
    bs, bq = n * 2.0 ** -52 * a, n * 2.0 ** -52 * q
    es, eq = (o.part[..., 0] - s).abs(), (o.part[..., 1] - q).abs()
    assert (es <= bs).all() and (eq <= bq).all(), ("partials", (es - bs).max().item(), (eq - bq).max().item(),
                                                    torch.nonzero((es > bs) | (eq > bq))[:8].tolist())
    tiny = 1e-300
    return max((es / (bs + tiny)).max().item(), (eq / (bq + tiny)).max().item())


def ab_ref(y):
    """alpha_ref = 1 / sqrt(var + 1e-5), beta_ref = -mean alpha_ref (biased variance) in fp64 from the returned y, and max |y| per image"""
    N, Ho, Wo, Cc = y.shape
    v = y.double().view(N, Ho * Wo, Cc)
    mean = v.mean(dim=1)
    var = ((v - mean[:, None, :]) ** 2).mean(dim=1)
    al = 1.0 / torch.sqrt(var + 1e-5)
    return al, -mean * al, v.abs().amax(dim=(1, 2))


def check_ab(y, o):
    """every word of alpha / beta within the derived bound; returns the worst alpha and beta errors in units of 2^-24 of the reference"""
    al, be, ymax = ab_ref(y)
    ea, eb = (o.alpha.double() - al).abs(), (o.beta.double() - be).abs()
    ba = 2.0 ** -21 * al
    bb = 2.0 ** -21 * be.abs() + 2.0 ** -40 * al * ymax[:, None]
    assert torch.isfinite(o.alpha).all() and torch.isfinite(o.beta).all(), "alpha / beta not written, or folded from a NaN-primed partial"
    assert (ea <= ba).all(), ("alpha", (ea / al).max().item() / 2.0 ** -24, torch.nonzero(ea > ba)[:8].tolist())
    assert (eb <= bb).all(), ("beta", ((eb - bb).max().item()), torch.nonzero(eb > bb)[:8].tolist())
    return (ea / al).max().item() / 2.0 ** -24, (eb / (be.abs() + 2.0 ** -19 * al * ymax[:, None])).max().item() / 2.0 ** -24


def check_amax(y, o):
    """word img = the float bits of max |y[img]| over the real channels and positions, exactly"""
    want = y.abs().amax(dim=(1, 2, 3)).view(torch.int32)
    assert torch.equal(o.amax, want), ("amax_out", o.amax.tolist(), want.tolist())


def check_plan(name, o):
    row = ROWS[name]
    assert o.family == row[0], (name, "the planner runs this row on", o.family, o.info)
    if row[0] == "W1":
        assert (o.chunk, o.tab2) == row[5], (name, o.chunk, o.tab2)
    if name.startswith("h2_tpi"):
        assert o.tpi == int(name[6:]), (name, o.tpi)


def report(name, o, **kw):
    route = "in-kernel" if o.fin else "launch"
    print(f"epilogue {name}: family {o.family} tile {o.rows}x{o.width} tpi {o.tpi} finalize {route} chunk {o.chunk} tab2 {o.tab2} "
          + " ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in kw.items()))


def check_stats(lib, dev, name):
    """One row: y keeps tsnet_op_conv2d's bits with the statistics, the counters and amax_out on; every partial, alpha / beta on both routes
    (stats = 2 three launches back to back on NaN-primed partials, stats = 1 once), amax_out, the counters left zero, the route the plan took."""
    family, shape, kernel, tile, nprod = ROWS[name][:5]
    t = inputs(shape)
    y0 = plain_y(lib, dev, name)
    o2 = _ok(run(lib, dev, shape, kernel, tile, nprod, t, stats=2, counters=True, repeat=3, amax=True))
    check_plan(name, o2)
    assert o2.fin == int(o2.tpi <= FIN_MAX_TILES), (name, o2.tpi, o2.fin)
    assert torch.equal(o2.y.view(torch.int32), y0.view(torch.int32)), (name, "y changed by the epilogue's extras", (o2.y - y0).abs().max().item())
    p2 = check_partials(o2.y, o2)
    a2, b2 = check_ab(o2.y, o2)
    check_amax(o2.y, o2)
    assert o2.nonzero == 0, (name, "arrival counters left non-zero", o2.nonzero)
    o1 = _ok(run(lib, dev, shape, kernel, tile, nprod, t, stats=1))
    assert o1.fin == 0 and o1.tpi == o2.tpi
    assert torch.equal(o1.y.view(torch.int32), y0.view(torch.int32)), (name, "y changed by the statistics")
    p1 = check_partials(o1.y, o1)
    a1, b1 = check_ab(o1.y, o1)
    report(name, o2, partial_err_over_bound=max(p1, p2), alpha_err_ulp24=max(a1, a2), beta_err_ulp24=max(b1, b2))


def check_all_families_occur():
    assert {r[0] for r in ROWS.values()} == set(FAMILIES)


def check_addend(lib, dev, name, add_nmod):
    """y_with == fl32(y_without + addend[img % add_nmod]) bit for bit (one fp32 addition); statistics and amax taken from y_with"""
    family, shape, kernel, tile, nprod = ROWS[name][:5]
    N, Cout = shape[0], shape[4]
    Ho, Wo = shape_out(shape)
    assert N % add_nmod == 0
    t = inputs(shape)
    y0 = plain_y(lib, dev, name)
    add = _rand(7, "addend", (add_nmod, Ho, Wo, Cout), -2.0, 2.0)
    o = _ok(run(lib, dev, shape, kernel, tile, nprod, t, stats=2, counters=True, amax=True, addend=add))
    check_plan(name, o)
    want = y0 + add.repeat(N // add_nmod, 1, 1, 1)                     # image n reads addend[n % add_nmod]
    assert torch.equal(o.y.view(torch.int32), want.view(torch.int32)), (name, add_nmod, (o.y - want).abs().max().item())
    p = check_partials(o.y, o)
    a, b = check_ab(o.y, o)
    check_amax(o.y, o)
    assert o.nonzero == 0
    report(f"{name} addend nmod {add_nmod}", o, partial_err_over_bound=p, alpha_err_ulp24=a, beta_err_ulp24=b)


def check_bf16_storage(lib, dev, name):
    """bf16 storage (nprod = 1): y_bf16 stores RNE-to-bf16 of the fp32-storage run's y, with the partials, alpha / beta and amax_out of that run
    (they come from the fp32 values); x_bf16 gives the bits of the fp32-input call on the widened tensor.  A quarter of x and the first output
    channels sit on bf16 ties (inputs(ties=True))."""
    family, shape, kernel, tile, nprod = ROWS[name][:5]
    assert nprod == 1
    t = inputs(shape, ties=True)
    f = _ok(run(lib, dev, shape, kernel, tile, 1, t, stats=2, counters=True, amax=True))
    check_plan(name, f)
    low = f.y.view(torch.int32) & 0xFFFF
    n_ties = int((low == 0x8000).sum())
    assert n_ties >= 16, (name, "the case puts no output on a bf16 tie", n_ties)
    s = _ok(run(lib, dev, shape, kernel, tile, 1, t, stats=2, counters=True, amax=True, y_bf16=True))
    assert torch.equal(s.y.view(torch.int16), bf16_bits(f.y)), (name, "bf16 store is not RNE of the fp32 accumulator")
    assert torch.equal(s.part.view(torch.int64), f.part.view(torch.int64)), (name, "partials differ under bf16 storage")
    assert torch.equal(s.alpha.view(torch.int32), f.alpha.view(torch.int32)) and torch.equal(s.beta.view(torch.int32), f.beta.view(torch.int32))
    assert torch.equal(s.amax, f.amax), (name, "amax_out must come from the fp32 values")
    check_partials(f.y, f)
    check_ab(f.y, f)
    check_amax(f.y, f)
    xb = t["x"].to(torch.bfloat16).float()
    wide = _ok(run(lib, dev, shape, kernel, tile, 1, t, x=xb))
    narrow = _ok(run(lib, dev, shape, kernel, tile, 1, t, x=xb, x_bf16=True))
    assert torch.equal(narrow.y.view(torch.int32), wide.y.view(torch.int32)), (name, "x_bf16", (narrow.y - wide.y).abs().max().item())
    both = _ok(run(lib, dev, shape, kernel, tile, 1, t, x=xb, x_bf16=True, y_bf16=True))
    assert torch.equal(both.y.view(torch.int16), bf16_bits(wide.y)), (name, "x_bf16 + y_bf16")
    report(f"{name} bf16 storage", f, outputs_on_ties=n_ties)


def check_in_amax(lib, dev, name, nprod, pair):
    """in_amax[img] = the float bits of the image's own max |x|, bound_add = 0.25: image img has the bits of the one-image call with the host
    bound max |x[img]| + 0.25 -- the same power-of-two scale, derived on the device (frexpf) and on the host (h2_scale_log2).  A power-of-two scale is exact, so another
    image's maximum shows through fp16 overflow / underflow: 300 under 0.9's scale overflows; a scale one binade off at the edge pair mostly does not."""
    family, shape, kernel, tile, _ = ROWS[name][:5]
    t = inputs(shape)
    N = shape[0]
    x = t["x"].clone()
    maxima = [AMAX_PAIRS[pair][i % 2] for i in range(N)]
    for i, m in enumerate(maxima):
        x[i] *= 0.7 * m / float(x[i].abs().max())
        x[i, 1, 2, 3] = -float(np.float32(m))                               # the maximum itself, exactly
    amax = x.abs().amax(dim=(1, 2, 3))
    assert [float(v) for v in amax] == [float(np.float32(m)) for m in maxima]
    o = _ok(run(lib, dev, shape, kernel, tile, nprod, t, x=x, in_amax=amax.view(torch.int32), bound=0.0, stats=2, counters=True, amax=True))
    check_plan(name, o)
    one = (1,) + shape[1:]
    one_tile = 1 if family == "W1" else tile                            # one image has no chunk of three; every chunk size gives the same bits
    for i in range(min(N, 4)):
        bound = float(np.float32(amax[i].item()) + np.float32(BOUND_ADD))
        al = None if t["al"] is None else t["al"][i:i + 1]
        be = None if t["be"] is None else t["be"][i:i + 1]
        r = _ok(run(lib, dev, one, kernel, one_tile, nprod, t, plain=True, x=x[i:i + 1], al=al, be=be, bound=bound))
        assert torch.equal(o.y[i:i + 1].view(torch.int32), r.y.view(torch.int32)), (name, nprod, pair, "image", i, (o.y[i:i + 1] - r.y).abs().max().item())
    check_partials(o.y, o)
    check_ab(o.y, o)
    check_amax(o.y, o)


def check_refusals(lib, dev):
    """TSNET_ERR_ARG with its message, and NaN-filled y / alpha / beta and the zeroed partials untouched"""
    def refused(o, words, stats=True):
        assert o.rc == TSNET_ERR_ARG, (words, o.rc)
        assert words in o.msg, (words, o.msg)
        assert torch.isnan(o.y.float()).all(), (words, "y was written")
        if stats:
            assert (o.part_all == 0).all() and torch.isnan(o.beta).all() and torch.isnan(o.alpha).all(), (words, "the statistics were written")

    family, shape, kernel, tile, nprod = ROWS["h2_64"][:5]
    t = inputs(shape)
    need = shape[0] * 2 * shape[4] * 2                                  # N * tpi * Cout * 2 with two 4 x 32 tiles per image
    assert _ok(run(lib, dev, shape, kernel, tile, nprod, t, stats=1, part_short=need)).tpi == 2
    refused(run(lib, dev, shape, kernel, tile, nprod, t, stats=1, part_short=need - 1), "part holds")
    refused(run(lib, dev, shape, kernel, tile, nprod, t, stats=2, counters=True, part_short=need - 1), "part holds")
    for name in ("w1_chunk1", "h2s", "h2s32"):
        f, sh, kn, tl, _ = ROWS[name][:5]
        sh = (2,) + sh[1:]
        ts = inputs(sh)
        assert _ok(run(lib, dev, sh, kn, tl, 1, ts)).family == f          # bf16 operands alone are built on this family
        refused(run(lib, dev, sh, kn, tl, 1, ts, x_bf16=True), "bf16-stored input", stats=False)
        _ok(run(lib, dev, sh, kn, tl, 1, ts, y_bf16=True))                # every family stores through conv_epilogue
    refused(run(lib, dev, shape, kernel, tile, 3, t, y_bf16=True), "bf16 storage goes with bf16 operands", stats=False)
    refused(run(lib, dev, shape, kernel, tile, 3, t, x_bf16=True), "bf16 storage goes with bf16 operands", stats=False)
    o = run(lib, dev, shape, kernel, tile, nprod, t, stats=1, null_alpha=True)
    assert o.rc == TSNET_ERR_ARG and "statistics need" in o.msg and torch.isnan(o.y).all() and (o.part_all == 0).all() and torch.isnan(o.beta).all()
    N4 = (4,) + shape[1:]
    add = _rand(7, "addend", (3,) + tuple(shape_out(shape)) + (shape[4],))
    refused(run(lib, dev, N4, kernel, tile, nprod, inputs(N4), stats=1, addend=add), "add_nmod must divide N")
    refused(run(lib, dev, N4, kernel, tile, nprod, inputs(N4), stats=1, addend=add, add_nmod=0), "add_nmod must divide N")


# ---- GPU only: the hand-off under many concurrent arrivals -------------------------------------------------------------------------------
HANDOFF_SHAPE = (13, 32, 64, 16, 200, 3, 1, 1, REFL, NORM)     # tpi = 16; seven 32-wide channel tiles with a ragged last one; 13 images
HANDOFF_TILES = (32, 128)


def check_handoff(lib, dev, tile):
    t = inputs(HANDOFF_SHAPE)
    o = _ok(run(lib, dev, HANDOFF_SHAPE, 2, tile, 3, t, stats=2, counters=True, repeat=3, amax=True))
    assert (o.family, o.tpi, o.fin, o.width) == ("H2", 16, 1, tile), o.info
    assert o.tiles_n == (HANDOFF_SHAPE[4] + tile - 1) // tile
    p = check_partials(o.y, o)
    a, b = check_ab(o.y, o)
    check_amax(o.y, o)
    assert o.nonzero == 0
    report(f"handoff tile {tile}", o, handoffs=HANDOFF_SHAPE[0] * o.tiles_n, partial_err_over_bound=p, alpha_err_ulp24=a, beta_err_ulp24=b)
