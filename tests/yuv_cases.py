"""Frames in and out as YUV 4:2:0 (`tsnet_yuv_coeffs`, `tsnet_rgb_to_yuv420`, `tsnet_yuv420_to_rgb`, FrameLoader.to_yuv420 / from_yuv420,
csrc/yuv_frames.hpp), shared by the CPU-emulation tier (test_yuv_frames.py) and the GPU tier (test_gpu_yuv_frames.py).  Every comparison
with the restatement is EQUALITY.

The contract, restated here in numpy on int64:
  tables   `derive(standard, full_range)`: the rows Y = sy (Kr, Kg, Kb), Cb = sc (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)), Cr = sc (1 - Kr, -Kg, -Kb) /
           (2 (1 - Kr)) in double, times 65536, rounded; the green entry corrected so that the Y row sums to round(65536 sy) and the chroma rows
           to 0; inv = {iy, rv, gu, gv, bu, oy}.  PINNED_FWD / PINNED_INV are the values the issue states.
  forward  `rgb_to_yuv`: Y = clamp((cR R + cG G + cB B + (off << 16) + 32768) >> 16); a chroma sample is clamp((S (4 / n) + (off << 18) +
           (1 << 17)) >> 18) with S the sum of its plane's cR R + cG G + cB B over the n = 4, 2 or 1 pixels of its 2 x 2 block inside the frame.
  inverse  `yuv_to_rgb`: the sample at (y >> 1, x >> 1); t = (Y - oy) iy, u = Cb - 128, v = Cr - 128; R = clamp((t + rv v + 32768) >> 16),
           G = clamp((t + gu u + gv v + 32768) >> 16), B = clamp((t + bu u + 32768) >> 16).
  layouts  0 = I420 (Y, Cb, Cr planes), 1 = NV12 (Y plane, interleaved Cb Cr rows); h w + 2 ch cw bytes per frame, frames contiguous.

Outputs sit between SENTINEL bytes that are compared too."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

SENTINEL, SENTINEL_BYTE = 4096, 0xA5
STANDARDS = {"bt601": (601, 0.299, 0.114), "bt709": (709, 0.2126, 0.0722)}
TABLES = (("bt601", True), ("bt601", False), ("bt709", True), ("bt709", False))
LAYOUTS = ("i420", "nv12")
ROW_SUM_MAX, INV_COEF_MAX, MAX_FRAMES = 1 << 17, 1 << 21, 65535                # kYuvRowSumMax, kYuvInvCoefMax, kYuvMaxFrames

PINNED_FWD = {   # rows Y / Cb / Cr without their offsets
    ("bt601", True): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329)),
    ("bt601", False): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681)),
    ("bt709", True): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005)),
    ("bt709", False): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639)),
}
PINNED_INV = {   # iy, rv, gu, gv, bu
    ("bt601", True): (65536, 91881, -22553, -46802, 116130),
    ("bt601", False): (76309, 104597, -25675, -53279, 132201),
    ("bt709", True): (65536, 103206, -12276, -30679, 121609),
    ("bt709", False): (76309, 117489, -13975, -34925, 138438),
}


# ------------------------------------------------------------------------------------------------------------------------------- the tables
def matrix(standard, full_range):
    """the real 3 x 3 matrix (rows Y, Cb, Cr), the offsets, and (Kr, Kg, Kb, sy, sc)"""
    _, kr, kb = STANDARDS[standard]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    rows = ((sy * kr, sy * kg, sy * kb),
            (sc * -kr / (2 * (1 - kb)), sc * -kg / (2 * (1 - kb)), sc * (1 - kb) / (2 * (1 - kb))),
            (sc * (1 - kr) / (2 * (1 - kr)), sc * -kg / (2 * (1 - kr)), sc * -kb / (2 * (1 - kr))))
    return rows, (0 if full_range else 16, 128, 128), (kr, kg, kb, sy, sc)


def derive(standard, full_range):
    """(fwd int32[12], inv int32[6]) as tsnet_yuv_coeffs computes them"""
    rnd = lambda v: int(math.floor(v * 65536.0 + 0.5))
    rows, offs, (kr, kg, kb, sy, sc) = matrix(standard, full_range)
    fwd = []
    for r, want_sum in zip(range(3), (rnd(sy), 0, 0)):
        c = [rnd(v) for v in rows[r]]
        c[1] = want_sum - c[0] - c[2]
        fwd += c + [offs[r]]
    inv = [rnd(1 / sy), rnd(2 * (1 - kr) / sc), -rnd(kb * 2 * (1 - kb) / (kg * sc)), -rnd(kr * 2 * (1 - kr) / (kg * sc)), rnd(2 * (1 - kb) / sc), offs[0]]
    return np.array(fwd, np.int32), np.array(inv, np.int32)


def coeffs_c(lib, standard, full_range):
    fwd, inv = np.full(12, -7, np.int32), np.full(6, -7, np.int32)
    rc = lib.tsnet_yuv_coeffs(STANDARDS[standard][0] if standard in STANDARDS else standard, int(full_range), fwd.ctypes.data, inv.ctypes.data)
    return rc, fwd, inv


# ------------------------------------------------------------------------------------------------------------------------- the restatement
def frame_bytes(h, w):
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def _pack(Y, Cb, Cr, layout):
    F = Y.shape[0]
    if layout == "i420":
        parts = [Y.reshape(F, -1), Cb.reshape(F, -1), Cr.reshape(F, -1)]
    else:
        parts = [Y.reshape(F, -1), np.stack([Cb, Cr], -1).reshape(F, -1)]
    return np.concatenate(parts, 1).astype(np.uint8)


def _unpack(yuv, h, w, layout):
    F, ch, cw = yuv.shape[0], (h + 1) // 2, (w + 1) // 2
    Y = yuv[:, :h * w].reshape(F, h, w)
    if layout == "i420":
        return Y, yuv[:, h * w:h * w + ch * cw].reshape(F, ch, cw), yuv[:, h * w + ch * cw:].reshape(F, ch, cw)
    uv = yuv[:, h * w:].reshape(F, ch, cw, 2)
    return Y, uv[..., 0], uv[..., 1]


def rgb_to_yuv_planes(rgb, fwd):
    """(Y (F,h,w), Cb (F,ch,cw), Cr (F,ch,cw)) int64, clamped, and the two unclamped chroma planes"""
    F, h, w, _ = rgb.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    c = np.asarray(fwd, np.int64).reshape(3, 4)
    p = rgb.astype(np.int64)
    lin = lambda r: c[r, 0] * p[..., 0] + c[r, 1] * p[..., 1] + c[r, 2] * p[..., 2]
    Y = np.clip((lin(0) + (int(c[0, 3]) << 16) + 32768) >> 16, 0, 255)
    inside = np.zeros((1, 2 * ch, 2 * cw), np.int64)
    inside[:, :h, :w] = 1
    n = inside.reshape(1, ch, 2, cw, 2).sum((2, 4))
    raw = []
    for r in (1, 2):
        L = np.zeros((F, 2 * ch, 2 * cw), np.int64)
        L[:, :h, :w] = lin(r)
        S = L.reshape(F, ch, 2, cw, 2).sum((2, 4)) * (4 // n)
        assert int(np.abs(S).max()) + (256 << 18) < 1 << 31                 # everything fits 32 bits
        raw.append((S + (int(c[r, 3]) << 18) + (1 << 17)) >> 18)
    return Y, np.clip(raw[0], 0, 255), np.clip(raw[1], 0, 255), raw


def rgb_to_yuv(rgb, fwd, layout="i420"):
    """the forward restatement: (F,h,w,3) uint8 -> (F, frame_bytes) uint8"""
    Y, Cb, Cr, _ = rgb_to_yuv_planes(rgb, fwd)
    return _pack(Y, Cb, Cr, layout)


def yuv_to_rgb(yuv, h, w, inv, layout="i420"):
    """the inverse restatement: (F, frame_bytes) uint8 -> (F,h,w,3) uint8"""
    iy, rv, gu, gv, bu, oy = (int(v) for v in inv)
    Y, Cb, Cr = (a.astype(np.int64) for a in _unpack(yuv, h, w, layout))
    up = lambda a: np.repeat(np.repeat(a, 2, 1), 2, 2)[:, :h, :w]
    t, u, v = (Y - oy) * iy, up(Cb) - 128, up(Cr) - 128
    assert int(np.abs(t).max()) + 128 * (abs(gu) + abs(gv) + abs(rv) + abs(bu)) + 32768 < 1 << 31
    out = np.stack([t + rv * v, t + gu * u + gv * v, t + bu * u], -1)
    return np.clip((out + 32768) >> 16, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------- cases
SHAPES = ((1, 1, 1), (1, 2, 2),                                               # blocks of n = 1 and n = 4 alone
          (1, 1, 9), (1, 9, 1),                                               # n = 2 along each axis
          (2, 5, 7), (3, 5, 5),                                               # odd x odd frames of odd byte size: later frames and both chroma planes unaligned
          (1, 6, 4), (1, 6, 5), (1, 6, 6), (1, 6, 7),                         # 3 w mod 4 = 0, 3, 2, 1: every row alignment
          (1, 4, 8), (1, 4, 9), (1, 4, 15), (1, 4, 16), (1, 4, 17),           # one lane block, one plus a ragged edge, two
          (2, 18, 33),                                                        # interior, right edge and bottom edge together
          (1, 64, 130))                                                       # more than one workgroup
CONTENTS = ("random", "primaries", "checker", "hramp", "vramp")
CASES = [(f"{F}x{h}x{w}-{k}", (F, h, w), k, TABLES[(si + ki) % 4]) for si, (F, h, w) in enumerate(SHAPES) for ki, k in enumerate(CONTENTS)]
IDS = [c[0] for c in CASES]


def make_rgb(name, shape, kind):
    F, h, w = shape
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind == "random":
        return rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    if kind == "primaries":                                                   # every pixel a saturated primary or secondary (black and white too)
        return (rng.integers(0, 2, (F, h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "checker":                                                     # 0 / 255 at pixel pitch: the block mean decides the chroma
        v = (((y + x) & 1) * 255).astype(np.uint8)
        a = np.stack([v, 255 - v, v], -1)
    elif kind == "hramp":
        a = np.stack([(x * 255 // max(w - 1, 1)), 255 - (x * 255 // max(w - 1, 1)), (x * 37) & 255], -1).astype(np.uint8)
    else:
        a = np.stack([(y * 29) & 255, (y * 255 // max(h - 1, 1)), 255 - (y * 255 // max(h - 1, 1))], -1).astype(np.uint8)
    return np.stack([np.roll(a, f, 2) for f in range(F)])                    # frame f: the channels rotated


def make_yuv(name, shape):
    """random yuv bytes for the inverse: every combination, out-of-gamut ones (which reach the clamps) included, and a band of extremes"""
    F, h, w = shape
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    yuv = rng.integers(0, 256, (F, frame_bytes(h, w)), dtype=np.uint8)
    yuv[:, ::7] = 255
    yuv[:, 3::11] = 0
    return yuv


_expected = {}


def expected(cid):
    """{rgb, table, fwd, inv, yuv_in, want[layout], want_rgb[layout]} of a case, computed once and shared (read-only arrays)"""
    if cid not in _expected:
        _, shape, kind, table = next(c for c in CASES if c[0] == cid)
        fwd, inv = derive(*table)
        rgb, yuv_in = make_rgb(cid, shape, kind), make_yuv(cid, shape)
        e = dict(rgb=rgb, table=table, fwd=fwd, inv=inv, yuv_in=yuv_in, shape=shape,
                 want={l: rgb_to_yuv(rgb, fwd, l) for l in LAYOUTS}, want_rgb={l: yuv_to_rgb(yuv_in, shape[1], shape[2], inv, l) for l in LAYOUTS})
        for a in [rgb, yuv_in] + list(e["want"].values()) + list(e["want_rgb"].values()):
            a.setflags(write=False)
        _expected[cid] = e
    return _expected[cid]


_big = {}


def all_colours(cut=None):
    """(1, 4096, 4096, 3): every RGB value once, in a seeded permutation (cut: its top-left cut x cut corner); and its 601-full restatement"""
    if "rgb" not in _big:
        v = np.random.default_rng(2024).permutation(1 << 24).astype(np.uint32)
        rgb = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
        rgb.setflags(write=False)
        _big["rgb"] = rgb
    rgb = _big["rgb"] if cut is None else np.ascontiguousarray(_big["rgb"][:, :cut, :cut])
    key = ("want", cut)
    if key not in _big:
        _big[key] = rgb_to_yuv(rgb, derive("bt709", False)[0], "i420")
        _big[key].setflags(write=False)
    return rgb, _big[key]


def lattice():
    """(1, 1024, 1024, 3): constant 2 x 2 blocks over the lattice of every fourth value per channel (64^3 colours = 512 x 512 blocks)"""
    if "lattice" not in _big:
        v = np.arange(1 << 18, dtype=np.uint32).reshape(512, 512)
        a = np.stack([(v >> 12) & 63, (v >> 6) & 63, v & 63], -1).astype(np.uint8) * 4
        a = np.repeat(np.repeat(a, 2, 0), 2, 1)[None]
        a.setflags(write=False)
        _big["lattice"] = a
    return _big["lattice"]


# ------------------------------------------------------------------------------------------------------------------------- the device side
def guarded(shape, dev):
    """SENTINEL bytes | an array of `shape` | SENTINEL bytes, all of them the sentinel byte -> (buffer, view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * SENTINEL,), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    return buf, buf[SENTINEL:SENTINEL + n].view(tuple(shape))


def sentinels_intact(buf):
    b = buf.cpu()
    return bool((b[:SENTINEL] == SENTINEL_BYTE).all()) and bool((b[-SENTINEL:] == SENTINEL_BYTE).all())


def untouched(buf):
    return bool((buf.cpu() == SENTINEL_BYTE).all())


def _stream(dev):
    dev = torch.device(dev)
    return torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None


def forward_c(lib, rgb_d, shape, fwd, lay, out_t, stream=None, **over):
    """tsnet_rgb_to_yuv420 on device tensors; `over` replaces single arguments (the error tests)"""
    F, h, w = shape
    fwd = np.ascontiguousarray(fwd, np.int32)
    a = dict(src=rgb_d.data_ptr(), F=F, h=h, w=w, table=fwd.ctypes.data, layout=LAYOUTS.index(lay), out=out_t.data_ptr())
    a.update(over)
    return lib.tsnet_rgb_to_yuv420(a["src"], a["F"], a["h"], a["w"], a["table"], a["layout"], a["out"], stream)


def inverse_c(lib, yuv_d, shape, inv, lay, out_t, stream=None, **over):
    F, h, w = shape
    inv = np.ascontiguousarray(inv, np.int32)
    a = dict(src=yuv_d.data_ptr(), F=F, h=h, w=w, table=inv.ctypes.data, layout=LAYOUTS.index(lay), out=out_t.data_ptr())
    a.update(over)
    return lib.tsnet_yuv420_to_rgb(a["src"], a["F"], a["h"], a["w"], a["table"], a["layout"], a["out"], stream)


def check_case(lib, dev, ld, cid):
    """one case, both layouts, forward and inverse: through the C entries with the output between sentinels, and through FrameLoader.
    Asserts equality with the restatement; returns a report entry."""
    e = expected(cid)
    dev = torch.device(dev)
    F, h, w = shape = e["shape"]
    std, full = e["table"]
    rgb_d, yuv_d = torch.from_numpy(np.array(e["rgb"])).to(dev), torch.from_numpy(np.array(e["yuv_in"])).to(dev)
    rep = dict(case=cid)
    for layout in LAYOUTS:
        want = torch.from_numpy(np.array(e["want"][layout]))
        obuf, out = guarded((F, frame_bytes(h, w)), dev)
        rc = forward_c(lib, rgb_d, shape, e["fwd"], layout, out, _stream(dev))
        assert rc == 0, (cid, layout, rc, lib.tsnet_op_last_error().decode())
        got = out.cpu()
        rep[f"differing_fwd_{layout}"] = int((got != want).sum())
        assert sentinels_intact(obuf), (rep, "sentinels")
        assert torch.equal(got, want), rep
        got2 = ld.to_yuv420(np.array(e["rgb"]) if F == 1 else rgb_d, layout, std, full)               # arrays and tensors
        assert got2.device.type == dev.type and got2.dtype == torch.uint8 and torch.equal(got2.cpu(), want), (rep, "loader")

        want = torch.from_numpy(np.array(e["want_rgb"][layout]))
        obuf, out = guarded((F, h, w, 3), dev)
        rc = inverse_c(lib, yuv_d, shape, e["inv"], layout, out, _stream(dev))
        assert rc == 0, (cid, layout, rc, lib.tsnet_op_last_error().decode())
        got = out.cpu()
        rep[f"differing_inv_{layout}"] = int((got != want).sum())
        assert sentinels_intact(obuf), (rep, "sentinels")
        assert torch.equal(got, want), rep
        got2 = ld.from_yuv420(np.array(e["yuv_in"]) if F == 1 else yuv_d, (h, w), layout, std, full)
        assert got2.device.type == dev.type and torch.equal(got2.cpu(), want), (rep, "loader")
    assert torch.equal(rgb_d.cpu(), torch.from_numpy(np.array(e["rgb"]))) and torch.equal(yuv_d.cpu(), torch.from_numpy(np.array(e["yuv_in"])))
    return rep


def check_large(ld, cut=None):
    """the all-colours frame (709 limited, I420) and the lattice frame with its round trip (all four tables) through FrameLoader on ld.device"""
    rgb, want = all_colours(cut)
    got = ld.to_yuv420(torch.from_numpy(np.array(rgb)), "i420", "bt709", False).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    lat = lattice()
    rep = {}
    for (std, full), layout in zip(TABLES, ("i420", "nv12", "nv12", "i420")):
        fwd, inv = derive(std, full)
        yuv = ld.to_yuv420(torch.from_numpy(np.array(lat)), layout, std, full)
        w1 = rgb_to_yuv(lat, fwd, layout)
        assert np.array_equal(yuv.cpu().numpy(), w1), (std, full, "forward")
        back = ld.from_yuv420(yuv, (1024, 1024), layout, std, full).cpu().numpy()
        assert np.array_equal(back, yuv_to_rgb(w1, 1024, 1024, inv, layout)), (std, full, "inverse")
        worst = int(np.abs(back.astype(np.int16) - lat.astype(np.int16)).max())
        rep[f"{std}-{'full' if full else 'limited'}"] = worst
        assert worst <= (1 if full else 2), (std, full, worst)                # the exhaustive maxima over all colours on constant blocks
    return rep


# ------------------------------------------------------------------------------------------------------------------------------- refusals
ERR_SHAPE = (2, 6, 10)
ROW_TOO_LARGE = np.array([65536, 65536, 1, 0, -11058, -21710, 32768, 128, 32768, -27439, -5329, 128], np.int32)
OFFSET_TOO_LARGE = np.array([19595, 38470, 7471, 256, -11058, -21710, 32768, 128, 32768, -27439, -5329, 128], np.int32)
OFFSET_NEGATIVE = np.array([19595, 38470, 7471, 0, -11058, -21710, 32768, 128, 32768, -27439, -5329, -1], np.int32)
INV_TOO_LARGE = np.array([65536, (1 << 21) + 1, -22553, -46802, 116130, 0], np.int32)
INV_OFFSET = np.array([65536, 91881, -22553, -46802, 116130, 256], np.int32)
ARG_ERRORS = {   # cause -> (direction, overrides, a word of the message)
    "src_null": ("both", dict(src=None), "null"),
    "out_null": ("both", dict(out=None), "null"),
    "table_null": ("both", dict(table=None), "null table"),
    "F_zero": ("both", dict(F=0), "shape"),
    "h_zero": ("both", dict(h=0), "shape"),
    "w_negative": ("both", dict(w=-4), "shape"),
    "F_over_the_grid": ("both", dict(F=MAX_FRAMES + 1), "kYuvMaxFrames"),
    "frame_over_32_bits": ("both", dict(h=30000, w=30000), "2^31"),
    "layout_unknown": ("both", dict(layout=2), "layout"),
    "layout_negative": ("both", dict(layout=-1), "layout"),
    "row_sum_overflows": ("fwd", dict(table=ROW_TOO_LARGE.ctypes.data), "kYuvRowSumMax"),
    "offset_over_255": ("fwd", dict(table=OFFSET_TOO_LARGE.ctypes.data), "offset"),
    "offset_negative": ("fwd", dict(table=OFFSET_NEGATIVE.ctypes.data), "offset"),
    "inverse_entry_overflows": ("inv", dict(table=INV_TOO_LARGE.ctypes.data), "kYuvInvCoefMax"),
    "inverse_offset_over_255": ("inv", dict(table=INV_OFFSET.ctypes.data), "offset"),
}


def check_refusal(lib, dev, cause):
    """the good call writes, the same call with the fault returns TSNET_ERR_ARG and writes nothing"""
    which, over, word = ARG_ERRORS[cause]
    F, h, w = ERR_SHAPE
    fwd, inv = derive("bt601", True)
    rgb = torch.from_numpy(make_rgb("errors", ERR_SHAPE, "random")).to(dev)
    yuv = torch.from_numpy(make_yuv("errors", ERR_SHAPE)).to(dev)
    for tag, name, call, src, table, oshape in (("fwd", "rgb_to_yuv420", forward_c, rgb, fwd, (F, frame_bytes(h, w))),
                                                ("inv", "yuv420_to_rgb", inverse_c, yuv, inv, (F, h, w, 3))):
        if which not in ("both", tag):
            continue
        obuf, out = guarded(oshape, dev)
        assert call(lib, src, ERR_SHAPE, table, "i420", out, _stream(dev)) == 0
        assert not untouched(obuf) and sentinels_intact(obuf)
        obuf.fill_(SENTINEL_BYTE)
        assert call(lib, src, ERR_SHAPE, table, "i420", out, _stream(dev), **over) == -1, (cause, name)
        msg = lib.tsnet_op_last_error().decode()
        assert msg.startswith(name) and word in msg, (cause, msg)
        assert untouched(obuf), (cause, name)


# ------------------------------------------------------------------------------------------------------------------------- Y4M + the clip
def write_y4m(path, yuv, w, h, **kw):
    from wacv23_tsnet_amd import video
    with video.Y4MWriter(path, w, h, **kw) as wr:
        wr.write(yuv)
    return path


def read_y4m(path):
    from wacv23_tsnet_amd import video
    with video.Y4MReader(path) as rd:
        frames = rd.read(1 << 20)
        return rd, frames.numpy()


def check_clip_runner(runner, ld, drv_args, video_frames, pbox, tmp_path, batch_note=""):
    """ClipRunner.run(y4m=...) with and without paste_into (the caller chose a frame count that leaves a ragged last group): the file's frames
    equal to_yuv420 of what `run` returns without y4m (and the restatement of it), and `run` returns the count"""
    from wacv23_tsnet_amd import video
    small = runner.run(*drv_args)
    full = runner.run(*drv_args, paste_into=video_frames, paste_box=pbox)
    n = small.shape[0]
    for name, frames, kw, table in (("gen", small, {}, ("bt601", True)), ("full", full, dict(paste_into=video_frames, paste_box=pbox), ("bt709", False))):
        path = str(tmp_path / f"{name}.y4m")
        got = runner.run(*drv_args, y4m=path, y4m_standard=table[0], y4m_full_range=table[1], **kw)
        assert got == n, (name, got)
        rd, file_frames = read_y4m(path)
        assert (rd.width, rd.height, rd.full_range, rd.fps) == (frames.shape[2], frames.shape[1], table[1], (25, 1))
        assert np.array_equal(file_frames, ld.to_yuv420(frames, "i420", *table).cpu().numpy()), name
        assert np.array_equal(file_frames, rgb_to_yuv(frames, derive(*table)[0], "i420")), name
    # a writer of the caller's: appended to over two runs and left open; with out_dir the RGB frames come back as without y4m
    path = str(tmp_path / "twice.y4m")
    with video.Y4MWriter(path, small.shape[2], small.shape[1], fps=(30, 1)) as wr:
        assert runner.run(*drv_args, y4m=wr) == n
        again = runner.run(*drv_args, y4m=wr, out_dir=str(tmp_path / "strips"))
        assert wr.frames_written == 2 * n
    assert np.array_equal(again, small)
    rd, file_frames = read_y4m(path)
    assert rd.fps == (30, 1) and file_frames.shape[0] == 2 * n and np.array_equal(file_frames[:n], file_frames[n:])
    return small, full
