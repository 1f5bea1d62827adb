"""Feathered paste masks (`tsnet_blur_mask`, `tsnet_gaussian_box_params`, FrameLoader.feather_mask, csrc/mask_blur.hpp), shared by the
CPU-emulation tier (test_feather_mask.py) and the GPU tier (test_gpu_feather_mask.py).  Everything is EQUALITY.

Two expected-value functions:
  (a) `expect_pillow`: live Pillow, the statement of the operation -- Image.fromarray(m, "L").filter(ImageFilter.GaussianBlur(r));
  (b) `expect_numpy`: a restatement of what Pillow computes, which is the contract:
      1. the box radius R of a blur radius r with passes = 3, in float32: s2 = r r / passes; L = (float)sqrt(12.0 s2 + 1.0) (a double inside);
         l = (float)floor((L - 1.0) / 2.0); a = (2l + 1)(l(l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)); R = l + a;
      2. radius = (int)R; ww = (uint32)((float)(1 << 24) / (R 2 + 1)); fw = ((1 << 24) - (2 radius + 1) ww) / 2;
      3. one pass along a line, clamp replicating the end pixels: acc = sum of in[clamp(x + d)] over |d| <= radius,
         far = in[clamp(x - radius - 1)] + in[clamp(x + radius + 1)], out[x] = (acc ww + far fw + (1 << 23)) >> 24;
      4. three passes along the rows, then three along the columns; an axis whose radius is 0 is skipped.
(b) does not depend on the installed Pillow; a disagreement of (a) alone gets PIL_NOTE.  test_feather_mask.py checks (a) == (b) on every case.

The output sits in a buffer with SENTINEL bytes before and after it, and so does the intermediate; the sentinels are compared too."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from PIL import Image, ImageFilter

PIL_NOTE = ("live Pillow %s disagrees with the numpy restatement; if the kernel equals the restatement (the contract), this Pillow's GaussianBlur "
            "differs" % Image.__version__)
SENTINEL, SENTINEL_BYTE = 4096, 0xA5
PASSES = 3
MAX_SIDE = 512                                                              # kMbMaxSide of csrc/mask_blur.hpp

RADII = (0.3, 1, 1.5, 3.7, 12.25, 40)                                       # 0.3: radius 0, the fractional part alone; 1: float32 against double
PAIRS = ((0, 3), (3, 0), (1, 7.5), (12.25, 0.3), (0, 0))
SMALL = ((1, 9), (33, 2), (3, 3), (5, 7))                                   # (H, W): a side shorter than the radius, both ends replicated at once
KINDS = ("random", "rect", "const255", "binary01")


def _cases():
    """[(id, (F, H, W), radius or (rx, ry), input kind)]: the smallest shapes at which each branch can go wrong"""
    out = []
    for h, w in SMALL:
        out += [(f"{h}x{w}-r{r}", (1, h, w), r, "random") for r in RADII]
    out += [(f"37x301-r{r}", (1, 37, 301), r, "random") for r in (1, 3.7, 12.25)]       # odd width, ragged last tile, several column tiles
    out += [(f"37x301-r{rx}_{ry}", (1, 37, 301), (rx, ry), "random") for rx, ry in PAIRS]
    out += [(f"70x130-r{rx}_{ry}-rect", (2, 70, 130), (rx, ry), "rect") for rx, ry in PAIRS]   # two row groups, three column tiles
    out += [(f"64x48-r{r}", (1, 64, 48), r, "random") for r in RADII + (100,)]
    out += [(f"64x48-r{r}-{k}", (1, 64, 48), r, k) for k in KINDS[1:] for r in (0.3, 1, 3.7, 40)]
    out.append(("256x256-F2", (2, 256, 256), 12.25, "random"))
    out.append(("512x512", (1, 512, 512), 3.7, "rect"))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


def rect_of(H, W):
    """the rectangle of the `rect` inputs: off centre, not empty at any size of the list"""
    x0, y0 = W // 4, H // 5
    return x0, y0, max(W - W // 7 - 1, x0 + 1), max(H - H // 6 - 1, y0 + 1)


def make_input(name, shape, kind):
    F, H, W = shape
    rng = np.random.default_rng(sum(map(ord, name)))
    if kind == "random":                                                   # random bytes with bands forced to 0 and to 255, other bands per frame
        m = rng.integers(0, 256, shape, dtype=np.uint8)
        m[:, H // 4:H // 4 + 10] = 0
        m[:, :, W // 2:W // 2 + 9] = 255
        m[:, H // 2:H // 2 + 8, :W // 3] = 0
        for f in range(1, F):
            m[f, :, :W // 5] = 255
        return m
    if kind == "const255":
        return np.full(shape, 255, np.uint8)
    x0, y0, x1, y1 = rect_of(H, W)
    m = np.zeros(shape, np.uint8)
    m[:, y0:y1, x0:x1] = 1 if kind == "binary01" else 255
    return m


# ------------------------------------------------------------------------------------------------------------------------- expected values
def as_pair(radius):
    return (radius, radius) if np.ndim(radius) == 0 else tuple(radius)


def box_params(r, passes=PASSES):
    """(radius, ww, fw) of steps 1-2, in float32 as the C code computes them"""
    f = np.float32
    r = f(r)
    s2 = r * r / f(passes)
    L = f(np.sqrt(12.0 * float(s2) + 1.0))
    l = f(np.floor((float(L) - 1.0) / 2.0))
    a = (f(2) * l + f(1)) * (l * (l + f(1)) - f(3) * s2)
    a = a / (f(6) * (s2 - (l + f(1)) * (l + f(1))))
    R = l + a
    assert R.dtype == np.float32
    radius = int(R)
    ww = int(f(1 << 24) / (R * f(2) + f(1)))
    fw = ((1 << 24) - (2 * radius + 1) * ww) // 2
    return radius, ww, fw


def box_pass(a, axis, radius, ww, fw):
    """step 3 along `axis` of a uint8 array"""
    a = np.moveaxis(a, axis, -1).astype(np.int64)
    n = a.shape[-1]
    p = np.pad(a, [(0, 0)] * (a.ndim - 1) + [(radius + 1, radius + 1)], mode="edge")          # p[.., i] = in[clamp(i - radius - 1)]
    c = np.concatenate([np.zeros(p.shape[:-1] + (1,), np.int64), np.cumsum(p, -1)], -1)
    x = np.arange(n)
    acc = c[..., x + 2 * radius + 2] - c[..., x + 1]
    far = p[..., x] + p[..., x + 2 * radius + 2]
    t = acc * ww + far * fw + (1 << 23)
    assert int(t.max()) < 1 << 32
    return np.moveaxis((t >> 24).astype(np.uint8), -1, axis)


def expect_numpy(m, radius, binary=False):
    """(b) the restatement: m (F,H,W) uint8"""
    rx, ry = as_pair(radius)
    out = np.where(m != 0, 255, 0).astype(np.uint8) if binary else m.copy()
    for r, axis in ((rx, 2), (ry, 1)):
        if r == 0:
            continue
        k = box_params(r)
        for _ in range(PASSES):
            out = box_pass(out, axis, *k)
    return out


def expect_pillow(m, radius, binary=False):
    """(a) live Pillow"""
    if binary:
        m = np.where(m != 0, 255, 0).astype(np.uint8)
    r = radius if np.ndim(radius) == 0 else tuple(radius)
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(m[f]), "L").filter(ImageFilter.GaussianBlur(r))) for f in range(m.shape[0])])


_expected = {}


def expected(cid):
    """{m, radius, kind, binary, rect, want} of a case, computed once and shared (read-only arrays)"""
    if cid not in _expected:
        _, shape, radius, kind = next(c for c in CASES if c[0] == cid)
        m = make_input(cid, shape, kind)
        binary = kind == "binary01"
        want = expect_numpy(m, radius, binary)
        m.setflags(write=False); want.setflags(write=False)
        _expected[cid] = dict(m=m, radius=radius, kind=kind, binary=binary, want=want,
                              rect=rect_of(*shape[1:]) if kind in ("rect", "binary01") else None)
    return _expected[cid]


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


def blur_c(lib, src_d, shape, rect_t, radius, flag_bits, out_t, tmp_t, stream=None, **over):
    """the C entry on device tensors; `over` replaces single arguments (the error tests)"""
    rx, ry = as_pair(radius)
    F, H, W = shape
    a = dict(src=None if src_d is None else src_d.data_ptr(), F=F, H=H, W=W, rect=None if rect_t is None else (C.c_int * 4)(*rect_t),
             rx=rx, ry=ry, flags=flag_bits, out=out_t.data_ptr(), tmp=tmp_t.data_ptr())
    a.update(over)
    return lib.tsnet_blur_mask(a["src"], a["F"], a["H"], a["W"], a["rect"], a["rx"], a["ry"], a["flags"], a["out"], a["tmp"], stream)


def check_case(lib, dev, ld, cid, routes=(0,)):
    """one case through the C entry (output and intermediate between sentinels; every route of `routes`) and through
    FrameLoader.feather_mask; a rectangle input also in its in = NULL form.  Asserts equality with (b); returns a report entry."""
    e = expected(cid)
    dev = torch.device(dev)
    shape = e["m"].shape
    want = torch.from_numpy(np.array(e["want"]))
    src_d = torch.from_numpy(np.array(e["m"])).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
    rep = dict(case=cid)
    forms = [("image", src_d, None)] + ([("rect", None, e["rect"])] if e["kind"] == "rect" else [])
    for form, s, rect in forms:
        for route in routes:
            obuf, out = guarded(shape, dev)
            tbuf, tmp = guarded(shape, dev)
            rc = blur_c(lib, s, shape, rect, e["radius"], (1 if e["binary"] else 0) | (route << 8), out, tmp, stream)
            assert rc == 0, (cid, form, route, rc, lib.tsnet_op_last_error().decode())
            got = out.cpu()
            key = f"differing_{form}_route{route}"
            rep[key] = int((got != want).sum())
            assert sentinels_intact(obuf) and sentinels_intact(tbuf), (rep, "sentinels")
            assert torch.equal(got, want), rep
            assert torch.equal(src_d.cpu(), torch.from_numpy(np.array(e["m"])))              # the input is left as it is
    got2 = ld.feather_mask(np.array(e["m"]) if shape[0] == 1 else src_d, e["radius"], binary=e["binary"])   # arrays and tensors
    assert got2.device.type == dev.type and got2.dtype == torch.uint8
    rep["differing_loader"] = int((got2.cpu() != want).sum())
    assert torch.equal(got2.cpu(), want), rep
    if e["kind"] == "rect":
        got3 = ld.feather_mask(None, e["radius"], size=shape, rect=e["rect"]).cpu()
        assert torch.equal(got3, want), (rep, "loader, rectangle form")
    return rep
