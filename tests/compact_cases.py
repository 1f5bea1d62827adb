"""Compact inputs (tsnet_*_u8, Engine calls on uint8 tensors) against the float32 path, shared by the CPU-emulation tier
(test_compact_inputs.py) and the GPU tier (test_gpu_compact_inputs.py).

A case draws the COMPACT form -- image bytes, class-index maps, 0 / 1 mask bytes -- and widens it the way the reference's loaders do:
byte.float() - mean, one-hot by comparison, mask.float().  Each step is exact arithmetic (or the very fp32 operation the packing kernel
performs), so the acceptance criterion everywhere is bit equality: every comparison made on these cases is torch.equal."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import helpers as Hh
import op_cases as oc
from oracle import tsnet_oracle as O
from wacv23_tsnet_amd import demo, prng

MEAN = [float(v) for v in demo.IMG_MEAN]                       # B, G, R (float32 values)


def _bytes(seed, name, shape, hi=256):
    """uint8 uniform on 0 .. hi-1"""
    return (prng.uniform01(seed, name, shape) * hi).floor().clamp_(max=hi - 1).to(torch.uint8)


def widen_img(b, mean=MEAN):
    return b.float() - torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)


def widen_lbl(c, L):
    """class map (B,H,W) -> one-hot (B,L,H,W); an index >= L gives zeros everywhere, as vl2ch's `== ci`"""
    return torch.stack([(c == j) for j in range(L)], dim=1).float()


def widen_box(m):
    return m.float()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the packing kernel alone: tsnet_op_pack_input_u8 against tsnet_op_pack_input on the widened tensors
PACK_U8_CASES = {                                               # (S, B, H, W, L, nimg, Cp, coords, divisors, plant 255 in the labels)
    "face_32": (2, 2, 32, 32, 2, 3, 8, True, (255.0, 1.0), False),              # whole words everywhere: the 32-bit loads
    "face_32_no_coords_cp16": (1, 2, 32, 32, 2, 3, 16, False, None, False),
    "pose_32": (2, 2, 32, 32, 25, 3, 32, True, None, True),
    "label_only_face_32": (1, 3, 32, 32, 2, 0, 8, True, None, True),
    "label_only_pose_32": (1, 2, 32, 32, 25, 0, 32, False, None, False),
    "odd_5x7_face": (2, 4, 5, 7, 2, 3, 8, True, (1.0, 255.0), True),            # H*W = 35: S*B = 8 images, planes at every residue mod 4, a 3-pixel tail
    "odd_5x7_pose": (1, 3, 5, 7, 25, 3, 32, True, None, False),
    "odd_5x7_label_only": (2, 2, 5, 7, 25, 0, 32, True, None, True),
    "two_blocks_33x33": (1, 2, 33, 33, 2, 3, 8, True, None, False),             # 1089 pixels: above one workgroup's 1024, odd, a 1-pixel tail
    "loop_363x362": (1, 2, 363, 362, 2, 0, 8, False, None, False),              # 131406 pixels: above the grid's 131072, the loop repeats; 2-pixel tail
}


def pack_pair(lib, dev, S, B, H, W, L, nimg, Cp, coords, divs, plant, seed=0):
    """-> dict of (compact result, float result) pairs: out, amax, bbox"""
    divs = list(divs) if divs is not None else [255.0] * S
    img8 = [_bytes(seed + s, "img", (B, 3, H, W)) for s in range(S)]
    lbl8 = [_bytes(seed + s, "lbl", (B, H, W), L) for s in range(S)]
    box8 = [_bytes(seed + s, "box", (B, H, W), 2) for s in range(S)]
    if plant:                                                   # indices >= L: every label channel 0
        for t in lbl8:
            t.view(-1)[::5] = 255
            t.view(-1)[3::11] = L
    imgf, lblf = [widen_img(t) for t in img8], [widen_lbl(t, L) for t in lbl8]
    if plant:
        assert all((f.sum(dim=1) == 0).any() for f in lblf)
    to = lambda ts: [t.to(dev) for t in ts]
    arr = lambda ts: (C.c_void_p * S)(*[t.data_ptr() for t in ts])
    div_c = (C.c_float * S)(*divs) if nimg else None
    mk = lambda: (torch.full((S * B, H, W, Cp), float("nan"), device=dev), torch.full((S * B,), -1, dtype=torch.int32, device=dev))
    i8, l8, b8, i32, l32 = to(img8), to(lbl8), to(box8), to(imgf), to(lblf)
    out32, amax32 = mk()
    rc = lib.tsnet_op_pack_input(arr(i32) if nimg else None, arr(l32), S, B, H, W, L, nimg, Cp, int(coords), div_c, out32.data_ptr(), amax32.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    out8, amax8 = mk()
    box_out = torch.full((S * B, H, W), float("nan"), device=dev)
    rc = lib.tsnet_op_pack_input_u8(arr(i8) if nimg else None, arr(l8), arr(b8), S, B, H, W, L, nimg, Cp, int(coords), div_c,
                                    (C.c_float * 3)(*MEAN) if nimg else None, out8.data_ptr(), box_out.data_ptr(), amax8.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    oc._sync(dev)
    return {"out": (out8.cpu(), out32.cpu()), "amax": (amax8.cpu(), amax32.cpu()), "bbox": (box_out.cpu(), torch.cat([widen_box(t) for t in box8])),
            "label_channels": out8.cpu()[..., nimg:nimg + L], "label_bytes": torch.cat(lbl8)}


def check_pack(lib, dev, name):
    S, B, H, W, L, nimg, Cp, coords, divs, plant = PACK_U8_CASES[name]
    r = pack_pair(lib, dev, S, B, H, W, L, nimg, Cp, coords, divs, plant)
    for k in ("out", "amax", "bbox"):
        got, want = r[k]
        assert not torch.isnan(want.float()).any() and torch.equal(got, want), (name, k)
    if plant:                                                   # a label byte >= L: every label channel of that pixel is 0
        off = r["label_bytes"] >= L
        assert off.any() and (r["label_channels"][off] == 0).all() and (r["label_channels"][~off].sum(dim=-1) == 1).all()


def pack_u8_refusals(lib, dev):
    """bad arguments of tsnet_op_pack_input_u8: TSNET_ERR_ARG, a message, nothing written.  Returns the number walked."""
    z = torch.zeros(4096, dtype=torch.uint8, device=dev)
    outs = [torch.full((4096,), float("nan"), device=dev) for _ in range(3)]
    p, o = z.data_ptr(), [t.data_ptr() for t in outs]
    ptrs = lambda *v: (C.c_void_p * 8)(*v)
    two, div, mean = ptrs(p, p), (C.c_float * 8)(255.0, 255.0), (C.c_float * 3)(*MEAN)
    # (img, lbl, bbox, S, B, H, W, L, nimg, Cp, coords, img_div, mean, out, bbox_out, amax, stream)
    good = [two, two, two, 2, 1, 4, 4, 2, 3, 8, 1, div, mean, o[0], o[1], o[2], None]
    assert lib.tsnet_op_pack_input_u8(*good) == 0
    for t in outs:
        t.fill_(float("nan"))
    bad = [{0: None}, {1: None}, {11: None}, {12: None}, {13: None}, {14: None}, {15: None}, {0: ptrs(p, None)}, {1: ptrs(None, p)}, {2: ptrs(p, None)},
           {3: 0}, {3: 9}, {8: 1}, {9: 7}, {7: 3}, {9: 24}, {10: 0, 9: 4}, {4: 0}, {5: 0}, {7: 0}, {11: (C.c_float * 8)(255.0, 0.0)}, {8: 0, 9: 4},
           {8: 0, 7: 25, 9: 24}, {7: 256, 9: 272}]
    for change in bad:
        args = list(good)
        for i, v in change.items():
            args[i] = v
        rc = lib.tsnet_op_pack_input_u8(*args)
        msg = lib.tsnet_op_last_error().decode()
        oc._sync(dev)
        assert rc == -1 and msg, (change, rc, msg)
        assert all(torch.isnan(t).all().item() for t in outs), change
    return len(bad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# engine level: both forms of one input set
class Inputs:
    """n sources of batch B and B driving frames, compact (.c) and widened (.f): tuples (src_img, src_lbl, src_bbox, tar_lbl, tar_bbox)"""

    def __init__(self, L, n, B, H, W, seed, dev="cpu"):
        img = [_bytes(seed, f"src_img.{i}", (B, 3, H, W)) for i in range(n)]
        lbl = [_bytes(seed, f"src_lbl.{i}", (B, H, W), L) for i in range(n)]
        box = [_bytes(seed, f"src_bbox.{i}", (B, H, W), 2) for i in range(n)]
        tl, tb = _bytes(seed, "tar_lbl", (B, H, W), L), _bytes(seed, "tar_bbox", (B, H, W), 2)
        to = lambda ts: [t.to(dev) for t in ts]
        self.c = (to(img), to(lbl), to(box), tl.to(dev), tb.to(dev))
        self.f = (to([widen_img(t) for t in img]), to([widen_lbl(t, L) for t in lbl]), to([widen_box(t) for t in box]),
                  widen_lbl(tl, L).to(dev), widen_box(tb).to(dev))

    def src(self, form, ids=None, b=None):
        """(img, lbl, bbox) lists of sources `ids` in form 'c' / 'f'; b: batch element b alone (batch 1)"""
        t = self.c if form == "c" else self.f
        ids = range(len(t[0])) if ids is None else ids
        cut = (lambda x: x) if b is None else (lambda x: x[b:b + 1])
        return tuple([cut(part[i]) for i in ids] for part in t[:3])

    def tar(self, form, rows=None):
        t = self.c if form == "c" else self.f
        return (t[3], t[4]) if rows is None else (t[3][rows], t[4][rows])

    @staticmethod
    def kw(form):
        return {"mean": MEAN} if form == "c" else {}


def narrow_net(L=2, n_source=2, nb=1, seed=3, wscale=4.0, enc_blocks=2):
    """test_source_bank.py's narrow net: ngf = 8"""
    cfg = O.TSNetConfig(label_nc=L, n_blocks=nb, n_source=n_source, ngf=8, enc_blocks=enc_blocks, fuse_ngf=128)
    sd = O.synth_state_dict(cfg, seed=seed, bias_std=0.02)
    return cfg, {k: (v * wscale if k.endswith("weight") else v) for k, v in sd.items()}


def same(got, want):
    return torch.equal(got[0], want[0]) and len(got[1]) == len(want[1]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))


def sync(dev):
    oc._sync(dev)


def check_forward(eng, inp, dev):
    """one-shot forward: compact == float, rec and flows"""
    want = eng.forward(*inp.f, return_flow=True); sync(dev)
    want = (want[0].clone(), [f.clone() for f in want[1]])
    got = eng.forward(*inp.c, return_flow=True, mean=MEAN); sync(dev)
    assert torch.isfinite(want[0]).all() and want[0].abs().max() > 0
    assert same(got, want)
    return want


def check_clip_modes(eng, inp, dev, shared, combos=(("f", "c"), ("c", "f"), ("c", "c"))):
    """set_sources (+ shared) + forward_target in every combination of forms == the all-float result"""
    b = 0 if shared else None
    def run(fs, ft):
        eng.set_sources(*inp.src(fs, b=b), shared=shared, **Inputs.kw(fs))
        r = eng.forward_target(*inp.tar(ft), return_flow=True); sync(dev)
        return r[0].clone(), [f.clone() for f in r[1]]
    want = run("f", "f")
    assert torch.isfinite(want[0]).all()
    for fs, ft in combos:
        assert same(run(fs, ft), want), (shared, fs, ft)
    return want


def check_bank(eng, pool, inp_tar, dev, table, forms):
    """pool: Inputs of n sources at batch 1.  Slots j <- source j, put in the form forms[j] (runs of one form share a call); forward_bank with
    `table` on compact and on float driving frames == the all-float bank forward; then a compact put replaces slot `table[0][0]` with the last
    pool source: its readers change, the other frames keep their bits."""
    n = len(forms)
    def fill(fm):
        j = 0
        while j < n:
            k = j
            while k < n and fm[k] == fm[j]:
                k += 1
            eng.bank_put(j, *pool.src(fm[j], range(j, k)), **Inputs.kw(fm[j]))
            j = k
    def run(ft):
        r = eng.forward_bank(table, *inp_tar.tar(ft), return_flow=True); sync(dev)
        return r[0].clone(), [f.clone() for f in r[1]]
    fill(["f"] * n)
    want = run("f")
    assert torch.isfinite(want[0]).all()
    eng.set_source_divisors(None)                               # drops the bank: the mixed one starts empty
    fill(forms)
    assert same(run("f"), want) and same(run("c"), want)
    # replacement
    slot, new = table[0][0], len(pool.c[0]) - 1
    eng.bank_put(slot, *pool.src("c", [new]), **Inputs.kw("c"))
    after = run("c")
    eng.bank_put(slot, *pool.src("f", [new]))
    after_f = run("f")
    assert same(after, after_f)
    reads = [slot in row for row in table]
    assert any(reads) and not all(reads)
    for bi, rd in enumerate(reads):
        assert torch.equal(after[0][bi], want[0][bi]) != rd, bi
    return want


def golden_compact(name):
    """(meta, cfg, sd, float inputs, compact inputs) of a g10 golden -- the reference loader's own outputs as BYTES: in_src_bgr (K,H,W,3)
    resized BGR bytes, in_src_lbl / in_tar_lbl class maps, in_*_bbox packed bits.  The compact form is those bytes; the float form is
    helpers.stored_inputs' exact widening of them (the goldens hold no float tensors of their own)."""
    meta, z, cfg, sd, finp = Hh.golden_case(name)
    assert meta.get("inputs") == "stored"
    B, W = meta["B"], meta["W"]
    bits = lambda a: torch.from_numpy(np.unpackbits(a, axis=-1)[..., :W].copy())
    src_img = [torch.from_numpy(b.copy()).permute(2, 0, 1).unsqueeze(0).repeat(B, 1, 1, 1).contiguous() for b in z["in_src_bgr"]]
    src_lbl = [torch.from_numpy(l.astype(np.uint8)).unsqueeze(0).repeat(B, 1, 1).contiguous() for l in z["in_src_lbl"]]
    src_bbox = [bits(x).unsqueeze(0).repeat(B, 1, 1).contiguous() for x in z["in_src_bbox"]]
    tar_lbl = torch.stack([torch.from_numpy(l.astype(np.uint8)) for l in z["in_tar_lbl"]])
    tar_bbox = torch.stack([bits(x) for x in z["in_tar_bbox"]])
    mean = [float(v) for v in np.asarray(meta["img_mean_bgr"], dtype=np.float32)]
    return meta, cfg, sd, finp, (src_img, src_lbl, src_bbox, tar_lbl, tar_bbox), mean
