"""fp16 operands (tsnet_op_conv2d nprod = TSNET_NPROD_F16 = 16, tsnet_cfg.operand_mode = 3) against an OPERAND-EXACT reference, shared by the
CPU-emulation tier (test_fp16_operands.py) and the GPU tier (test_gpu_fp16_operands.py).

The kernels stage  rne16(t * 2^sa)  with  t = fp32(x*alpha + beta), ReLU, padding of t,  and read weights  rne16(w * 2^sw);  the power-of-two
scales come from `bound` and from max|w| (engine.cpp h2_scale_log2, restated below) and the epilogue multiplies by 2^-(sa + sw).  The
reference rounds at the same points -- q(t) = rne16(t * 2^sa) * 2^-sa, q(w) likewise -- and sums in fp64.  A product of two 11-bit numbers is
exact in fp32, so only the fp32 accumulation error is left: the error class of the bf16 operand-exact tests, held to the same REL_BF16
(1e-5 of max|reference|).  The shapes are op_cases.BF16_CASES / BF16_EXACT_CASES: an fp16 layer runs on the plan of its bf16 twin."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import op_cases as oc
from wacv23_tsnet_amd import prng

NPROD_F16 = 16          # include/tsnet_abi.h TSNET_NPROD_F16
REL = oc.REL_BF16
FAMILIES = list(oc.BF16_CASES)


def scale_log2(bound, lim):
    """engine.cpp h2_scale_log2: |x| <= bound -> |x * 2^sa| <= 2^15; |sa| <= lim (64 for an fp16-kind activation, 24 for the weights)"""
    _, e = math.frexp(float(torch.tensor(bound, dtype=torch.float32)))
    return max(-lim, min(lim, 15 - e))


def q16(t, s):
    """rne16(t * 2^s) * 2^-s in fp64 (exact: the scaled value is rounded from its fp32 form, the scalings are powers of two)"""
    scaled = torch.ldexp(t.float(), torch.tensor(s))
    assert torch.equal(torch.ldexp(scaled, torch.tensor(-s)), t.float()), "the scale left fp32's range"
    return torch.ldexp(scaled.half().double(), torch.tensor(-s))


def bound_of(t):
    return float((t.abs().max() * 1.0001).float()) + 1e-30


def conv_ref(x, w, b, al, be, relu, stride, pad, reflect, bound=None):
    """operand-exact reference of an fp16-operand convolution, fp64 NCHW; returns (reference, bound)"""
    t = oc.bf16_operand(x, al, be, relu)
    bound = bound_of(t) if bound is None else bound
    if pad:
        t = F.pad(t, (pad,) * 4, mode="reflect" if reflect else "constant")
    wmax = float(w.abs().max())
    sw = scale_log2(wmax, 24) if wmax > 0 else 0
    b64 = None if b is None else b.double()
    return F.conv2d(q16(t, scale_log2(bound, 64)), q16(w, sw), b64, stride=stride), bound


def _inputs(N, H, W, Cin, Cout, k, norm, relu, bias, seed, scale):
    x = oc._rand(seed, "x", (N, Cin, H, W)) * scale
    w = oc._rand(seed, "w", (Cout, Cin, k, k)) * (2.0 / (Cin * k * k) ** 0.5)
    b = oc._rand(seed, "b", (Cout,)) if bias else None
    relu = norm if relu is None else relu
    al = oc._rand(seed, "al", (N, Cin), 0.5, 1.5) if norm else None
    be = oc._rand(seed, "be", (N, Cin), -0.3, 0.3) if norm else None
    return x, w, b, al, be, relu


def conv_case(lib, dev, N, H, W, Cin, Cout, k, stride, pad, reflect, norm=False, relu=None, bias=True, seed=0, kernel=0, tile=0, scale=1.0,
              loosen=1.0, return_output=False):
    """tsnet_op_conv2d with the f16 kind against the operand-exact reference; inputs as op_cases.conv_bf16_case's.  loosen: factor on the
    bound (reference and call alike).  Returns max|d| relative to max|reference|."""
    x, w, b, al, be, relu = _inputs(N, H, W, Cin, Cout, k, norm, relu, bias, seed, scale)
    bound = bound_of(oc.bf16_operand(x, al, be, relu)) * loosen
    r, _ = conv_ref(x, w, b, al, be, relu, stride, pad, reflect, bound=bound)
    y = oc.run_conv_op(lib, dev, x, w, b, al, be, relu, k, stride, pad, reflect, bound, NPROD_F16, kernel, tile)
    return y if return_output else oc._rel(y, r)


def family_worst(lib, dev, family):
    """test 1: the worst error relative to max|operand-exact reference| over BF16_CASES[family] with the f16 kind"""
    worst = 0.0
    for (N, H, W, Ci, Co, k, s, p, r, kern, tile, kw) in oc.BF16_CASES[family]:
        worst = max(worst, conv_case(lib, dev, N, H, W, Ci, Co, k, s, p, r, kernel=kern, tile=tile, **kw))
    return worst


def tie_values(seed, name, shape, emin=-4, emax=4):
    """fp32 values m * 2^e with a 12-bit ODD m (2049 .. 4095): exactly half way between two fp16 neighbours whatever the power-of-two scale
    -- the kept LSB (bit 1 of m) even and odd in equal shares -- mixed with their one-fp32-ulp neighbours and random mantissas, both signs.
    emin .. emax keep the scaled values inside fp16's normal range next to the tensor's maximum."""
    n = 1
    for s in shape:
        n *= s
    u = lambda tag: prng.uniform01(seed, name + tag, (n,)).double()
    exp = (u("_e") * (emax - emin + 1)).floor().long().clamp(max=emax - emin) + emin + 127
    m12 = ((u("_m") * 1024).floor().long().clamp(max=1023) << 1) | 1 | 2048                  # 12 bits, leading and last bit set
    mant = (m12 - 2048) << 12                                                               # below the implicit bit: 11 bits, then 12 zeros
    delta = torch.tensor([0, 0, 0, 0, -1, 1, 0, 0])[(u("_k") * 8).floor().long().clamp(max=7)]
    rnd = (u("_r") * (1 << 23)).floor().long().clamp(max=(1 << 23) - 1)
    mant = torch.where(u("_x") < 0.125, rnd, mant + delta)
    sgn = (u("_s") < 0.5).long() << 31
    bits = sgn | (exp << 23) | mant
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.view(torch.float32).view(shape).clone()


def delta_case(lib, dev, N, H, W, Cin, Cout, k, stride, pad, reflect, transform=None, relu=False, seed=0, kernel=0, tile=0):
    """BIT-EXACT activation rounding: op_cases._delta_weights (1.0 is exact at any weight scale) on inputs full of fp16 ties, no bias: every
    output is q(t) of one pixel.  transform: None, "pow2" (alpha = 2^j, beta = 0: the tie survives the fmaf) or "rand".  Returns (y, ref)."""
    x = tie_values(seed, "xt", (N, Cin, H, W))
    al = be = None
    if transform == "pow2":
        al = torch.exp2((prng.uniform01(seed, "alj", (N, Cin)) * 7).floor() - 3)
        be = torch.zeros(N, Cin)
    elif transform == "rand":
        al = oc._rand(seed, "al", (N, Cin), 0.5, 1.5)
        be = oc._rand(seed, "be", (N, Cin), -0.3, 0.3)
    w = oc._delta_weights(Cout, Cin, k)
    ref, bound = conv_ref(x, w, None, al, be, relu, stride, pad, reflect)
    y = oc.run_conv_op(lib, dev, x, w, None, al, be, relu, k, stride, pad, reflect, bound, NPROD_F16, kernel, tile)
    return y, ref.float()


def weight_case(lib, dev, Cin, Cout, k, stride, pad, reflect, seed=0, kernel=0, tile=0):
    """BIT-EXACT weight rounding: op_cases.conv_bf16_weight_case's one-hot inputs (1.0 at bound 1.0001: 2^14 after the scale, exact) on
    weights full of fp16 ties: every output is q(w) of one weight, or zero.  Returns (y, ref)."""
    sp = k + stride
    H, W = 16 * stride, 32 * stride
    while True:
        pos = [(r, c) for r in range(pad + 1, H - pad - 1, sp) for c in range(pad + 1, W - pad - 1, sp)]
        if len(pos) >= Cin:
            break
        H, W = (2 * H, W) if H < W else (H, 2 * W)
    x = torch.zeros(1, Cin, H, W)
    perm = torch.argsort(prng.uniform01(seed, "perm", (len(pos),)))
    for c in range(Cin):
        r, q = pos[int(perm[c])]
        x[0, c, r, q] = 1.0
    w = tie_values(seed, "wt", (Cout, Cin, k, k), -8, 2)
    ref, bound = conv_ref(x, w, None, None, None, False, stride, pad, reflect)
    y = oc.run_conv_op(lib, dev, x, w, None, None, None, False, k, stride, pad, reflect, bound, NPROD_F16, kernel, tile)
    return y, ref.float()


def exact_mismatches(lib, dev, family):
    """test 2: BF16_EXACT_CASES[family] with the f16 kind through the delta filter on ties (no transform; alpha = 2^j with and without ReLU;
    one random alpha / beta) and the one-hot input on tied weights.  Returns the cases whose bits differ (empty: all exact)."""
    bad = []
    for i, (N, H, W, Ci, Co, k, s, p, r, kern, tile) in enumerate(oc.BF16_EXACT_CASES[family]):
        stem = k == 7                                                  # the stems take no transform
        for tr, relu in ((None, False),) + (() if stem else (("pow2", False), ("pow2", True), ("rand", True))):
            y, ref = delta_case(lib, dev, N, H, W, Ci, Co, k, s, p, r, transform=tr, relu=relu, seed=i, kernel=kern, tile=tile)
            if not torch.equal(y, ref):
                bad.append(("delta", tr, relu, (N, H, W, Ci, Co, k, s, tile), int((y != ref).sum())))
        y, ref = weight_case(lib, dev, Ci, Co, k, s, p, r, seed=i, kernel=kern, tile=tile)
        if not torch.equal(y, ref):
            bad.append(("weights", (Ci, Co, k, s, tile), int((y != ref).sum())))
    return bad


def covariance_problems(lib, dev, family):
    """test 3 on the family's first exact case, no bias and no transform: op(x 2^j, bound 2^j) == 2^j op(x, bound) bit for bit for j = +-40 (the
    scale follows the bound; nothing in between has a range of its own); a bound loosened by 2^8 stays inside REL; an operand exactly AT the
    bound (2^15 after the scale when the bound is a power of two's upper neighbour... here: the bound itself is a value of x) comes out
    finite and exact.  Returns a list of problems (empty: none)."""
    N, H, W, Ci, Co, k, s, p, r, kern, tile = oc.BF16_EXACT_CASES[family][0]
    bad = []
    x, w, _, _, _, _ = _inputs(N, H, W, Ci, Co, k, False, False, False, 11, 1.0)
    bound = bound_of(x)
    run = lambda xx, bb, ww=w: oc.run_conv_op(lib, dev, xx, ww, None, None, None, False, k, s, p, r, bb, NPROD_F16, kern, tile)
    y0 = run(x, bound)
    for j in (40, -40):
        yj = run(torch.ldexp(x, torch.tensor(j)), float(torch.ldexp(torch.tensor(bound), torch.tensor(j))))
        if not torch.equal(yj, torch.ldexp(y0, torch.tensor(j))):
            bad.append(("covariance", j, int((yj != torch.ldexp(y0, torch.tensor(j))).sum())))
    loose = conv_case(lib, dev, N, H, W, Ci, Co, k, s, p, r, bias=False, seed=11, kernel=kern, tile=tile, loosen=256.0)
    if not loose < REL:
        bad.append(("loosened bound", loose))
    # every pixel of channel 0 holds +-bound (1.75: scaled to 1.75 * 2^14, an fp16 number), the other channels ties below it; delta filter
    xb = tie_values(12, "xb", (N, Ci, H, W), -6, -1)
    xb[:, 0] = torch.where(prng.uniform01(12, "sg", (N, H, W)) < 0.5, -1.75, 1.75)
    wd = oc._delta_weights(Co, Ci, k)
    ref, _ = conv_ref(xb, wd, None, None, None, False, s, p, r, bound=1.75)
    yb = run(xb, 1.75, wd)
    if not (torch.isfinite(yb).all() and torch.equal(yb, ref.float()) and float(yb[:, 0].abs().max()) == 1.75):
        bad.append(("operand at the bound", int((yb != ref.float()).sum())))
    return bad


def cat_worst(lib, dev):
    """test 4: the three shapes of test_emu_ops.py::test_bf16_conv_cat (the concat formed on load: 1 x 1 on conv_g64, 3 x 3 on conv_h2r, with and
    without a shared second tensor) with the f16 kind against the operand-exact reference"""
    worst = 0.0
    for (N, H, W, C1, C2, Co, k, shared) in ((2, 8, 8, 64, 64, 128, 1, False), (2, 8, 8, 128, 64, 256, 1, True), (3, 5, 6, 16, 48, 24, 3, True)):
        x = oc._rand(0, "x", (N, C1, H, W))
        x2 = oc._rand(0, "x2", (1 if shared else N, C2, H, W)) * 3.0
        w = oc._rand(0, "w", (Co, C1 + C2, k, k)) * (2.0 / ((C1 + C2) * k * k) ** 0.5)
        b = oc._rand(0, "b", (Co,))
        xin = torch.cat([x, x2.expand(N, -1, -1, -1)], dim=1)
        r, bound = conv_ref(xin, w, b, None, None, False, 1, k // 2, False)
        worst = max(worst, oc._rel(oc.run_cat_op(lib, dev, x, x2, w, b, k, NPROD_F16, bound), r))
    return worst


# test 5: the one-group tile codes of a kernel on one layer (the tiles BF16_CASES runs it on): identical bits
SAME_BITS = {
    "H2": ((2, 8, 32, 48, 128, 3, 1, 1, True, 2), (0, 32, 64, 128, 2128, 3128)),
    "H2D": ((2, 8, 64, 16, 128, 3, 2, 1, False, 2), (0, 64, 128, 2128)),
    "G64": ((1, 16, 16, 64, 192, 3, 2, 1, False, 1), (3064, 3128)),
}


def tile_outputs(lib, dev, family):
    (N, H, W, Ci, Co, k, s, p, r, kern), tiles = SAME_BITS[family]
    return [conv_case(lib, dev, N, H, W, Ci, Co, k, s, p, r, norm=True, kernel=kern, tile=t, return_output=True) for t in tiles]


def refusals(lib, dev):
    """test 6 (operator part): kernel = 3, tile 12128 and an unknown nprod return TSNET_ERR_ARG with a message and leave the output alone.
    Returns the messages."""
    msgs = []
    for (shape, nprod, kernel, tile) in (((1, 4, 32, 32, 64, 3, 1, 1, True), NPROD_F16, 3, 0),
                                          ((1, 8, 64, 16, 128, 3, 2, 1, False), NPROD_F16, 2, 12128),
                                          ((1, 4, 32, 32, 64, 3, 1, 1, True), 2, 0, 0),
                                          ((1, 4, 32, 32, 64, 3, 1, 1, True), 17, 0, 0)):
        N, H, W, Ci, Co, k, s, p, r = shape
        x, w = torch.zeros(N, H, W, Ci, device=dev), torch.zeros(Co, Ci, k, k, device=dev)
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        y = torch.full((N, Ho, Wo, Co), float("nan"), device=dev)
        rc = lib.tsnet_op_conv2d(x.data_ptr(), N, H, W, Ci, w.data_ptr(), None, Co, k, s, p, int(r), None, None, 0, 1.0, nprod, kernel, tile,
                                 y.data_ptr(), None)
        oc._sync(dev)
        msg = lib.tsnet_op_last_error().decode()
        assert rc == oc.TSNET_ERR_ARG and msg, (nprod, kernel, tile, rc, msg)
        assert torch.isnan(y).all()
        if nprod not in (1, 3, 4, NPROD_F16):       # the entry's own check, ahead of the layer's packing and of the planner's "conv: ..." refusal
            assert msg.startswith("conv2d op: nprod"), (nprod, msg)
        msgs.append(msg)
    return msgs


def mode_refusals(lib):
    """test 6 (engine part): tsnet_create takes operand_mode 3 and refuses 4 and -1 with a message that lists the modes; there is no
    "fp16s" (storage stays fp32): TSNetEngine and TSNet raise ValueError and name 'fp16' among the modes they take"""
    import ctypes as C
    import pytest
    from wacv23_tsnet_amd import _lib
    from wacv23_tsnet_amd.engine import TSNetEngine
    from wacv23_tsnet_amd.model import TSNet
    cfg = _lib.TsnetCfg()
    cfg.label_nc, cfg.n_blocks, cfg.n_downsampling, cfg.n_source, cfg.ngf, cfg.enc_blocks, cfg.addcoords = 2, 0, 3, 1, 8, 0, 1
    cfg.height, cfg.width, cfg.max_batch = 32, 32, 1
    for mode, ok in ((3, True), (4, False), (-1, False)):
        cfg.operand_mode = mode
        h = C.c_void_p()
        rc = lib.tsnet_create(C.byref(cfg), C.byref(h))
        assert (rc == 0) == ok, (mode, rc)
        if ok:
            lib.tsnet_destroy(h)
        else:
            assert "operand_mode" in lib.tsnet_last_error(None).decode() and "3 (fp16 operands)" in lib.tsnet_last_error(None).decode()
    with pytest.raises(ValueError, match="'fp16'"):
        TSNetEngine(label_nc=2, n_blocks=0, height=32, width=32, operands="fp16s", lib=lib)
    with pytest.raises(ValueError, match="'fp16'"):
        TSNet(is_train=False, label_nc=2, n_downsampling=3, operands="fp16s")
    assert TSNet(is_train=False, label_nc=2, n_downsampling=3, operands="fp16").operands == "fp16"


# ---- the whole forward in the fp16-operand mode (TSNetEngine(operands="fp16")) ----------------------------------------------------------
def r16(t):
    """oracle.tsnet_oracle._r for the fp16-operand mode: scale by a power of two to <= 2^15 (here from the tensor's own maximum; the engine's
    a-priori bounds are looser, which costs nothing at these magnitudes), round to fp16, unscale.  Identity outside a rounding forward."""
    from oracle import tsnet_oracle as O
    if not O._ROUND_BF16:
        return t
    m = float(t.abs().max())
    if not m > 0:
        return t
    s = torch.tensor(15 - math.frexp(m)[1])
    return torch.ldexp(torch.ldexp(t, s).half().to(t.dtype), -s)


def _stage_dists(eng, stages, K, B, dev):
    import helpers as Hh
    rep = Hh.stage_report(eng, stages, K, B, dev)
    return dict(src_fea=max(rep[k] for k in rep if k.startswith("src_fea")), tar_fea=rep["tar_fea"], sg=rep["sg"])


def forward_report(monkeypatch, cfg, sd, inp, B, H, W, dev, lib=None):
    """One (weights, inputs) draw through the engine in fp16 AND bf16 mode and through the oracle with fp16 rounding (O._r = r16: every
    operand the bf16 oracle rounds, nothing else), bf16 rounding and none.  Returns
      a: src_fea / tar_fea / sg max distances and decoder_on_engine_features (max, mean) of the fp16 engine against the fp16 oracle,
      b: {stage: (fp16 engine vs fp32 oracle, bf16 engine vs fp32 oracle, fp16 oracle vs fp32 oracle, bf16 oracle vs fp32 oracle)},
      c: (flow_on_engine_features, pg_on_engine_features),  finite: every stage and the output are finite;  rec: the fp16 engine's output"""
    import helpers as Hh
    from oracle import tsnet_oracle as O
    K = cfg.n_source
    ref32 = O.tsnet_forward(sd, cfg, *inp, want_stages=True)
    refb = O.tsnet_forward(sd, cfg, *inp, round_operands="bf16", want_stages=True)
    eb = Hh.make_engine(cfg, sd, H, W, B, dev, lib=lib, operands="bf16")
    Hh.run_engine(eb, inp, dev, return_flow=False)
    db = _stage_dists(eb, ref32["stages"], K, B, dev)
    eb.close()
    eng = Hh.make_engine(cfg, sd, H, W, B, dev, lib=lib, operands="fp16")
    rec, flows = Hh.run_engine(eng, inp, dev)
    with monkeypatch.context() as mp:
        mp.setattr(O, "_r", r16)
        ref16 = O.tsnet_forward(sd, cfg, *inp, round_operands="bf16", want_stages=True)
        pg, sg = Hh.nhwc_to_nchw(eng.stage("pg", dev).cpu()), Hh.nhwc_to_nchw(eng.stage("sg", dev).cpu())
        with O.bf16_operands():
            dec, _ = O.decoder(pg, sg, sd, cfg)
    a = _stage_dists(eng, ref16["stages"], K, B, dev)
    a["decoder_on_engine_features"] = (rec - dec).abs().max().item()
    a["decoder_on_engine_features_mean"] = (rec - dec).abs().mean().item()
    d16 = _stage_dists(eng, ref32["stages"], K, B, dev)
    odist = lambda r, k: max((x - y).abs().max().item() for x, y in zip(r["stages"][k], ref32["stages"][k])) if k == "src_fea" \
        else (r["stages"][k] - ref32["stages"][k]).abs().max().item()
    b = {k: (d16[k], db[k], odist(ref16, k), odist(refb, k)) for k in ("src_fea", "tar_fea", "sg")}
    c = Hh.transformation_on_engine_features(eng, cfg, inp, flows, B, dev)
    names = ["src_fea", "tar_fea", "pg", "sg", "dec_map"]
    finite = bool(torch.isfinite(rec).all()) and all(bool(torch.isfinite(eng.stage(k, dev)).all()) for k in names)
    out = dict(a=a, b=b, c=c, finite=finite, rec=rec,
               mean_vs_fp32=((rec - ref32["rec_tar_img"]).abs().mean().item(), (refb["rec_tar_img"] - ref32["rec_tar_img"]).abs().mean().item()))
    return out, eng


def report_line(tag, r):
    return (f"[{tag}] a: " + " ".join(f"{k}={v:.3e}" for k, v in r["a"].items()) + " | b (fp16 eng, bf16 eng, fp16 oracle, bf16 oracle vs fp32): " +
            " ".join(f"{k}={v[0]:.3e}/{v[1]:.3e}/{v[2]:.3e}/{v[3]:.3e}" for k, v in r["b"].items()) +
            f" | c: flow={r['c'][0]:.3e} pg={r['c'][1]:.3e} | finite={r['finite']} | image mean vs fp32 (fp16 engine, bf16 oracle)={r['mean_vs_fp32'][0]:.3e}/{r['mean_vs_fp32'][1]:.3e}")


def check_forward(tag, r, gates):
    """the assertions of one forward case: (a) gates against the fp16 oracle, (b) <= 1/4 of the bf16 engine's distance to the fp32 oracle on
    the same draw, (c) the transformation branch on the engine's features at the constants of tests/test_gpu_forward.py::_gate (flows 1e-4,
    pg 4e-3), (d) finite"""
    print(report_line(tag, r))
    for k, lim in gates.items():
        assert r["a"][k] <= lim, (tag, k, r["a"][k], lim)
    for k, (d16, db, o16, ob) in r["b"].items():
        assert 6.0 * o16 <= ob, (tag, k, "the reference alone gives less than 6x on this draw: pick another", o16, ob)
        assert 4.0 * d16 <= db, (tag, k, d16, db)
    assert r["c"][0] <= 1e-4 and r["c"][1] <= 4e-3, (tag, r["c"])
    assert r["finite"], tag
