"""Operator-level parity cases, shared by the CPU-emulation tier (tests/test_emu_*.py) and the GPU
tier (tests/test_gpu_ops.py).  Every case calls through the C ABI (tsnet_op_*) and compares with
plain PyTorch CPU fp32 ops -- the same ATen ops the reference's modules resolve to."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from wacv23_tsnet_amd import prng


def _rand(seed, name, shape, lo=-1.0, hi=1.0):
    return prng.uniform01(seed, name, shape) * (hi - lo) + lo


def _p(t):
    return None if t is None else t.data_ptr()


def _sync(dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def conv_case(lib, dev, N, H, W, Cin, Cout, k, stride, pad, reflect, norm=False, bias=True, seed=0, nprod=3, kernel=0, tile=0, scale=1.0,
              relu=None, return_output=False):
    """nn.Conv2d (+ReflectionPad2d / zero pad), optionally on relu(x*alpha+beta) -- the consumer side of nn.InstanceNorm2d + nn.ReLU --
    vs tsnet_op_conv2d (fp16 x 2 operands, the transform fused into the operand staging).  kernel: 0 = the forward's own choice for the
    layer, 1 = general implicit GEMM, 2 = patch kernel.  Returns max|d| relative to max|fp64 reference| (or the NHWC output)."""
    x = _rand(seed, "x", (N, Cin, H, W)) * scale
    w = _rand(seed, "w", (Cout, Cin, k, k)) * (2.0 / (Cin * k * k) ** 0.5)
    b = _rand(seed, "b", (Cout,)) if bias else None
    xin, al, be = x, None, None
    relu = norm if relu is None else relu
    if norm:
        al = _rand(seed, "al", (N, Cin), 0.5, 1.5)
        be = _rand(seed, "be", (N, Cin), -0.3, 0.3)
        xin = x * al[:, :, None, None] + be[:, :, None, None]
    if relu:
        xin = F.relu(xin)
    b64 = None if b is None else b.double()
    if reflect:
        ref = F.conv2d(F.pad(xin.double(), (pad,) * 4, mode="reflect"), w.double(), b64, stride=stride)
    else:
        ref = F.conv2d(xin.double(), w.double(), b64, stride=stride, padding=pad)
    bound = float(xin.abs().max()) * 1.0001 + 1e-30
    Ho, Wo = ref.shape[2:]
    xd = nhwc(x).to(dev)
    y = torch.full((N, Ho, Wo, Cout), float("nan"), device=dev)
    ald = al.contiguous().to(dev) if norm else None
    bed = be.contiguous().to(dev) if norm else None
    wd, bd = w.to(dev), (b.to(dev) if bias else None)
    rc = lib.tsnet_op_conv2d(xd.data_ptr(), N, H, W, Cin, wd.data_ptr(), _p(bd), Cout, k, stride, pad, int(reflect),
                             _p(ald), _p(bed), int(relu), bound, nprod, kernel, tile, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    if return_output:
        return y.cpu()
    return ((nchw(y.cpu()).double() - ref).abs().max() / ref.abs().max()).item()


def conv_h2_case(lib, dev, N, H, W, Cin, Cout, reflect, norm=False, bias=True, nprod=3, tile_n=0, seed=0, scale=1.0, return_output=False):
    """3x3 / stride 1 / pad 1 on the PATCH kernel (conv_h2.hpp h2_tile); tile_n: 0, 32, 64, 128 (4-row tiles), 2128 (2 rows x 128), 3128 (bf16 operands: 4 x 128, four waves side by side), 20032 / 20064 (two K groups, 4 x 32 / 4 x 64)."""
    return conv_case(lib, dev, N, H, W, Cin, Cout, 3, 1, 1, reflect, norm=norm, bias=bias, seed=seed, nprod=nprod, kernel=2, tile=tile_n,
                     scale=scale, return_output=return_output)


def conv_w1_case(lib, dev, N, H, W, Cin, Cout, reflect, norm=False, bias=True, nprod=3, seed=0, scale=1.0, relu=None, return_output=False, chunk=0):
    """3x3 / stride 1 / pad 1 in the Winograd F(2,3)-along-x form (conv_w1.hpp; kernel = 3): same contract as conv_h2_case.  chunk: tiles per
    workgroup (1, 2, 3; 0 = the launcher's choice)"""
    return conv_case(lib, dev, N, H, W, Cin, Cout, 3, 1, 1, reflect, norm=norm, bias=bias, seed=seed, nprod=nprod, kernel=3, tile=chunk, scale=scale,
                     relu=relu, return_output=return_output)


def conv_h2r_case(lib, dev, N, H, W, Cin, Cout, ksize, norm=False, bias=True, seed=0, kernel=0, tile=0, return_output=False):
    """the encoder's stem (7x7, reflection pad 3) and downsampling (3x3, stride 2, zero pad 1) convolutions; kernel as conv_case."""
    if ksize == 7:
        return conv_case(lib, dev, N, H, W, Cin, Cout, 7, 1, 3, True, norm=norm, bias=bias, seed=seed, kernel=kernel, tile=tile, return_output=return_output)
    return conv_case(lib, dev, N, H, W, Cin, Cout, 3, 2, 1, False, norm=norm, bias=bias, seed=seed, kernel=kernel, tile=tile, return_output=return_output)


def conv_cat_case(lib, dev, N, H, W, C1, C2, Cout, k=1, seed=0, shared=False, nprod=3, ref="fp64"):
    """convolution of torch.cat((x, x2), dim=1) with the concat formed on load (dec.map_conv on cat(pg, sg), TSNet.py:163); `shared`: x2 has
    one image that every image of x is concatenated with (image index n % x2_nmod).  nprod as conv_case's (the forward's bf16 modes run
    this layer with 1); ref: "fp64" (the unrounded convolution) or "bf16" (the operand-exact reference, bf16_conv_ref)."""
    x = _rand(seed, "x", (N, C1, H, W))
    x2 = _rand(seed, "x2", (1 if shared else N, C2, H, W)) * 3.0
    w = _rand(seed, "w", (Cout, C1 + C2, k, k)) * (2.0 / ((C1 + C2) * k * k) ** 0.5)
    b = _rand(seed, "b", (Cout,))
    xin = torch.cat([x, x2.expand(N, -1, -1, -1)], dim=1)
    if ref == "bf16":
        r = bf16_conv_ref(xin, w, b, None, None, False, 1, k // 2, False)
    else:
        r = F.conv2d(xin.double(), w.double(), b.double(), padding=k // 2)
    y = run_cat_op(lib, dev, x, x2, w, b, k, nprod, float(xin.abs().max()) * 1.0001)
    return ((y.double() - r).abs().max() / r.abs().max()).item()


def head_case(lib, dev, N, H, W, C, norm=True, composite=False, seed=0, rows=0, return_output=False):
    """the decoder's RGB head: ReflectionPad2d(3) + Conv2d(C -> 3, 7x7) + bias + Tanh on relu(IN(x)) (TSNet.py:151-152), optional pose
    composite (TSNet_pose.py:416-417) vs tsnet_op_head.  rows: tile rows of head_conv3 to force (8, 16, 32; 0 = the launcher's choice).
    Returns max|d| (or the output)."""
    x = _rand(seed, "x", (N, C, H, W))
    w = _rand(seed, "w", (3, C, 7, 7)) * (2.0 / (C * 49) ** 0.5)
    b = _rand(seed, "b", (3,))
    xin, al, be = x, None, None
    if norm:
        al = _rand(seed, "al", (N, C), 0.5, 1.5)
        be = _rand(seed, "be", (N, C), -0.3, 0.3)
        xin = F.relu(x * al[:, :, None, None] + be[:, :, None, None])
    ref = torch.tanh(F.conv2d(F.pad(xin, (3,) * 4, mode="reflect"), w, b))
    bg = [0.25, -0.5, 0.75]
    if composite:
        for c in range(3):
            ref[:, c, :, :64] = bg[c]
            ref[:, c, :, 192:] = bg[c]
    import ctypes
    y = torch.full((N, 3, H, W), float("nan"), device=dev)
    xd, wd, bd = nhwc(x).to(dev), w.to(dev), b.to(dev)
    ald = al.contiguous().to(dev) if norm else None
    bed = be.contiguous().to(dev) if norm else None
    rc = lib.tsnet_op_head(xd.data_ptr(), N, H, W, C, _p(ald), _p(bed), wd.data_ptr(), bd.data_ptr(), int(composite) | (rows << 8), (ctypes.c_float * 3)(*bg),
                           y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    if return_output:
        return y.cpu()
    return (y.cpu() - ref).abs().max().item()


def instnorm_case(lib, dev, N, H, W, C, relu, resid, seed=0, offset=0.0):
    """InstanceNorm2d(eps=1e-5, biased var) [+ReLU] [+residual] vs stats + norm_act kernels."""
    x = _rand(seed, "x", (N, C, H, W), -2, 2) + offset
    ref = F.instance_norm(x, eps=1e-5)
    if relu:
        ref = F.relu(ref)
    r = _rand(seed, "r", (N, C, H, W)) if resid else None
    if resid:
        ref = r + ref
    xd = nhwc(x).to(dev)
    al = torch.empty(N * C, device=dev)
    be = torch.empty(N * C, device=dev)
    rc = lib.tsnet_op_instnorm_stats(xd.data_ptr(), N, H * W, C, al.data_ptr(), be.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    y = torch.empty_like(xd)
    rd = nhwc(r).to(dev) if resid else None
    rc = lib.tsnet_op_norm_act(xd.data_ptr(), al.data_ptr(), be.data_ptr(), int(relu), _p(rd), N, H * W, C, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    return (nchw(y.cpu()) - ref).abs().max().item()


def upsample_case(lib, dev, N, H, W, C, norm, seed=0):
    """nn.Upsample(x2, bilinear, align_corners=False) [after IN+ReLU] vs tsnet_op_upsample2x."""
    x = _rand(seed, "x", (N, C, H, W), -2, 2)
    xin, al, be = x, None, None
    if norm:
        al = _rand(seed, "al", (N, C), 0.5, 1.5)
        be = _rand(seed, "be", (N, C), -0.3, 0.3)
        xin = F.relu(x * al[:, :, None, None] + be[:, :, None, None])
    ref = F.interpolate(xin, scale_factor=2, mode="bilinear", align_corners=False)
    xd = nhwc(x).to(dev)
    y = torch.empty((N, 2 * H, 2 * W, C), device=dev)
    ald = al.contiguous().to(dev) if norm else None
    bed = be.contiguous().to(dev) if norm else None
    rc = lib.tsnet_op_upsample2x(xd.data_ptr(), _p(ald), _p(bed), int(norm), N, H, W, C, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    return (nchw(y.cpu()) - ref).abs().max().item()


def flow_case(lib, dev, B, h, w, C, mask_mode="bernoulli", seed=0, spike=False):
    """Transformation branch up to the flow (TSNet.py:319-365) + grid_sample (:366) vs the oracle's
    transformation_branch.  spike=True plants one dominant source per target (forces online-softmax
    rescales in every tile order).  Returns (max|d flow|, max|d warped|)."""
    from oracle import tsnet_oracle as O
    H, W = h * 8, w * 8
    tar = F.relu(_rand(seed, "tar", (B, C, h, w), -1, 1))
    src = _rand(seed, "src", (B, C, h, w), -1, 1) * 3
    if spike:
        P = h * w
        perm = torch.arange(P - 1, -1, -1)
        srcf = src.view(B, C, P)
        tarf = tar.view(B, C, P)
        srcf[:, :, perm] = srcf[:, :, perm] * 0.2 + 4.0 * tarf    # source perm[t] ~ aligned with target t
    if mask_mode == "ones":
        mt, ms = torch.ones(B, H, W), torch.ones(B, H, W)
    elif mask_mode == "zeros":
        mt, ms = torch.zeros(B, H, W), torch.zeros(B, H, W)
    elif mask_mode == "soft":
        mt, ms = prng.uniform01(seed, "mt", (B, H, W)), prng.uniform01(seed, "ms", (B, H, W))
    else:
        mt, ms = prng.bernoulli(seed, "mt", (B, H, W)), prng.bernoulli(seed, "ms", (B, H, W))
    warped_ref, flow_ref = O.transformation_branch(tar, src, mt.unsqueeze(1), ms.unsqueeze(1))
    tard, srcd = nhwc(tar).to(dev), nhwc(src).to(dev)
    mtd, msd = mt.to(dev), ms.to(dev)
    flow = torch.empty((B, h, w, 2), device=dev)
    rc = lib.tsnet_op_flow(tard.data_ptr(), srcd.data_ptr(), mtd.data_ptr(), msd.data_ptr(), B, h, w, C, H, W, flow.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    # a second run must give the same bits (the packed-fp32 build of the large-map kernel did not: csrc/flow_persist.hpp; both flow kernels
    # are now compiled without the SLP vectorizer and both are held to this)
    flow2 = torch.full((B, h, w, 2), float("nan"), device=dev)
    rc = lib.tsnet_op_flow(tard.data_ptr(), srcd.data_ptr(), mtd.data_ptr(), msd.data_ptr(), B, h, w, C, H, W, flow2.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    assert torch.equal(flow, flow2)
    warped = torch.empty((B, h, w, C), device=dev)
    rc = lib.tsnet_op_warp(srcd.data_ptr(), flow.data_ptr(), B, h, w, C, warped.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    return (flow.cpu() - flow_ref).abs().max().item(), (nchw(warped.cpu()) - warped_ref).abs().max().item()


def flow_k_case(lib, dev, B, K, h, w, C, mask_mode="bernoulli", seed=0, spike=True):
    """K sources per driving frame (the model's loop, TSNet.py:336-366) through tsnet_op_flow_k vs the oracle's transformation_branch run
    once per source.  Maps of >= 2048 positions take flow_kernel_p (csrc/flow_persist.hpp): a workgroup keeps its target tile for the K
    sources, G workgroups share a (source, target tile) and the last to arrive merges their partial softmax states.  Both calls start from
    fresh scratch memory: a partial state read before it is visible would show as a difference.  Returns max|d flow| over all sources."""
    from oracle import tsnet_oracle as O
    H, W = h * 8, w * 8
    P = h * w
    tar = F.relu(_rand(seed, "tar", (B, C, h, w), -1, 1))
    mt = prng.bernoulli(seed, "mt", (B, H, W)) if mask_mode == "bernoulli" else prng.uniform01(seed, "mt", (B, H, W))
    srcs, mss, refs = [], [], []
    for k in range(K):
        src = _rand(seed + 1 + k, "src", (B, C, h, w), -1, 1) * 3
        if spike:                                                         # one dominant source per target, somewhere else for every k
            perm = (torch.arange(P) * (2 * k + 3) + 7 * k) % P if P % (2 * k + 3) else torch.arange(P - 1, -1, -1)
            srcf, tarf = src.view(B, C, P), tar.view(B, C, P)
            srcf[:, :, perm] = srcf[:, :, perm] * 0.2 + 4.0 * tarf
        ms = prng.bernoulli(seed + 1 + k, "ms", (B, H, W)) if mask_mode == "bernoulli" else prng.uniform01(seed + 1 + k, "ms", (B, H, W))
        _, flow_ref = O.transformation_branch(tar, src, mt.unsqueeze(1), ms.unsqueeze(1))
        srcs.append(nhwc(src)); mss.append(ms); refs.append(flow_ref)
    tard, srcd = nhwc(tar).to(dev), torch.cat(srcs, 0).contiguous().to(dev)
    mtd, msd = mt.to(dev), torch.cat(mss, 0).contiguous().to(dev)
    flow = torch.empty((K * B, h, w, 2), device=dev)
    rc = lib.tsnet_op_flow_k(tard.data_ptr(), srcd.data_ptr(), mtd.data_ptr(), msd.data_ptr(), B, K, h, w, C, H, W, flow.data_ptr(), 0, 1, None, None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    # a second call must give the same bits (arrival counters back at zero, merge order fixed)
    flow2 = torch.empty_like(flow)
    rc = lib.tsnet_op_flow_k(tard.data_ptr(), srcd.data_ptr(), mtd.data_ptr(), msd.data_ptr(), B, K, h, w, C, H, W, flow2.data_ptr(), 0, 2, None, None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    assert torch.equal(flow, flow2)
    return (flow.cpu() - torch.cat(refs, 0)).abs().max().item()


def flow_k_batch_independence_case(lib, dev, batches, K, h, w, C, seed=0):
    """flow_kernel_p splits every source image into a number of slices that depends on the MAP alone and merges them in slice order; how
    many workgroups share a target tile (G: 4, 2, 1 as the batch grows) only decides who computes which slice.  The flows of the first
    batch element must therefore be the same BITS in every batch size (the tree used to be built on G).  Returns the list of
    flows of element 0, one per batch size."""
    H, W, P = h * 8, w * 8, h * w
    Bmax = max(batches)
    tar = F.relu(_rand(seed, "tar", (Bmax, C, h, w), -1, 1))
    mt = prng.bernoulli(seed, "mt", (Bmax, H, W))
    srcs = [_rand(seed + 1 + k, "src", (Bmax, C, h, w), -1, 1) * 3 for k in range(K)]
    for k in range(K):
        perm = (torch.arange(P) * (2 * k + 3) + 7 * k) % P if P % (2 * k + 3) else torch.arange(P - 1, -1, -1)
        srcs[k].view(Bmax, C, P)[:, :, perm] = srcs[k].view(Bmax, C, P)[:, :, perm] * 0.2 + 4.0 * tar.view(Bmax, C, P)
    mss = [prng.bernoulli(seed + 1 + k, "ms", (Bmax, H, W)) for k in range(K)]
    out = []
    for B in batches:
        tard = nhwc(tar[:B]).to(dev)
        srcd = torch.cat([nhwc(s[:B]) for s in srcs], 0).contiguous().to(dev)
        mtd, msd = mt[:B].contiguous().to(dev), torch.cat([m[:B] for m in mss], 0).contiguous().to(dev)
        flow = torch.empty((K * B, h, w, 2), device=dev)
        rc = lib.tsnet_op_flow_k(tard.data_ptr(), srcd.data_ptr(), mtd.data_ptr(), msd.data_ptr(), B, K, h, w, C, H, W, flow.data_ptr(), 0, 1, None, None)
        assert rc == 0, lib.tsnet_op_last_error().decode()
        _sync(dev)
        out.append(flow.cpu().view(K, B, h, w, 2)[:, 0].clone())
    return out


def warp_case(lib, dev, B, h, w, C, seed=0):
    """F.grid_sample(bilinear, zeros, align_corners=False) with flows that leave [-1,1] (zero padding
    and border blending exercised) vs tsnet_op_warp."""
    src = _rand(seed, "src", (B, C, h, w), -2, 2)
    flow = _rand(seed, "flow", (B, h, w, 2), -1.3, 1.3)
    ref = F.grid_sample(src, flow, align_corners=False)
    srcd, fd = nhwc(src).to(dev), flow.to(dev)
    out = torch.empty((B, h, w, C), device=dev)
    rc = lib.tsnet_op_warp(srcd.data_ptr(), fd.data_ptr(), B, h, w, C, out.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    return (nchw(out.cpu()) - ref).abs().max().item()


def conv_split_worstcase_case(lib, dev, N, H, W, Cin, Cout, tiers=(-12, -18, -24), weights_too=True, corner=False, seed=0, kernel=2):
    """kernel: 2 = the direct patch kernel (conv_h2), 3 = the Winograd-along-x kernel (conv_w1: the forward's ResnetBlock / FuseNet layers --
    one bit less operand head-room, |V| <= 2 max|x|, and the output transform's own cancellation M1 - M2 - M3).
    Adversarial dynamic range INSIDE one image for the fp16 x 2 operand split (conv_common.hpp): 1 % of the activations sit at the
    image's maximum, the rest in equal shares at amax * 2^t for t in `tiers` (the operand scale is derived from amax alone, so the bulk
    lands deep in fp16's lower range, the last tier in its subnormals); the weights likewise.  corner=True confines the amax values to the
    top-left 8 x 8 pixels, so most outputs are sums of tiny terms only.
    Returns (max|y - ref64|, max|conv_fp32 - ref64|, max|y - ref64| over outputs that see no amax activation, their max|ref64|, amax_x, amax_w):
    the exact-fp32 chain on the same data is the yardstick (torch fp32 conv on the CPU)."""
    def tiered(name, shape, amax, spatial=None):
        u = prng.uniform01(seed, name + "_u", shape)                     # magnitude within a tier: [0.5, 1)
        sgn = torch.where(prng.uniform01(seed, name + "_s", shape) < 0.5, -1.0, 1.0)
        sel = prng.uniform01(seed, name + "_t", shape)
        e = torch.zeros(shape)
        nt = len(tiers)
        for i, t in enumerate(tiers):
            e = torch.where((sel >= 0.01 + 0.99 * i / nt) & (sel < 0.01 + 0.99 * (i + 1) / nt), float(t), e)
        top = sel < 0.01
        if spatial is not None:
            top = top & spatial
            e = torch.where((sel < 0.01) & ~spatial, float(tiers[0]), e)
        e = torch.where(top, 0.0, e)
        v = sgn * (0.5 + 0.5 * u) * torch.exp2(e) * amax
        if top.any():
            v.view(-1)[top.view(-1).nonzero()[0]] = amax                 # the maximum itself is present
        return v.float(), top

    sp = None
    if corner:
        sp = torch.zeros(N, Cin, H, W, dtype=torch.bool)
        sp[:, :, :8, :8] = True
    x, xtop = tiered("x", (N, Cin, H, W), 3.0, sp)
    if weights_too:
        w, _ = tiered("w", (Cout, Cin, 3, 3), 2.0 / (Cin * 9) ** 0.5)
    else:
        w = _rand(seed, "w", (Cout, Cin, 3, 3)) * (2.0 / (Cin * 9) ** 0.5)
    xp = F.pad(x, (1,) * 4, mode="reflect")
    ref = F.conv2d(xp.double(), w.double())
    y32 = F.conv2d(xp, w)
    bound = float(x.abs().max()) * 1.0001
    xd, wd = nhwc(x).to(dev), w.to(dev)
    y = torch.full((N, H, W, Cout), float("nan"), device=dev)
    rc = lib.tsnet_op_conv2d(xd.data_ptr(), N, H, W, Cin, wd.data_ptr(), None, Cout, 3, 1, 1, 1, None, None, 0, bound, 3, kernel, 0, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    yc = nchw(y.cpu()).double()
    e_h2 = (yc - ref).abs().max().item()
    e_32 = (y32.double() - ref).abs().max().item()
    # outputs whose 3 x 3 receptive field holds no amax activation in any channel
    seen = F.max_pool2d(F.pad(xtop.any(dim=1, keepdim=True).float(), (1,) * 4, mode="reflect"), 3, 1)      # (N,1,H,W)
    quiet = (seen == 0).expand(-1, Cout, -1, -1)
    e_quiet = (yc - ref)[quiet].abs().max().item() if quiet.any() else 0.0
    r_quiet = ref[quiet].abs().max().item() if quiet.any() else 0.0
    return e_h2, e_32, e_quiet, r_quiet, float(x.abs().max()), float(w.abs().max())


def conv_structured_filter_case(lib, dev, N, H, W, Cin, Cout, kind, kernel=3, norm=True, seed=0):
    """STRUCTURED 3 x 3 filters, as a trained checkpoint holds them (the op tests' and the seed sweep's weights are i.i.d. N(0, 0.02) / uniform):
    every (output, input, tap row) draws one amplitude a and the three taps along x follow a fixed profile --
      "smooth"    a * (2^-8, 1, 2^-8):  g0 = g2, |g1| >> |g0|: the Winograd filters U1 = (g0+g1+g2)/2 and U2 = (g0-g1+g2)/2 are +-g1/2 to eight bits
                  and the small taps live in their difference;
      "binomial"  a * (1/2, 1, 1/2):    a low-pass filter, g0 = g2;
      "sobel"     a * (-1, 0, 1):       antisymmetric: g0 + g2 = 0 and g1 = 0, so U1 = U2 = 0 and the whole output comes from M0 = V0 g0 and
                  M3 = V3 g2;
      "edge"      a * (1, -2, 1):       second difference: U1 = 0, U2 = 2 a -- out[2j+1] = M1 - M2 - M3 is all M2.
    Input: relu(x * alpha + beta) with the fused transform when `norm` (the ResnetBlock's second convolution), zero-free uniform data
    otherwise.  Returns (max|y - ref64|, max|conv_fp32 - ref64|, max|ref64|): the exact-fp32 chain (torch fp32 conv on the CPU) is the yardstick."""
    prof = {"smooth": (2.0 ** -8, 1.0, 2.0 ** -8), "binomial": (0.5, 1.0, 0.5), "sobel": (-1.0, 0.0, 1.0), "edge": (1.0, -2.0, 1.0)}[kind]
    a = _rand(seed, "wa", (Cout, Cin, 3, 1)) * (2.0 / (Cin * 9) ** 0.5)
    w = (a * torch.tensor(prof, dtype=torch.float32).view(1, 1, 1, 3)).contiguous()
    x = _rand(seed, "x", (N, Cin, H, W))
    xin, al, be = x, None, None
    if norm:
        al = _rand(seed, "al", (N, Cin), 0.5, 1.5)
        be = _rand(seed, "be", (N, Cin), -0.3, 0.3)
        xin = F.relu(x * al[:, :, None, None] + be[:, :, None, None])
    xp = F.pad(xin, (1,) * 4, mode="reflect")
    ref = F.conv2d(xp.double(), w.double())
    y32 = F.conv2d(xp, w)
    bound = float(xin.abs().max()) * 1.0001
    xd, wd = nhwc(x).to(dev), w.to(dev)
    ald = al.contiguous().to(dev) if norm else None
    bed = be.contiguous().to(dev) if norm else None
    y = torch.full((N, H, W, Cout), float("nan"), device=dev)
    rc = lib.tsnet_op_conv2d(xd.data_ptr(), N, H, W, Cin, wd.data_ptr(), None, Cout, 3, 1, 1, 1, _p(ald), _p(bed), int(norm), bound, 3, kernel, 0, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    yc = nchw(y.cpu()).double()
    return (yc - ref).abs().max().item(), (y32.double() - ref).abs().max().item(), ref.abs().max().item()


def conv_w1_odd_slab_case(lib, dev, N=1, H=4, W=32, Cin=48, Cout=64, seed=0):
    """conv_w1 with an ODD number of 16-channel slabs and a fused InstanceNorm: the last period stages 16 channels past Cin.  They
    used to be the next pixel's channels 0..15 transformed with the affine of channels 0..3 -- not bounded by the operand bound; beyond
    fp16's range they became inf, and inf x (zero weights) = NaN reached real outputs.  Here channels 0..3 carry a gain of 1e3 on tiny
    values (so the layer's bound stays ~1) while the next pixel's channels 16..19 are O(1): the old staging saw 1e3.  Now the lanes past Cin
    read zeros and the table holds zeros there.  Returns max|d| relative to max|fp64 reference| (NaN-safe: a NaN fails the comparison)."""
    x = _rand(seed, "x", (N, Cin, H, W))
    x[:, :4] *= 1e-3
    al = _rand(seed, "al", (N, Cin), 0.5, 1.5)
    al[:, :4] = 1e3
    be = _rand(seed, "be", (N, Cin), -0.3, 0.3)
    w = _rand(seed, "w", (Cout, Cin, 3, 3)) * (2.0 / (Cin * 9) ** 0.5)
    xin = F.relu(x * al[:, :, None, None] + be[:, :, None, None])
    ref = F.conv2d(F.pad(xin.double(), (1,) * 4, mode="reflect"), w.double())
    bound = float(xin.abs().max()) * 1.0001
    xd, wd, ald, bed = nhwc(x).to(dev), w.to(dev), al.contiguous().to(dev), be.contiguous().to(dev)
    y = torch.full((N, H, W, Cout), float("nan"), device=dev)
    rc = lib.tsnet_op_conv2d(xd.data_ptr(), N, H, W, Cin, wd.data_ptr(), None, Cout, 3, 1, 1, 1, ald.data_ptr(), bed.data_ptr(), 1, bound, 3, 3, 0, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    yc = nchw(y.cpu()).double()
    assert torch.isfinite(yc).all(), "non-finite outputs"
    return ((yc - ref).abs().max() / ref.abs().max()).item()


def conv_g64_cases(lib, dev, big=False):
    """conv_g64 (csrc/conv_g64.hpp: the general implicit GEMM in 64-deep K steps) against conv_h2r (16-deep steps) on the layer kinds the
    forward sends it -- the two kernels run the same chains, so the outputs must be EQUAL BITS -- and against the fp64 reference.  Shapes:
    1 x 1 (fuse_net.conv / dec.map_conv), 3 x 3 stride 2 with the producer's InstanceNorm + ReLU on load (the 64 -> 128 layer; with bf16
    operands every stride-2 layer), 3 x 3 stride 1 with reflection on a ragged frame, 192 channels (three steps per tap), both tile heights;
    the concat formed on load (own channel split per tensor, shared second image).  Returns the worst relative error of the fp16 x 2 cases."""
    worst = 0.0
    shapes = [(2, 8, 8, 128, 128, 1, 1, 0, False, False, 3, 64), (1, 16, 16, 64, 128, 3, 2, 1, False, True, 3, 128), (2, 10, 12, 64, 256, 3, 1, 1, True, True, 3, 128),
              (1, 16, 16, 128, 128, 3, 2, 1, False, True, 1, 128), (1, 9, 7, 192, 128, 3, 2, 1, False, False, 3, 128)]
    if big:      # the forward's own shapes at the headline batch
        shapes += [(4, 32, 32, 1024, 512, 1, 1, 0, False, False, 3, 64), (3, 256, 256, 64, 128, 3, 2, 1, False, True, 3, 128), (2, 64, 64, 256, 512, 3, 2, 1, False, True, 1, 128)]
    for (N, H, W, Cin, Cout, k, st, pad, refl, norm, nprod, ref_tile) in shapes:
        a = conv_case(lib, dev, N, H, W, Cin, Cout, k, st, pad, refl, norm=norm, nprod=nprod, kernel=1, tile=ref_tile, return_output=True)
        for tile in (3064, 3128):
            b = conv_case(lib, dev, N, H, W, Cin, Cout, k, st, pad, refl, norm=norm, nprod=nprod, kernel=1, tile=tile, return_output=True)
            assert torch.equal(a, b), (N, H, W, Cin, Cout, k, st, nprod, tile, (a - b).abs().max().item())
        if nprod == 3:
            worst = max(worst, conv_case(lib, dev, N, H, W, Cin, Cout, k, st, pad, refl, norm=norm, nprod=nprod, kernel=1, tile=3064))
        c = conv_case(lib, dev, N, H, W, Cin, Cout, k, st, pad, refl, norm=norm, nprod=nprod, kernel=1, tile=0, return_output=True)    # the launcher's own choice
        assert torch.equal(a, c)
    worst = max(worst, conv_cat_case(lib, dev, 2, 8, 8, 64, 64, 128), conv_cat_case(lib, dev, 2, 8, 8, 128, 64, 256, shared=True))
    if big:
        worst = max(worst, conv_cat_case(lib, dev, 4, 32, 32, 512, 512, 512))
    return worst


def conv_h2s32_cases(lib, dev, big=False):
    """The pose model's 7 x 7 stems (32 padded input channels) on their patch kernel (csrc/conv_h2s32.hpp; kernel = 0: the layer's own) against
    the general kernel (kernel = 1, conv_h2r) -- same K order and chains: EQUAL BITS -- and against the fp64 reference: one tile, several tiles
    and images with reflection at all four borders, a narrow net (8 output channels), three channel tiles with a ragged last one, bf16 operands."""
    worst = 0.0
    shapes = [(1, 4, 32, 64, 3, True, 0), (2, 8, 64, 64, 3, False, 3), (1, 12, 32, 8, 3, True, 5), (1, 4, 64, 130, 3, True, 7), (1, 8, 32, 64, 1, True, 9)]
    if big:
        shapes += [(2, 256, 256, 64, 3, True, 11)]
    for (N, H, W, Cout, nprod, bias, seed) in shapes:
        a = conv_case(lib, dev, N, H, W, 32, Cout, 7, 1, 3, True, nprod=nprod, bias=bias, seed=seed, kernel=1, tile=64, return_output=True)
        b = conv_case(lib, dev, N, H, W, 32, Cout, 7, 1, 3, True, nprod=nprod, bias=bias, seed=seed, kernel=0, return_output=True)
        assert torch.equal(a, b), (N, H, W, Cout, nprod, (a - b).abs().max().item())
        if nprod == 3:
            worst = max(worst, conv_case(lib, dev, N, H, W, 32, Cout, 7, 1, 3, True, nprod=nprod, bias=bias, seed=seed, kernel=2))
    return worst


# ---- the request grid: what tsnet_op_conv2d accepts ------------------------------------------------------------------------------------
# One layer of every kind, each the smallest shape at which its kernel has a whole tile, crossed with kernel 0..3, every documented tile
# code (kernel 3: tiles per workgroup) and nprod 1 / 3 / 4.  "What the planner accepts is what is built": an accepted entry runs and
# matches the reference, a refused one returns TSNET_ERR_ARG before the convolution is launched.  The table below was generated once from
# the planner (tests/emu/plan_driver.cpp, query R) and is read from here on: tests/test_conv_plan.py holds the planner to it entry by entry,
# tests/test_emu_ops.py and tests/test_gpu_ops.py walk it through the operator.
REQUEST_LAYERS = {   # name: (N, H, W, Cin, Cout, k, stride, pad, reflect, norm)
    "s1_c32": (1, 4, 32, 32, 128, 3, 1, 1, True, True),
    "s1_c48": (1, 4, 32, 48, 128, 3, 1, 1, True, True),          # three 16-channel slabs: no two-K-group tile
    "s2_c16": (1, 8, 64, 16, 128, 3, 2, 1, False, True),
    "stem_c8": (1, 4, 32, 8, 64, 7, 1, 3, True, False),
    "stem_c32": (1, 4, 32, 32, 64, 7, 1, 3, True, False),
    "p1_c16": (1, 5, 7, 16, 24, 1, 1, 0, False, False),
    "p1_c64": (1, 8, 8, 64, 128, 1, 1, 0, False, False),
}
REQUEST_TILES = (0, 1, 2, 3, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064)
# (layer, kernel) -> nprod -> the tile codes accepted; every other tile code of REQUEST_TILES is refused.  (The stems' kernels have one
# tile and take any decodable code for it.)
_REQUEST_ACCEPTED = {
    ("s1_c32", 0): {1: (0, 32, 64, 128, 2128, 3128, 20032, 20064), 3: (0, 32, 64, 128, 2128, 20032, 20064), 4: (0, 64, 128)},
    ("s1_c32", 1): {1: (0, 64, 128), 3: (0, 64, 128), 4: ()},
    ("s1_c32", 2): {1: (0, 32, 64, 128, 2128, 3128, 20032, 20064), 3: (0, 32, 64, 128, 2128, 20032, 20064), 4: (0, 64, 128)},
    ("s1_c32", 3): {1: (0, 1), 3: (0, 1), 4: ()},
    ("s1_c48", 0): {1: (0, 32, 64, 128, 2128, 3128), 3: (0, 32, 64, 128, 2128), 4: (0, 64, 128)},
    ("s1_c48", 1): {1: (0, 64, 128), 3: (0, 64, 128), 4: ()},
    ("s1_c48", 2): {1: (0, 32, 64, 128, 2128, 3128), 3: (0, 32, 64, 128, 2128), 4: (0, 64, 128)},
    ("s1_c48", 3): {1: (0, 1), 3: (0, 1), 4: ()},
    ("s2_c16", 0): {1: (0, 64, 128), 3: (0, 64, 128), 4: ()},
    ("s2_c16", 1): {1: (0, 64, 128), 3: (0, 64, 128), 4: ()},
    ("s2_c16", 2): {1: (0, 64, 128, 2128), 3: (0, 64, 128, 2128, 12128), 4: ()},
    ("s2_c16", 3): {1: (), 3: (), 4: ()},
    ("stem_c8", 0): {1: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 3: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 4: ()},
    ("stem_c8", 1): {1: (0, 64), 3: (0, 64), 4: ()},
    ("stem_c8", 2): {1: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 3: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 4: ()},
    ("stem_c8", 3): {1: (), 3: (), 4: ()},
    ("stem_c32", 0): {1: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 3: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 4: ()},
    ("stem_c32", 1): {1: (0, 64), 3: (0, 64), 4: ()},
    ("stem_c32", 2): {1: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 3: (0, 32, 64, 128, 2128, 3064, 3128, 12128, 20032, 20064), 4: ()},
    ("stem_c32", 3): {1: (), 3: (), 4: ()},
    ("p1_c16", 0): {1: (0, 64), 3: (0, 64), 4: ()},
    ("p1_c16", 1): {1: (0, 64), 3: (0, 64), 4: ()},
    ("p1_c16", 2): {1: (), 3: (), 4: ()},
    ("p1_c16", 3): {1: (), 3: (), 4: ()},
    ("p1_c64", 0): {1: (0, 64, 3064, 3128), 3: (0, 64, 3064, 3128), 4: ()},
    ("p1_c64", 1): {1: (0, 64, 3064, 3128), 3: (0, 64, 3064, 3128), 4: ()},
    ("p1_c64", 2): {1: (), 3: (), 4: ()},
    ("p1_c64", 3): {1: (), 3: (), 4: ()},
}
REQUEST_GRID = [dict(layer=l, kernel=k, tile=t, nprod=n, accepted=t in _REQUEST_ACCEPTED[(l, k)][n])
                for l in REQUEST_LAYERS for k in (0, 1, 2, 3) for n in (1, 3, 4) for t in REQUEST_TILES]
TSNET_ERR_ARG = -1


def request_shape(e, cus=256):
    """the ConvShape fields of a REQUEST_GRID entry as tests/emu/plan_driver.cpp reads them (tsnet_op_conv2d's OpLayer padding rules)"""
    N, H, W, Ci, Co, k, st, pad, refl, norm = REQUEST_LAYERS[e["layer"]]
    form = int(e["kernel"] == 3)
    kpad = (12 * Ci if form else k * k * Ci) + 31 & ~31
    npad = Co + 127 & ~127 if Co >= 128 else Co + 63 & ~63
    return [k, st, pad, int(refl), Ci, Co, npad, kpad, form, N, H, W, 0, int(norm), e["nprod"], 0, cus]


def request_grid_walk(lib, dev, rel3, rel1, entries=REQUEST_GRID):
    """`entries` of REQUEST_GRID through tsnet_op_conv2d on a NaN-filled output.  Accepted: rc == 0 and max|d| / max|fp64 reference| below
    rel3 (3 / 4 products) or rel1 (bf16 operands).  Refused: TSNET_ERR_ARG, a message, the output untouched.  One input set and one fp64
    reference per layer.  Returns (accepted, refused) counts."""
    data, count, reasons = {}, [0, 0], set()
    for e in entries:
        N, H, W, Ci, Co, k, st, pad, refl, norm = REQUEST_LAYERS[e["layer"]]
        if e["layer"] not in data:
            x = _rand(1, "x", (N, Ci, H, W))
            w = _rand(1, "w", (Co, Ci, k, k)) * (2.0 / (Ci * k * k) ** 0.5)
            b = _rand(1, "b", (Co,))
            al = _rand(1, "al", (N, Ci), 0.5, 1.5) if norm else None
            be = _rand(1, "be", (N, Ci), -0.3, 0.3) if norm else None
            xin = F.relu(x * al[:, :, None, None] + be[:, :, None, None]) if norm else x
            xp = F.pad(xin.double(), (pad,) * 4, mode="reflect" if refl else "constant")
            ref = F.conv2d(xp, w.double(), b.double(), stride=st)
            dv = [None if t is None else t.contiguous().to(dev) for t in (nhwc(x), w, b, al, be)]
            data[e["layer"]] = (dv, ref, float(xin.abs().max()) * 1.0001)
        (xd, wd, bd, ald, bed), ref, bound = data[e["layer"]]
        y = torch.full((N, ref.shape[2], ref.shape[3], Co), float("nan"), device=dev)
        rc = lib.tsnet_op_conv2d(xd.data_ptr(), N, H, W, Ci, wd.data_ptr(), bd.data_ptr(), Co, k, st, pad, int(refl), _p(ald), _p(bed), int(norm),
                                 bound, e["nprod"], e["kernel"], e["tile"], y.data_ptr(), None)
        _sync(dev)
        if e["accepted"]:
            assert rc == 0, (e, lib.tsnet_op_last_error().decode())
            err = _rel(nchw(y.cpu()), ref)
            assert err < (rel1 if e["nprod"] == 1 else rel3), (e, err)
        else:
            msg = lib.tsnet_op_last_error().decode()       # (kept from the last failing call: it must be this entry's own)
            assert rc == TSNET_ERR_ARG and msg.startswith("conv"), (e, rc, msg)
            if e["kernel"] != 3 and e["tile"] in (1, 2, 3):
                assert msg.endswith(f"unknown tile code {e['tile']}"), (e, msg)
            if e["kernel"] == 3 and k != 3:
                assert "Winograd" in msg, (e, msg)
            if e["nprod"] == 4 and e["kernel"] == 1 and e["tile"] in (0, 64):
                assert "products" in msg, (e, msg)
            reasons.add(msg)
            assert torch.isnan(y).all().item(), e
        count[0 if e["accepted"] else 1] += 1
    assert entries is not REQUEST_GRID or len(reasons) >= 12, reasons      # the whole grid's refusals name a dozen different reasons
    return tuple(count)


# ---- bf16 operands (nprod = 1, tsnet_cfg.operand_mode 1 / 2) against an OPERAND-EXACT reference ------------------------------------------
# A bf16 conversion is exactly specified: with both operands rounded to nearest even, every product is exact in fp32 and the only error left
# is the fp32 accumulation.  The reference therefore rounds where the kernels round -- t = fp32(x*alpha + beta) (one rounding: the staging's
# fmaf), ReLU, padding of t, bf16(t) and bf16(w) -- and sums in fp64.  A model that rounds anywhere else differs by ~2^-9 relative.
REL_BF16 = 1e-5


def bf16_round(t):
    """round to nearest even to bf16, widened back to the input's dtype"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def bf16_operand(x, al=None, be=None, relu=False):
    """the operand the kernels stage, NCHW fp32, before padding: fp32(x*alpha + beta) rounded once from fp64, ReLU"""
    t = x
    if al is not None:
        t = (x.double() * al.double()[:, :, None, None] + be.double()[:, :, None, None]).float()
    if relu:
        t = F.relu(t)
    return t


def bf16_conv_ref(x, w, b, al, be, relu, stride, pad, reflect):
    """operand-exact reference of a bf16-operand convolution (fp64 NCHW): transform, ReLU, pad t, round t and w to bf16, fp64 conv + bias"""
    t = bf16_operand(x, al, be, relu)
    if pad:
        t = F.pad(t, (pad,) * 4, mode="reflect" if reflect else "constant")
    b64 = None if b is None else b.double()
    return F.conv2d(bf16_round(t).double(), bf16_round(w).double(), b64, stride=stride)


def w1_bf16_model(x, w, b, al, be, relu, reflect):
    """conv_w1 (the Winograd F(2,3)-along-x form, 3 x 3 / stride 1 / pad 1) with bf16 operands, as its header specifies it: d = the padded
    fp32 t; V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3 formed in fp32 and rounded to bf16; U = the filter transform in fp64,
    rounded once to fp32, then to bf16; M_p = fp64 sums over (c, ky); out[2j] = M0 + M1 + M2, out[2j+1] = M1 - M2 - M3 (+ bias).  fp64 NCHW."""
    d = F.pad(bf16_operand(x, al, be, relu), (1,) * 4, mode="reflect" if reflect else "constant")      # (N, C, H+2, W+2) fp32
    d0, d1, d2, d3 = (d[..., i:i + d.shape[-1] - 3:2] for i in range(4))                               # d[2j-1+i] in unpadded columns
    V = [bf16_round(v).double() for v in (d0 - d2, d1 + d2, d2 - d1, d1 - d3)]                          # (N, C, H+2, W/2)
    g = w.double()
    U = [g[..., 0], 0.5 * (g[..., 0] + g[..., 1] + g[..., 2]), 0.5 * (g[..., 0] - g[..., 1] + g[..., 2]), g[..., 2]]
    M = [F.conv2d(v, bf16_round(u.float()).double().unsqueeze(-1)) for v, u in zip(V, U)]               # (N, O, H, W/2)
    out = torch.stack((M[0] + M[1] + M[2], M[1] - M[2] - M[3]), dim=-1).flatten(-2)
    return out if b is None else out + b.double()[None, :, None, None]


def run_conv_op(lib, dev, x, w, b, al, be, relu, k, stride, pad, reflect, bound, nprod, kernel, tile):
    """tsnet_op_conv2d on NCHW CPU tensors; returns the NCHW fp32 output on the CPU"""
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xd, wd = nhwc(x).to(dev), w.contiguous().to(dev)
    bd = None if b is None else b.to(dev)
    ald = None if al is None else al.contiguous().to(dev)
    bed = None if be is None else be.contiguous().to(dev)
    y = torch.full((N, Ho, Wo, Cout), float("nan"), device=dev)
    rc = lib.tsnet_op_conv2d(xd.data_ptr(), N, H, W, Cin, wd.data_ptr(), _p(bd), Cout, k, stride, pad, int(reflect),
                             _p(ald), _p(bed), int(relu), bound, nprod, kernel, tile, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    return nchw(y.cpu())


def _rel(y, ref):
    return ((y.double() - ref).abs().max() / ref.abs().max()).item()


def conv_bf16_case(lib, dev, N, H, W, Cin, Cout, k, stride, pad, reflect, norm=False, relu=None, bias=True, seed=0, kernel=0, tile=0,
                   scale=1.0, ref="bf16"):
    """tsnet_op_conv2d with bf16 operands (nprod = 1) against the operand-exact reference (ref = "bf16", every direct kernel) or the
    Winograd-domain model (ref = "w1", kernel = 3).  Inputs as conv_case's; with `norm` the per-image alpha / beta differ per image.
    Returns max|d| relative to max|reference|."""
    x = _rand(seed, "x", (N, Cin, H, W)) * scale
    w = _rand(seed, "w", (Cout, Cin, k, k)) * (2.0 / (Cin * k * k) ** 0.5)
    b = _rand(seed, "b", (Cout,)) if bias else None
    relu = norm if relu is None else relu
    al = _rand(seed, "al", (N, Cin), 0.5, 1.5) if norm else None
    be = _rand(seed, "be", (N, Cin), -0.3, 0.3) if norm else None
    if ref == "w1":
        r = w1_bf16_model(x, w, b, al, be, relu, reflect)
    else:
        r = bf16_conv_ref(x, w, b, al, be, relu, stride, pad, reflect)
    y = run_conv_op(lib, dev, x, w, b, al, be, relu, k, stride, pad, reflect, 1.0, 1, kernel, tile)
    return _rel(y, r)


def run_cat_op(lib, dev, x, x2, w, b, k, nprod, bound=1.0):
    """tsnet_op_conv2d_cat on NCHW CPU tensors (x2: x2_nmod images); returns the NCHW fp32 output on the CPU"""
    N, C1, H, W = x.shape
    C2, Cout = x2.shape[1], w.shape[0]
    y = torch.full((N, H, W, Cout), float("nan"), device=dev)
    xd, x2d, wd = nhwc(x).to(dev), nhwc(x2).to(dev), w.contiguous().to(dev)
    bd = None if b is None else b.to(dev)
    rc = lib.tsnet_op_conv2d_cat(xd.data_ptr(), x2d.data_ptr(), N, H, W, C1, C2, x2.shape[0], wd.data_ptr(), _p(bd), Cout, k, 1, k // 2, 0,
                                 bound, nprod, y.data_ptr(), None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    _sync(dev)
    return nchw(y.cpu())


def bf16_tie_values(seed, name, shape, emin=-100, emax=100):
    """fp32 values where a bf16 conversion is decided: exact ties (low 16 bits 0x8000) with an even and with an odd kept LSB, their
    neighbours one fp32 ulp either side (0x7fff, 0x8001), 0xffff (the carry into the exponent) and random low bits, both signs, binades
    2^emin .. 2^emax (normal fp32, far from bf16's overflow)"""
    n = 1
    for s in shape:
        n *= s
    u = lambda tag: prng.uniform01(seed, name + tag, (n,)).double()
    exp = (u("_e") * (emax - emin + 1)).floor().long().clamp(max=emax - emin) + emin + 127
    hi7 = (u("_m") * 128).floor().long().clamp(max=127)                          # the 7 kept mantissa bits: their LSB is the tie's parity
    low = torch.tensor([0x8000, 0x8000, 0x7FFF, 0x8001, 0xFFFF, 0x0000, 0x8000, 0x7FFF])[(u("_k") * 8).floor().long().clamp(max=7)]
    rnd = (u("_r") * 65536).floor().long().clamp(max=65535)
    low = torch.where(u("_x") < 0.125, rnd, low)
    sgn = (u("_s") < 0.5).long() << 31
    bits = sgn | (exp << 23) | (hi7 << 16) | low
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.view(torch.float32).view(shape).clone()


def _delta_weights(Cout, Cin, k):
    """channel c -> output c through the centre tap (1.0), all other taps zero: each output is one staged operand, in any summation order"""
    w = torch.zeros(Cout, Cin, k, k)
    for c in range(min(Cin, Cout)):
        w[c, c, k // 2, k // 2] = 1.0
    return w


def conv_bf16_delta_case(lib, dev, N, H, W, Cin, Cout, k, stride, pad, reflect, transform="pow2", relu=False, seed=0, kernel=0, tile=0):
    """BIT-EXACT activation rounding: a delta filter (centre tap 1.0 from channel c to output c; 1 x 1: the identity) on inputs full of bf16
    ties, no bias.  Every output is bf16(t) of one pixel, so the kernel must return the reference's bits -- a ties-away, truncating or
    misplaced rounding cannot hide in the accumulation.  transform: None (t = x), "pow2" (alpha = 2^j per (image, channel), beta = 0: the
    tie survives the fmaf), "rand" (random alpha / beta: the rounding point of the fmaf).  Returns (y, reference) as fp32 NCHW."""
    emin, emax = (-100, 100) if transform != "rand" else (-4, 4)
    x = bf16_tie_values(seed, "xt", (N, Cin, H, W), emin, emax)
    al = be = None
    if transform == "pow2":
        al = torch.exp2((prng.uniform01(seed, "alj", (N, Cin)) * 7).floor() - 3)
        be = torch.zeros(N, Cin)
    elif transform == "rand":
        al = _rand(seed, "al", (N, Cin), 0.5, 1.5)
        be = _rand(seed, "be", (N, Cin), -0.3, 0.3)
    w = _delta_weights(Cout, Cin, k)
    ref = bf16_conv_ref(x, w, None, al, be, relu, stride, pad, reflect).float()
    y = run_conv_op(lib, dev, x, w, None, al, be, relu, k, stride, pad, reflect, 1.0, 1, kernel, tile)
    return y, ref


def conv_cat_bf16_delta_case(lib, dev, N, H, W, C1, C2, shared=False, seed=0):
    """the concat formed on load, bit-exact: the identity over C1 + C2 channels on inputs full of ties.  Returns (y, reference)."""
    x = bf16_tie_values(seed, "xt", (N, C1, H, W))
    x2 = bf16_tie_values(seed, "x2t", (1 if shared else N, C2, H, W))
    C = C1 + C2
    w = _delta_weights(C, C, 1)
    ref = bf16_round(torch.cat([x, x2.expand(N, -1, -1, -1)], dim=1))
    return run_cat_op(lib, dev, x, x2, w, None, 1, 1), ref


def conv_bf16_weight_case(lib, dev, Cin, Cout, k, stride, pad, reflect, seed=0, kernel=0, tile=0):
    """BIT-EXACT weight rounding: one-hot inputs -- one 1.0 per input channel, at interior pixels spaced wider than the kernel (and at least
    pad + 1 from every border, so that no reflection duplicates them) -- no transform, no bias, weights full of bf16 ties.  Every output is
    one bf16-rounded weight or zero.  The frame (whole 4 x 32 output tiles) grows until Cin pixels fit.  Returns (y, reference), fp32 NCHW."""
    sp = k + stride                                                   # no output window sees two one-hot pixels
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
    w = bf16_tie_values(seed, "wt", (Cout, Cin, k, k), -12, 2)
    ref = bf16_conv_ref(x, w, None, None, None, False, stride, pad, reflect).float()
    y = run_conv_op(lib, dev, x, w, None, None, None, False, k, stride, pad, reflect, 1.0, 1, kernel, tile)
    return y, ref


def conv_bf16_bound_case(lib, dev, N, H, W, Cin, Cout, k, stride, pad, reflect, norm=True, seed=0, kernel=0, tile=0):
    """`bound` fixes the fp16 x 2 split's operand scale and nothing else: with bf16 operands the same call with bound 1e-30 and 1e30 must
    give the same bits.  Returns the two outputs."""
    x = _rand(seed, "x", (N, Cin, H, W))
    w = _rand(seed, "w", (Cout, Cin, k, k)) * (2.0 / (Cin * k * k) ** 0.5)
    b = _rand(seed, "b", (Cout,))
    al = _rand(seed, "al", (N, Cin), 0.5, 1.5) if norm else None
    be = _rand(seed, "be", (N, Cin), -0.3, 0.3) if norm else None
    return [run_conv_op(lib, dev, x, w, b, al, be, norm, k, stride, pad, reflect, bound, 1, kernel, tile) for bound in (1e-30, 1e30)]


# Every family and tile code tsnet_op_conv2d accepts with bf16 operands.  A case: (N, H, W, Cin, Cout, k, stride, pad, reflect, kernel, tile,
# options).  The deep stride-2 schedule (12128) and conv_w1's chunks of 2 / 3 tiles are fp16 x 2 only (the planner refuses them).
BF16_CASES = {
    "H2": [(2, 8, 32, 48, 128, 3, 1, 1, True, 2, t, dict(norm=True)) for t in (0, 32, 64, 128, 2128, 3128)] + [
        (1, 4, 32, 80, 96, 3, 1, 1, False, 2, 64, dict(norm=True, relu=False)),        # zero padding, a transform without ReLU, Cout 96
        (1, 4, 64, 64, 128, 3, 1, 1, True, 2, 20032, dict(norm=True)),                 # the two-K-group tiles
        (2, 4, 32, 64, 128, 3, 1, 1, False, 2, 20064, dict(norm=True, seed=1)),
        (1, 4, 32, 16, 64, 3, 1, 1, True, 2, 64, dict(bias=False, scale=2.0 ** 40)),   # any fp16 intermediate / operand scale would show
        (1, 4, 32, 16, 128, 3, 1, 1, True, 2, 128, dict(bias=False, scale=2.0 ** -40, seed=2))],
    "H2D": [(2, 8, 64, 16, 128, 3, 2, 1, False, 2, t, dict(norm=True)) for t in (0, 64, 128, 2128)] + [
        (1, 8, 64, 48, 96, 3, 2, 1, False, 2, 64, dict(norm=True, relu=False, seed=3)),
        (1, 8, 64, 80, 128, 3, 2, 1, False, 2, 2128, dict(bias=False, scale=2.0 ** 40))],
    "H2S": [(2, 4, 32, 8, 64, 7, 1, 3, True, 2, 0, dict()), (1, 8, 64, 8, 64, 7, 1, 3, True, 2, 0, dict(bias=False, scale=2.0 ** -40, seed=4))],
    "H2S32": [(1, 4, 32, 32, 72, 7, 1, 3, True, 0, 0, dict()), (2, 8, 32, 32, 64, 7, 1, 3, True, 0, 0, dict(bias=False, scale=2.0 ** 40, seed=5))],
    "G64": [(2, 8, 8, 128, 192, 1, 1, 0, False, 1, t, dict()) for t in (3064, 3128)] + [
        (1, 16, 16, 64, 192, 3, 2, 1, False, 1, t, dict(norm=True)) for t in (3064, 3128)] + [
        (2, 10, 12, 64, 256, 3, 1, 1, True, 1, 3064, dict(norm=True, relu=False, seed=6)),
        (1, 9, 7, 192, 128, 3, 2, 1, False, 1, 3128, dict(bias=False, scale=2.0 ** -40, seed=7))],
    "H2R": [(2, 12, 10, c, 24, k, s, p, r, 1, 64, dict(norm=n, seed=c)) for (k, s, p, r) in ((7, 1, 3, True), (3, 2, 1, False), (3, 1, 1, True))
            for (c, n) in ((8, False), (48, True))] + [
        (2, 12, 10, 16, 130, 3, 1, 1, True, 1, 128, dict(norm=True, relu=False)), (2, 5, 7, 16, 24, 1, 1, 0, False, 1, 64, dict()),
        (1, 13, 11, 80, 128, 3, 2, 1, False, 1, 128, dict(bias=False, scale=2.0 ** 40, seed=8))],
}


def bf16_family_worst(lib, dev, family):
    """the worst error relative to max|operand-exact reference| over BF16_CASES[family]"""
    worst = 0.0
    for (N, H, W, Ci, Co, k, s, p, r, kern, tile, kw) in BF16_CASES[family]:
        worst = max(worst, conv_bf16_case(lib, dev, N, H, W, Ci, Co, k, s, p, r, kernel=kern, tile=tile, **kw))
    return worst


def bf16_w1_worst(lib, dev, big=False):
    """conv_w1 with bf16 operands against the Winograd-domain model (w1_bf16_model): reflection and zero padding, the fused transform with
    and without ReLU, odd slab counts, N > 1 with per-image alpha / beta, inputs scaled by 2^+-40 without bias"""
    cases = [(2, 8, 32, 48, 96, True, dict(norm=True)), (1, 4, 32, 80, 64, False, dict(norm=True, relu=False, seed=1)),
             (1, 8, 32, 16, 128, True, dict(seed=2)), (1, 4, 32, 32, 64, True, dict(bias=False, scale=2.0 ** 40, seed=3)),
             (1, 4, 64, 32, 64, False, dict(bias=False, scale=2.0 ** -40, seed=4))]
    if big:     # the ResnetBlock / FuseNet / first up-convolution shapes
        cases += [(2, 32, 32, 512, 512, True, dict(norm=True)), (1, 32, 32, 1024, 1024, True, dict(norm=True, seed=5)),
                  (1, 64, 64, 512, 256, False, dict(norm=True, relu=False, seed=6))]
    worst = 0.0
    for (N, H, W, Ci, Co, refl, kw) in cases:
        worst = max(worst, conv_bf16_case(lib, dev, N, H, W, Ci, Co, 3, 1, 1, refl, kernel=3, ref="w1", **kw))
    return worst


# bit-exact cases per family: (N, H, W, Cin, Cout, k, stride, pad, reflect, kernel, tile); the stems take no transform
BF16_EXACT_CASES = {
    "H2": [(2, 8, 32, 48, 128, 3, 1, 1, True, 2, t) for t in (32, 64, 2128)] + [(1, 4, 32, 64, 128, 3, 1, 1, False, 2, t) for t in (128, 3128, 20032)],
    "H2D": [(2, 8, 64, 48, 128, 3, 2, 1, False, 2, t) for t in (64, 128, 2128)],
    "H2S": [(2, 8, 32, 8, 64, 7, 1, 3, True, 2, 0)],
    "H2S32": [(1, 8, 32, 32, 64, 7, 1, 3, True, 0, 0)],
    "G64": [(2, 8, 8, 64, 128, 1, 1, 0, False, 1, 3064), (1, 16, 16, 64, 128, 3, 2, 1, False, 1, 3128)],
    "H2R": [(2, 12, 10, 16, 24, 3, 1, 1, True, 1, 64), (2, 12, 10, 8, 24, 7, 1, 3, True, 1, 64), (1, 13, 11, 16, 130, 3, 2, 1, False, 1, 128),
            (2, 5, 7, 16, 24, 1, 1, 0, False, 1, 64)],
}


def bf16_exact_mismatches(lib, dev, family):
    """BF16_EXACT_CASES[family] through the delta filter on ties (no transform; alpha = 2^j with and without ReLU; one random alpha / beta),
    the one-hot input on tied weights and the two extreme bounds.  Returns the list of cases whose bits differ (empty: all exact)."""
    bad = []
    for i, (N, H, W, Ci, Co, k, s, p, r, kern, tile) in enumerate(BF16_EXACT_CASES[family]):
        stem = k == 7
        for tr, relu in ((None, False),) + (() if stem else (("pow2", False), ("pow2", True), ("rand", True))):
            y, ref = conv_bf16_delta_case(lib, dev, N, H, W, Ci, Co, k, s, p, r, transform=tr, relu=relu, seed=i, kernel=kern, tile=tile)
            if not torch.equal(y, ref):
                bad.append(("delta", tr, relu, (N, H, W, Ci, Co, k, s, tile), int((y != ref).sum())))
        y, ref = conv_bf16_weight_case(lib, dev, Ci, Co, k, s, p, r, seed=i, kernel=kern, tile=tile)
        if not torch.equal(y, ref):
            bad.append(("weights", (Ci, Co, k, s, tile), int((y != ref).sum())))
        a, b = conv_bf16_bound_case(lib, dev, N, H, W, Ci, Co, k, s, p, r, norm=not stem, seed=i, kernel=kern, tile=tile)
        if not torch.equal(a, b):
            bad.append(("bound", (N, H, W, Ci, Co, k, s, tile)))
    return bad


def bf16_forward_layers(table):
    """the distinct bf16-operand convolutions of the forward (nprod == 1 in tests/golden/conv_plan_table.json's layers), one per (shape,
    family, tile) -> (config, layer, shape dict, kernel, tile code)"""
    out, seen = [], set()
    for c in table["layers"]:
        s, p = c["shape"], c["plan"]
        if s["nprod"] != 1:
            continue
        key = tuple(s[k] for k in ("ks", "stride", "pad", "reflect", "cin", "cout", "form", "H", "W", "csplit", "transform")) + \
            tuple(p[k] for k in ("family", "rows", "width", "side_by_side", "sched"))
        if key in seen:
            continue
        seen.add(key)
        fam = p["family"]
        if fam == "H2":
            assert p["sched"] == "plain"
            kernel, tile = 2, (3128 if p["side_by_side"] else (2128 if p["rows"] == 2 else p["width"]))
        elif fam == "G64":
            kernel, tile = 1, 3000 + p["rows"]
        elif fam == "H2R":
            kernel, tile = 1, p["width"]
        elif fam in ("H2S", "H2S32"):
            kernel, tile = 2 if fam == "H2S" else 0, 0
        else:
            raise AssertionError(f"no tile code for a bf16 layer on {fam}")
        out.append((c["config"], c["layer"], s, kernel, tile))
    return out


def bf16_forward_layer_case(lib, dev, s, kernel, tile, seed=0):
    """one bf16 layer of the forward with its own tile forced, at N <= 2 (a tile's bits do not depend on the batch: tests/test_conv_plan.py),
    the producer's InstanceNorm + ReLU fused where the forward fuses it; error relative to max|operand-exact reference|"""
    N = 2 if s["H"] * s["W"] <= 64 * 64 else 1
    if s["csplit"]:         # dec.map_conv on cat(pg, sg): its own launch path, no tile request
        return conv_cat_case(lib, dev, N, s["H"], s["W"], s["csplit"], s["cin"] - s["csplit"], s["cout"], k=s["ks"], seed=seed, nprod=1, ref="bf16")
    return conv_bf16_case(lib, dev, N, s["H"], s["W"], s["cin"], s["cout"], s["ks"], s["stride"], s["pad"], bool(s["reflect"]),
                          norm=bool(s["transform"]), seed=seed, kernel=kernel, tile=tile)


# ---- the kernels between the convolutions, one operator at a time --------------------------------------------------------------------------
# Each case draws its inputs from the PRNG, evaluates the operation in fp64 torch on the CPU and returns the error (or, where one correctly
# rounded fp32 operation per element leaves no room, the tensors for torch.equal).  Images that share a launch differ from each other, and
# per-image coefficients are drawn per (image, channel): a swapped image or channel index moves the result by O(1).
def _check(lib, rc):
    assert rc == 0, lib.tsnet_op_last_error().decode()


def warp_k_inputs(B, K, h, w, C, SB, seed=0, hand=False):
    """src (K*SB, C, h, w) and flow (K*B, h, w, 2) of one warp launch.  hand=True: flows placed by hand instead of drawn -- sample positions
    (pixel units, per axis) on pixel centres, on the outermost sample positions (grid -1 and +1: half a pixel outside the border centres),
    one and several pixels outside on either side; the product of the two axes' lists holds every corner with all four neighbours outside.
    Each (source, frame) image walks the list from another start."""
    src = _rand(seed, "src", (K * SB, C, h, w), -2, 2)
    flow = _rand(seed, "flow", (K * B, h, w, 2), -1.3, 1.3)
    if hand:
        ax = lambda n: [0.0, 1.0, n - 1.0, n - 2.0, -0.5, n - 0.5, -1.0, float(n), -1.5, n + 0.5, -4.0, n + 3.0, 0.25 * n]
        pts = [((2 * x + 1) / w - 1, (2 * y + 1) / h - 1) for y in ax(h) for x in ax(w)]
        assert h * w >= len(pts), "the map is too small for every hand-placed position"
        t = torch.tensor(pts, dtype=torch.float64).float()
        for n in range(K * B):
            idx = (torch.arange(h * w) + 37 * n) % len(pts)
            flow[n] = t[idx].view(h, w, 2)
    return src, flow


def warp_k_ref(src, flow, B, K, SB):
    """fp64 grid_sample per source, then the mean over sources: (B, C, h, w); (source k, frame b) reads src[k*SB + b % SB], flow[k*B + b]"""
    acc = 0
    for k in range(K):
        sel = [k * SB + b % SB for b in range(B)]
        acc = acc + F.grid_sample(src[sel].double(), flow[k * B:(k + 1) * B].double(), mode="bilinear", padding_mode="zeros", align_corners=False)
    return acc / K


def run_warp_k(lib, dev, src, flow, B, K, SB, entry="shared"):
    """the warp through tsnet_op_warp_k_shared ("shared"), tsnet_op_warp_k ("k": SB = B) or tsnet_op_warp ("one": K = 1); NCHW on the CPU"""
    _, C, h, w = src.shape
    srcd, fd = nhwc(src).to(dev), flow.contiguous().to(dev)
    out = torch.full((B, h, w, C), float("nan"), device=dev)
    if entry == "shared":
        rc = lib.tsnet_op_warp_k_shared(srcd.data_ptr(), fd.data_ptr(), B, K, SB, h, w, C, out.data_ptr(), None)
    elif entry == "k":
        assert SB == B
        rc = lib.tsnet_op_warp_k(srcd.data_ptr(), fd.data_ptr(), B, K, h, w, C, out.data_ptr(), 1, None, None)
    else:
        assert SB == B and K == 1
        rc = lib.tsnet_op_warp(srcd.data_ptr(), fd.data_ptr(), B, h, w, C, out.data_ptr(), None)
    _check(lib, rc)
    _sync(dev)
    return nchw(out.cpu())


def warp_k_case(lib, dev, B, K, h, w, C, seed=0, hand=False, entry="shared"):
    """warp_mean_kernel with K sources per driving frame against fp64 grid_sample + mean.  Returns max|d|."""
    src, flow = warp_k_inputs(B, K, h, w, C, B, seed, hand)
    return (run_warp_k(lib, dev, src, flow, B, K, B, entry).double() - warp_k_ref(src, flow, B, K, B)).abs().max().item()


def warp_k_shared_case(lib, dev, B, K, h, w, C, seed=0):
    """one source set shared by the batch (SB = 1) and the same set replicated per frame (SB = B): (shared output, replicated output,
    max|shared - fp64 reference|)"""
    src, flow = warp_k_inputs(B, K, h, w, C, 1, seed)
    rep = src.repeat_interleave(B, dim=0)                                   # image k*B + b = source k
    a = run_warp_k(lib, dev, src, flow, B, K, 1)
    b = run_warp_k(lib, dev, rep, flow, B, K, B)
    return a, b, (a.double() - warp_k_ref(src, flow, B, K, 1)).abs().max().item()


def warp_one_source_entries(lib, dev, B, h, w, C, seed=0):
    """K = 1 through tsnet_op_warp, tsnet_op_warp_k and tsnet_op_warp_k_shared: the three outputs"""
    src, flow = warp_k_inputs(B, 1, h, w, C, B, seed)
    return [run_warp_k(lib, dev, src, flow, B, 1, B, e) for e in ("one", "k", "shared")]


def fuse_tail_inputs(B, K, P, C1, SB, seed=0):
    C = 2 * C1
    return (_rand(seed, "src", (K * SB, P, C1), -2, 2), _rand(seed, "tar", (B, P, C1), -2, 2), _rand(seed, "y2", (K * B, P, C), -2, 2),
            _rand(seed, "al", (K * B, C), 0.5, 1.5), _rand(seed, "be", (K * B, C), -0.3, 0.3))


def run_fuse_tail(lib, dev, src, tar, y2, al, be, B, K, SB):
    P, C1 = tar.shape[1:]
    d = [t.contiguous().to(dev) for t in (src, tar, y2, al, be)]
    z = torch.full((B, P, 2 * C1), float("nan"), device=dev)
    _check(lib, lib.tsnet_op_fuse_tail(*[t.data_ptr() for t in d], B, K, SB, P, C1, z.data_ptr(), None))
    _sync(dev)
    return z.cpu()


def fuse_tail_ref(src, tar, y2, al, be, B, K, SB):
    """fp64 mean over sources of cat(src[k*SB + b % SB], tar[b]) + (y2[k*B + b] * alpha + beta): (B, P, 2*C1)"""
    acc = 0
    for k in range(K):
        sel = [k * SB + b % SB for b in range(B)]
        n = slice(k * B, (k + 1) * B)
        acc = acc + torch.cat([src[sel].double(), tar.double()], dim=2) + (y2[n].double() * al[n].double()[:, None, :] + be[n].double()[:, None, :])
    return acc / K


def fuse_tail_case(lib, dev, B, K, P, C1, seed=0):
    """fuse_resid_mean_kernel against the fp64 reference; alpha / beta per (image, channel).  Returns max|d|."""
    t = fuse_tail_inputs(B, K, P, C1, B, seed)
    return (run_fuse_tail(lib, dev, *t, B, K, B).double() - fuse_tail_ref(*t, B, K, B)).abs().max().item()


def fuse_tail_shared_case(lib, dev, B, K, P, C1, seed=0):
    """SB = 1 and the same sources replicated with SB = B: (shared output, replicated output, max|shared - fp64 reference|)"""
    src, tar, y2, al, be = fuse_tail_inputs(B, K, P, C1, 1, seed)
    a = run_fuse_tail(lib, dev, src, tar, y2, al, be, B, K, 1)
    b = run_fuse_tail(lib, dev, src.repeat_interleave(B, dim=0), tar, y2, al, be, B, K, B)
    return a, b, (a.double() - fuse_tail_ref(src, tar, y2, al, be, B, K, 1)).abs().max().item()


def _instnorm64(y):
    """InstanceNorm (eps 1e-5, biased variance) of (N, HW, C) in fp64 (F.instance_norm refuses HW = 1)"""
    y = y.double()
    mean = y.mean(dim=1, keepdim=True)
    var = ((y - mean) ** 2).mean(dim=1, keepdim=True)
    return (y - mean) / torch.sqrt(var + 1e-5)


def add_stats_case(lib, dev, K, B, x_sb, HW, C, seed=0, offset=0.0):
    """add_stats_partial_kernel + its finalize: N = K*B images, add_nmod = B, x of K*x_sb images.  Returns (y, torch's fp32 x + add: one IEEE
    addition per element, so the bits must agree; max|y*alpha + beta - fp64 instance_norm(y)|)."""
    N = K * B
    x = _rand(seed, "x", (K * x_sb, HW, C), -2, 2) + offset
    add = _rand(seed, "add", (B, HW, C), -2, 2)
    sel = [n // B * x_sb + n % B % x_sb for n in range(N)]
    yref = x[sel] + add[[n % B for n in range(N)]]
    xd, ad = x.to(dev), add.to(dev)
    y = torch.full((N, HW, C), float("nan"), device=dev)
    al = torch.full((N * C,), float("nan"), device=dev)
    be = torch.full((N * C,), float("nan"), device=dev)
    _check(lib, lib.tsnet_op_add_stats(xd.data_ptr(), ad.data_ptr(), B, x_sb, N, HW, C, y.data_ptr(), al.data_ptr(), be.data_ptr(), None))
    _sync(dev)
    y, al, be = y.cpu(), al.cpu().view(N, 1, C), be.cpu().view(N, 1, C)
    return y, yref, (y * al + be - _instnorm64(yref)).abs().max().item()


# tsnet_op_finalize_stats against the same formula in fp64 on the same partials: max relative error of alpha, and of beta relative to
# |beta| + alpha.  The kernels round var to fp32, add eps, take sqrtf and divide; beta is the product of two rounded fp32 numbers: a handful
# of half-ulps (2^-24 = 6.0e-8 each).  Worst readings over S in FINALIZE_S x C in (8, 24, 64):
#   emulated build (sqrtf and / correctly rounded):  in_finalize  alpha 9.85e-8  beta 8.77e-8;   in_finalize2  alpha 1.14e-7  beta 1.39e-7
#   MI355X:                                          in_finalize  alpha 9.03e-8  beta 1.15e-7;   in_finalize2  alpha 1.05e-7  beta 1.19e-7
# The gate is twice the worse of the two builds' worst reading (1.39e-7), and not above 1e-6.
FINALIZE_TOL = 2.8e-7
FINALIZE_S = (1, 8, 9, 15, 16, 17, 127, 128, 129, 130, 1000, 1024)


def finalize_partials(S, C, N=2, rows=2, seed=0):
    """fp64 partials (N, S, C, 2) of real data (N, S*rows, C) split into S groups of `rows` rows: values in [-2, 2] plus the group's offset
    3 + 0.3 (g % 5).  Every element then lies in (0, 2 mean), so that a partial lost or counted twice moves the mean AND the variance by about
    1 / S of themselves, whichever group it is (offsets that grow with g let the group near twice the mean vanish without a trace).
    Measured on the CPU for S = 1024 (C = 16, 64) and S = 1000 (C = 24): zeroing or doubling any one partial moves alpha by >= 1.7e-3
    relative and beta by >= 1.7e-3 of |beta| + alpha -- thousands of times FINALIZE_TOL."""
    off = 3.0 + 0.3 * (torch.arange(S, dtype=torch.float64) % 5)
    x = _rand(seed, "x", (N, S, rows, C), -2, 2).double() + off.view(1, S, 1, 1)
    return torch.stack([x.sum(dim=2), (x * x).sum(dim=2)], dim=-1).contiguous(), S * rows


def finalize_ref(part, HW):
    sm, sq = part[..., 0].sum(dim=1), part[..., 1].sum(dim=1)
    mean = sm / HW
    var = (sq / HW - mean * mean).clamp(min=0)
    alpha = 1.0 / torch.sqrt(var + 1e-5)
    return alpha, -mean * alpha


def finalize_case(lib, dev, S, C, N=2, seed=0):
    """in_finalize (S <= 8) / in_finalize2 (S > 8) on caller-supplied partials.  Returns (alpha error, beta error) as defined above."""
    part, HW = finalize_partials(S, C, N, seed=seed)
    pd = part.to(dev)
    al = torch.full((N, C), float("nan"), device=dev)
    be = torch.full((N, C), float("nan"), device=dev)
    _check(lib, lib.tsnet_op_finalize_stats(pd.data_ptr(), N, S, C, HW, al.data_ptr(), be.data_ptr(), None))
    _sync(dev)
    ra, rb = finalize_ref(part, HW)
    ea = ((al.cpu().double() - ra).abs() / ra).max().item()
    eb = ((be.cpu().double() - rb).abs() / (rb.abs() + ra)).max().item()
    return ea, eb


def finalize_worst(lib, dev):
    """the worst (alpha, beta) error per kernel over FINALIZE_S x C in (8, 24, 64): {"in_finalize": (ea, eb), "in_finalize2": (ea, eb)}"""
    worst = {"in_finalize": [0.0, 0.0], "in_finalize2": [0.0, 0.0]}
    for S in FINALIZE_S:
        for C in (8, 24, 64):
            ea, eb = finalize_case(lib, dev, S, C, seed=S + C)
            wk = worst["in_finalize" if S <= 8 else "in_finalize2"]
            wk[0], wk[1] = max(wk[0], ea), max(wk[1], eb)
            assert ea == ea and eb == eb, (S, C)                            # NaN: an entry the kernel did not write
    return {k: tuple(v) for k, v in worst.items()}


def pack_case(lib, dev, S, B, H, W, L, nimg, Cp, coords, divs=None, seed=0):
    """pack_input_kernel against torch's cat(img / div, lbl, coords, zeros) in NHWC, and its per-image amax against max|out|.  Images in
    [-120, 150] (a BGR frame minus its mean), labels in [0, 1); image 0's largest magnitude is planted in a label channel, image 1's (where
    there is one) in a NEGATIVE value -- of the second image channel, or of the first label channel in the label-only form.
    Returns (out, reference, amax as floats, reference amax)."""
    import ctypes
    divs = list(divs) if divs is not None else [255.0] * S
    imgs = [_rand(seed + s, "img", (B, 3, H, W), -120, 150) for s in range(S)] if nimg else None
    lbls = [_rand(seed + s, "lbl", (B, L, H, W), 0, 1) for s in range(S)]
    lbls[0][0, L - 1, H // 2, W // 3] = 7.0
    if S * B > 1:
        s1, b1 = divmod(1, B)
        if nimg:
            imgs[s1][b1, 1, H // 3, W // 2] = -9.0 * divs[s1]
        else:
            lbls[s1][b1, 0, H // 3, W // 2] = -5.0
    table = torch.empty(H, W, 3)
    if coords:
        lib.tsnet_coord_table(H, W, ctypes.cast(table.data_ptr(), ctypes.POINTER(ctypes.c_float)))
    ref = []
    for s in range(S):
        parts = ([imgs[s] / divs[s]] if nimg else []) + [lbls[s]] + ([table.permute(2, 0, 1).expand(B, 3, H, W)] if coords else [])
        creal = sum(p.shape[1] for p in parts)
        ref.append(torch.cat(parts + [torch.zeros(B, Cp - creal, H, W)], dim=1))
    ref = nhwc(torch.cat(ref, dim=0))
    imgd = [t.to(dev) for t in imgs] if nimg else None
    lbld = [t.to(dev) for t in lbls]
    arr = lambda ts: (ctypes.c_void_p * S)(*[t.data_ptr() for t in ts])
    out = torch.full((S * B, H, W, Cp), float("nan"), device=dev)
    amax = torch.full((S * B,), -1, dtype=torch.int32, device=dev)
    _check(lib, lib.tsnet_op_pack_input(arr(imgd) if nimg else None, arr(lbld), S, B, H, W, L, nimg, Cp, int(coords),
                                        (ctypes.c_float * S)(*divs) if nimg else None, out.data_ptr(), amax.data_ptr(), None))
    _sync(dev)
    return out.cpu(), ref, amax.cpu().view(torch.float32), ref.abs().amax(dim=(1, 2, 3))


def upsample64_case(lib, dev, N, H, W, C, norm, seed=0):
    """nn.Upsample(x2, bilinear, align_corners=False) [after IN + ReLU] in fp64 vs tsnet_op_upsample2x_st with fp32 storage, which must also
    be tsnet_op_upsample2x's bits.  Returns max|d|."""
    x = _rand(seed, "x", (N, C, H, W), -2, 2)
    al = _rand(seed, "al", (N, C), 0.5, 1.5) if norm else None
    be = _rand(seed, "be", (N, C), -0.3, 0.3) if norm else None
    xin = x.double()
    if norm:
        xin = F.relu(xin * al.double()[:, :, None, None] + be.double()[:, :, None, None])
    ref = F.interpolate(xin, scale_factor=2, mode="bilinear", align_corners=False)
    y = run_upsample_st(lib, dev, x, al, be, 0, 0)
    xd = nhwc(x).to(dev)
    ald, bed = (al.to(dev), be.to(dev)) if norm else (None, None)
    y0 = torch.full((N, 2 * H, 2 * W, C), float("nan"), device=dev)
    _check(lib, lib.tsnet_op_upsample2x(xd.data_ptr(), _p(ald), _p(bed), int(norm), N, H, W, C, y0.data_ptr(), None))
    _sync(dev)
    assert torch.equal(y0.cpu(), y)
    return (nchw(y).double() - ref).abs().max().item()


def run_upsample_st(lib, dev, x, al, be, x_bf16, y_bf16):
    """tsnet_op_upsample2x_st on an NCHW fp32 CPU tensor (stored as bf16 on the device when x_bf16: x must be representable); the NHWC output
    on the CPU, widened to fp32 when y_bf16"""
    N, C, H, W = x.shape
    xd = nhwc(x).to(dev)
    if x_bf16:
        assert torch.equal(bf16_round(x), x)
        xd = xd.to(torch.bfloat16)
    ald = None if al is None else al.contiguous().to(dev)
    bed = None if be is None else be.contiguous().to(dev)
    y = torch.full((N, 2 * H, 2 * W, C), float("nan"), device=dev, dtype=torch.bfloat16 if y_bf16 else torch.float32)
    _check(lib, lib.tsnet_op_upsample2x_st(xd.data_ptr(), _p(ald), _p(bed), int(al is not None), N, H, W, C, int(x_bf16), int(y_bf16), y.data_ptr(), None))
    _sync(dev)
    return y.cpu().float()


def upsample_storage_case(lib, dev, N, H, W, C, norm, seed=0, ties=False):
    """bf16 storage of the upsample's input and output.  Data: bf16-representable values in [-2, 2], or (ties=True) fp32 values where a
    bf16 rounding is decided (bf16_tie_values: a 1 x 1 map hands every one of them to the output unchanged).  Returns the pairs that must be
    equal bits: (bf16 input, the same values as fp32), (bf16 output, bf16_round of the fp32 output), (both, bf16_round of the fp32 output)."""
    al = _rand(seed, "al", (N, C), 0.5, 1.5) if norm else None
    be = _rand(seed, "be", (N, C), -0.3, 0.3) if norm else None
    x = bf16_tie_values(seed, "xt", (N, C, H, W), -20, 20) if ties else bf16_round(_rand(seed, "x", (N, C, H, W), -2, 2))
    y32 = run_upsample_st(lib, dev, x, al, be, 0, 0)
    pairs = [(run_upsample_st(lib, dev, x, al, be, 0, 1), bf16_round(y32))]
    if not ties:                                                            # (the ties themselves are not bf16 values)
        pairs += [(run_upsample_st(lib, dev, x, al, be, 1, 0), y32), (run_upsample_st(lib, dev, x, al, be, 1, 1), bf16_round(y32))]
    return pairs


def op_refusals(lib, dev, op):
    """the bad arguments of one of the new operators: each call must return TSNET_ERR_ARG with a message of its own and leave the
    NaN-filled outputs untouched (the host code refuses before anything is launched).  Returns the number of refusals walked."""
    import ctypes
    z = torch.zeros(4096, device=dev)
    zd = torch.zeros(4096, dtype=torch.float64, device=dev)
    outs = [torch.full((4096,), float("nan"), device=dev) for _ in range(3)]
    p, o = z.data_ptr(), [t.data_ptr() for t in outs]
    ptrs = lambda *v: (ctypes.c_void_p * 8)(*v)
    two = ptrs(p, p)
    div = (ctypes.c_float * 8)(255.0, 255.0)
    if op == "warp_k_shared":       # (src, flow, B, K, SB, h, w, C, out)
        fn, good = lib.tsnet_op_warp_k_shared, [p, p, 2, 2, 2, 4, 4, 8, o[0], None]
        bad = [{0: None}, {1: None}, {8: None}, {7: 6}, {7: 0}, {3: 0}, {3: 9}, {4: 0}, {2: 3, 4: 2}, {2: 0}, {5: 0}]
    elif op == "add_stats":         # (x, add, add_nmod, x_sb, N, HW, C, y, alpha, beta)
        fn, good = lib.tsnet_op_add_stats, [p, p, 2, 2, 4, 4, 8, o[0], o[1], o[2], None]
        bad = [{0: None}, {1: None}, {7: None}, {8: None}, {9: None}, {6: 6}, {6: 0}, {2: 3}, {2: 0}, {3: 0}, {2: 4, 3: 3}, {4: 0}, {5: 0}]
    elif op == "finalize_stats":    # (part, N, S, C, HW, alpha, beta)
        fn, good = lib.tsnet_op_finalize_stats, [zd.data_ptr(), 2, 4, 8, 16, o[0], o[1], None]
        bad = [{0: None}, {5: None}, {6: None}, {3: 6}, {3: 0}, {2: 0}, {4: 0}, {1: 0}]
    elif op == "fuse_tail":         # (src, tar, y2, alpha, beta, B, K, SB, P, C1, zbar)
        fn, good = lib.tsnet_op_fuse_tail, [p, p, p, p, p, 2, 2, 2, 4, 8, o[0], None]
        bad = [{i: None} for i in (0, 1, 2, 3, 4, 10)] + [{9: 6}, {9: 0}, {6: 0}, {6: 9}, {7: 0}, {5: 3, 7: 2}, {8: 0}, {5: 0}]
    elif op == "pack_input":        # (img, lbl, S, B, H, W, L, nimg, Cp, coords, img_div, out, amax)
        fn, good = lib.tsnet_op_pack_input, [two, two, 2, 1, 4, 4, 2, 3, 8, 1, div, o[0], o[1], None]
        bad = [{0: None}, {1: None}, {10: None}, {11: None}, {12: None}, {0: ptrs(p, None)}, {1: ptrs(None, p)}, {2: 0}, {2: 9}, {7: 1}, {8: 7}, {6: 3},
               {8: 24}, {9: 0, 8: 4}, {3: 0}, {4: 0}, {6: 0}, {10: (ctypes.c_float * 8)(255.0, 0.0)}, {7: 0, 8: 4}, {7: 0, 6: 25, 8: 24}]
    elif op == "upsample2x_st":     # (x, alpha, beta, relu, N, H, W, C, x_bf16, y_bf16, y)
        fn, good = lib.tsnet_op_upsample2x_st, [p, None, None, 0, 1, 4, 4, 8, 0, 0, o[0], None]
        bad = [{0: None}, {10: None}, {1: p}, {7: 6}, {7: 0}, {4: 0}, {5: 0}, {6: 0}]
    else:
        raise AssertionError(op)
    for change in bad:
        args = list(good)
        for i, v in change.items():
            args[i] = v
        rc = fn(*args)
        msg = lib.tsnet_op_last_error().decode()
        _sync(dev)
        assert rc == TSNET_ERR_ARG and msg, (op, change, rc, msg)
        assert all(torch.isnan(t).all().item() for t in outs), (op, change)
    return len(bad)


# the shapes both tiers run: the smallest at which each kernel can still go wrong
WARP_K_SHAPES = [(2, 3, 16, 12, 128), (1, 8, 7, 9, 16), (3, 2, 32, 32, 64),         # (B, K, h, w, C)
                 (5, 1, 32, 32, 512)]                                               # 2560 blocks of 256 quads: the grid-stride loop (2048 blocks) repeats
FUSE_TAIL_SHAPES = [(2, 3, 7 * 9, 16), (1, 8, 16, 8), (3, 2, 64, 512),              # (B, K, P, C1)
                    (2, 2, 1040, 512)]                                              # 2080 blocks: the loop repeats, the last pass ragged
ADD_STATS_CASES = {                                                                 # (K, B, x_sb, HW, C): N = K*B, add_nmod = B
    "per_frame_sources": (3, 2, 2, 35, 16),
    "shared_sources": (3, 2, 1, 35, 16),
    "c1024_hw64": (2, 2, 2, 64, 1024),          # 8 splits: the last size in_finalize takes
    "c1024_hw72": (2, 2, 1, 72, 1024),          # 9 splits: in_finalize2 with a ragged first batch
    "c1024_hw520": (2, 1, 1, 520, 1024),        # the 64-split cap (58 splits of 9 rows): in_finalize2
    "c24_hw27": (2, 2, 2, 27, 24),
    "hw1": (3, 2, 1, 1, 16),
}
PACK_CASES = {                                                                      # (S, B, H, W, L, nimg, Cp, coords, divisors)
    "face_coords_s3": (3, 2, 24, 20, 2, 3, 8, True, (255.0, 1.0, 255.0)),           # S*B = 6, no padding channel
    "face_no_coords": (1, 2, 24, 20, 2, 3, 8, False, None),                         # three padding channels
    "pose": (2, 1, 24, 20, 25, 3, 32, True, None),
    "label_only_face": (1, 2, 24, 20, 2, 0, 8, True, None),
    "label_only_pose": (1, 2, 24, 20, 25, 0, 32, True, None),
    "frame_192": (1, 2, 192, 192, 2, 3, 8, True, None),                             # 144 blocks of pixels per image: the loop (128 blocks) repeats
}
UPSAMPLE_SHAPES = [(1, 1, 1, 8), (1, 1, 9, 8), (2, 5, 1, 16), (1, 3, 72, 512)]      # (N, H, W, C); the last: 72 blocks per output row (64 launched)
INSTNORM_EDGES = {                                                                  # instnorm_case's (N, H, W, C, relu, resid, seed)
    "loop_fixed_quad": (64, 32, 32, 128, True, False, 0),       # 128 blocks of quads per image, 64 launched (4096 / N): two passes
    "loop_moving_quad": (4096, 10, 10, 24, True, False, 1),     # one block per image, three passes, the channel quad advances by 256 % 6 = 4
    "c2048": (2, 4, 4, 2048, False, False, 2),                  # statistics: blockIdx.z = 0, 1
    "c1040": (2, 4, 4, 1040, True, False, 3),                   # C / 4 = 260: four columns left to the second block
}
OPS_WITH_REFUSALS = ("warp_k_shared", "add_stats", "finalize_stats", "fuse_tail", "pack_input", "upsample2x_st")
