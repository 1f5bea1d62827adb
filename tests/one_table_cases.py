"""The cases that pin "one slot table for every forward": the kernels that read the encoded sources find a source image through the table
alone, and the two cache modes and the one-shot forward are tables the engine writes itself.  Only the ORIGIN of a source image's and a
mask's address changed; the arithmetic did not -- so every output below keeps the bits the commit before gave, when each kernel still had a
cache form (image s*SB + b % SB, masks (K, Bmax, H, W)) beside its slot form.  Shared by tools/probes/one_table_capture_bits.py (which
recorded tests/golden/one_table_parent_bits.npz with the emulation build of that commit), tests/test_one_table.py and the GPU tier's
tests/test_gpu_one_table.py.

forward_outputs: test_source_bank.py's narrow net (ngf 8, 32 x 32, K = 2, max_batch 3, n_blocks 1) through every way a forward can be
asked for; op_outputs: each of the five kernels through every spelling of its operator entry point; stale_table_sequence: the calls that
would show a device table left over from an earlier forward."""
import ctypes as C
import os

import torch

import compact_cases as cc
import helpers as Hh
import op_cases as oc
import test_source_bank as sb
from oracle import tsnet_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "one_table_parent_bits.npz")
LIMIT = 1000 * 1024          # a committed file stays under 1 MiB: the record is written in parts if it has to be
K, BMAX, H, W = sb.K, sb.BMAX, sb.H, sb.W


def part_path(i):
    return GOLDEN if i == 0 else GOLDEN.replace(".npz", f".part{i + 1}.npz")


def load_golden():
    import numpy as np
    rec, i = {}, 0
    while os.path.exists(part_path(i)):
        with np.load(part_path(i)) as z:
            rec.update({k: torch.from_numpy(z[k]) for k in z.files})
        i += 1
    return rec


def _named(out, name, res):
    """(rec, flows) of a forward -> entries name.rec, name.flow<s>"""
    rec, flows = res
    out[name + ".rec"] = rec.clone()
    for s, f in enumerate(flows):
        out[f"{name}.flow{s}"] = f.clone()


class Net:
    """the narrow net, a pool of seven sources of batch 1, BMAX driving frames, and the compact inputs of the B = 2 cases"""

    def __init__(self, n_blocks=1, ngf=8, size=(H, W), dev="cpu"):
        self.dev, (self.H, self.W) = dev, size
        if ngf == 8:
            self.cfg, self.sd = sb._net(nb=n_blocks)
        else:                                              # the GPU tier: smoke()'s shape, full widths
            self.cfg = O.TSNetConfig(label_nc=2, n_blocks=n_blocks, n_source=K)
            self.sd = O.synth_state_dict(self.cfg, seed=3, bias_std=0.02)
        pool_cfg = O.TSNetConfig(label_nc=2, n_blocks=0, n_source=7)       # (the inputs depend on n_source and label_nc alone)
        self.pool = tuple([t.to(dev) for t in part] for part in O.synth_inputs(pool_cfg, 1, *size, seed=4, mask_mode="bernoulli")[:3])
        self.tar_lbl, self.tar_bbox = (t.to(dev) for t in O.synth_inputs(self.cfg, BMAX, *size, seed=5, mask_mode="bernoulli")[3:])

    def engine(self, lib=None):
        return Hh.make_engine(self.cfg, self.sd, self.H, self.W, BMAX, self.dev, lib=lib)

    def src(self, ids):
        """sources of batch 1: pool entries `ids`"""
        return tuple([part[i] for i in ids] for part in self.pool)

    def batched(self, B):
        """K sources of batch B: source s of frame b is pool entry s*B + b"""
        return tuple([torch.cat(part[s * B:(s + 1) * B]) for s in range(K)] for part in self.pool)

    def tar(self, B):
        return self.tar_lbl[:B], self.tar_bbox[:B]

    def done(self, res):
        if torch.device(self.dev).type == "cuda":
            torch.cuda.synchronize()
        return res[0].cpu(), [f.cpu() for f in res[1]]


def forward_outputs(lib):
    """{name: tensor}: the image and every flow of each forward case, on the emulation build `lib`"""
    net, out = Net(), {}
    eng = net.engine(lib)
    for B in (3, 1):
        _named(out, f"one_shot_b{B}", eng.forward(*net.batched(B), *net.tar(B), return_flow=True))
    eng.set_sources(*net.batched(3))
    _named(out, "per_batch_b3", eng.forward_target(*net.tar(3), return_flow=True))
    eng.set_sources(*net.src([0, 1]), shared=True)
    for B in (3, 2):
        _named(out, f"shared_b{B}", eng.forward_target(*net.tar(B), return_flow=True))
    eng.bank_put(2, *net.src([2, 3, 4, 5]))
    eng.bank_put([0, 1], *net.src([0, 1]))
    _named(out, "bank", eng.forward_bank(sb.TABLE, *net.tar(3), return_flow=True))
    # compact (uint8) inputs at B = 2: the only path on which the packing kernel writes the masks into the engine's copy itself
    inp = cc.Inputs(2, K, 2, H, W, seed=21)
    _named(out, "u8_one_shot_b2", eng.forward(*inp.c, return_flow=True, mean=cc.MEAN))
    eng.set_sources(*inp.src("c"), mean=cc.MEAN)
    _named(out, "u8_per_batch_b2", eng.forward_target(*inp.tar("c"), return_flow=True))
    eng.set_sources(*inp.src("c", b=1), shared=True, mean=cc.MEAN)
    _named(out, "u8_shared_b2", eng.forward_target(*inp.tar("c"), return_flow=True))
    eng.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
def _ok(lib, rc):
    assert rc == 0, lib.tsnet_op_last_error().decode()


def _add_stats(lib, x, add, N, HW, Cc, call):
    y, al, be = torch.full((N, HW, Cc), float("nan")), torch.full((N * Cc,), float("nan")), torch.full((N * Cc,), float("nan"))
    _ok(lib, call(y.data_ptr(), al.data_ptr(), be.data_ptr()))
    return torch.cat([y.flatten(), al, be])


def op_outputs(lib):
    """{name: tensor}: every spelling of the five operator families, on the shapes their _shared / _slots tests use"""
    out, dev = {}, "cpu"
    OB, OK, NSRC, OH, OW, OC, TAB = sb.OB, sb.OK, sb.NSRC, sb.OH, sb.OW, sb.OC, sb.OP_TABLE
    # warp: tsnet_op_warp, _warp_k, _warp_k_shared (SB = 1, SB = B), _warp_k_slots
    for e, y in zip(("one", "k", "shared"), oc.warp_one_source_entries(lib, dev, 2, 7, 9, 16)):
        out[f"warp.k1.{e}"] = y
    out["warp.shared.sb1"], out["warp.shared.sbB"], _ = oc.warp_k_shared_case(lib, dev, 3, 2, 7, 9, 16)
    src, flow = oc.warp_k_inputs(3, 2, 7, 9, 16, 3, seed=1)
    out["warp.k"] = oc.run_warp_k(lib, dev, src, flow, 3, 2, 3, entry="k")
    _, flow = oc.warp_k_inputs(OB, OK, OH, OW, OC, 1, seed=11)
    pool = oc._rand(11, "pool", (NSRC, OC, OH, OW), -2, 2)
    y = torch.full((OB, OH, OW, OC), float("nan"))
    _ok(lib, lib.tsnet_op_warp_k_slots(oc.nhwc(pool).data_ptr(), flow.data_ptr(), OB, OK, OH, OW, OC, y.data_ptr(), sb._ints(TAB), NSRC, None))
    out["warp.slots"] = y
    # fuse_tail: tsnet_op_fuse_tail (SB = 1, SB = B), _fuse_tail_slots
    out["fuse_tail.sb1"], out["fuse_tail.sbB"], _ = oc.fuse_tail_shared_case(lib, dev, 3, 2, 7 * 9, 16)
    P = OH * OW
    _, tar, y2, al, be = oc.fuse_tail_inputs(OB, OK, P, OC, 1, seed=12)
    pool = oc._rand(12, "pool", (NSRC, P, OC), -2, 2)
    z = torch.full((OB, P, 2 * OC), float("nan"))
    _ok(lib, lib.tsnet_op_fuse_tail_slots(*[t.data_ptr() for t in (pool, tar, y2, al, be)], OB, OK, P, OC, z.data_ptr(), sb._ints(TAB), NSRC, None))
    out["fuse_tail.slots"] = z
    # add_stats: tsnet_op_add_stats (x_sb = add_nmod, x_sb = 1), _add_stats_slots: y | alpha | beta
    for name in ("per_frame_sources", "shared_sources", "hw1"):
        Kk, B, x_sb, HW, Cc = oc.ADD_STATS_CASES[name]
        x, add = oc._rand(0, "x", (Kk * x_sb, HW, Cc), -2, 2), oc._rand(0, "add", (B, HW, Cc), -2, 2)
        out[f"add_stats.{name}"] = _add_stats(lib, x, add, Kk * B, HW, Cc, lambda *o: lib.tsnet_op_add_stats(
            x.data_ptr(), add.data_ptr(), B, x_sb, Kk * B, HW, Cc, *o, None))
    x, add = oc._rand(13, "pool", (NSRC, P, OC), -2, 2), oc._rand(13, "add", (OB, P, OC), -2, 2)
    out["add_stats.slots"] = _add_stats(lib, x, add, OK * OB, P, OC, lambda *o: lib.tsnet_op_add_stats_slots(
        x.data_ptr(), add.data_ptr(), OB, OK * OB, P, OC, *o, sb._ints(TAB), NSRC, None))
    # flow: tsnet_op_flow, _flow_k and _flow_k_slots on a small map with 64 and with 32 targets per workgroup, and on the large map
    tar, src, mt, ms = sb._flow_inputs(OB, 1, OB, OH, OW, OC, seed=15)
    f = torch.full((OB, OH, OW, 2), float("nan"))
    _ok(lib, lib.tsnet_op_flow(tar.data_ptr(), src.data_ptr(), mt.data_ptr(), ms.data_ptr(), OB, OH, OW, OC, OH * 8, OW * 8, f.data_ptr(), None))
    out["flow.plain"] = f
    for name, args in (("small", (OB, OK, NSRC, OH, OW, OC, TAB, 0)), ("small_nt1", (2, 2, 3, 4, 6, 1024, [2, 0, 1, 1], 0)),
                       ("large", (1, 2, 3, 32, 64, 8, [2, 0], 0)), ("large_forced", (1, 2, 3, 32, 64, 8, [2, 0], 1))):
        out[f"flow.slots.{name}"], out[f"flow.k.{name}"] = sb._flow_pair(lib, *args)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
STALE_TABLE = [[1, 4], [4, 0], [0, 0]]      # a permuted table on the bank of step 4


def stale_table_steps(net):
    """[(name, what to run first on the engine, the forward)]: every step's table differs from the one before it in content or in length,
    or (step 5) is the same on purpose -- an engine that kept an earlier table on the device would show it here"""
    put = lambda e: (e.bank_put(2, *net.src([2, 3, 4, 5])), e.bank_put([0, 1], *net.src([0, 1])))
    bank = lambda e: e.forward_bank(STALE_TABLE, *net.tar(3), return_flow=True)
    return [
        ("one_shot_b2", None, lambda e: e.forward(*net.batched(2), *net.tar(2), return_flow=True)),
        ("shared_b3", lambda e: e.set_sources(*net.src([0, 1]), shared=True), lambda e: e.forward_target(*net.tar(3), return_flow=True)),
        ("shared_b1", None, lambda e: e.forward_target(*net.tar(1), return_flow=True)),
        ("bank", put, bank),
        ("bank_again", None, bank),
        ("per_batch_b2", lambda e: e.set_sources(*net.batched(2)), lambda e: e.forward_target(*net.tar(2), return_flow=True)),
        ("one_shot_b1", None, lambda e: e.forward(*net.batched(1), *net.tar(1), return_flow=True)),
    ]


def check_stale_table(net, lib=None):
    """the sequence on ONE engine; every result against the same call on a fresh engine (which gets what the step builds on -- the sources
    of the step that set them -- and nothing else)"""
    steps = stale_table_steps(net)
    eng, got = net.engine(lib), []
    for name, prep, run in steps:
        if prep:
            prep(eng)
        got.append(net.done(run(eng)))
    eng.close()
    preps = []
    for i, (name, prep, run) in enumerate(steps):
        preps = [prep] if prep else (preps if name in ("shared_b1", "bank_again") else [])
        fresh = net.engine(lib)
        for p in preps:
            p(fresh)
        want = net.done(run(fresh))
        fresh.close()
        assert torch.isfinite(want[0]).all() and cc.same(got[i], want), name
    assert not torch.equal(got[1][0][:1], got[0][0][:1])         # (the steps do differ: shared sources against per-frame ones)
