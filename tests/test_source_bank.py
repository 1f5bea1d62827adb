"""CPU tier: the source bank (tsnet_bank_put / tsnet_forward_bank) under the fiber emulator, on test_shared_sources.py's narrow net (ngf = 8,
32 x 32).  The bank sees the source-side cache as n_source * max_batch slots of one encoded source each; every driving frame of a forward
names the slots it reads.  The acceptance criterion is exact: frame b of a bank forward carries the bits of the one-shot forward() at
B = 1 on (the sources it names, in the order it names them; frame b).  Every comparison below is torch.equal.

The operator cases at the end run each kernel of the indexed path through its own entry point (tsnet_op_*_slots) against its sibling on
inputs gathered by hand with torch.index_select."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import helpers as Hh
import op_cases as oc
from oracle import tsnet_oracle as O
from wacv23_tsnet_amd import prng

K, BMAX, H, W = 2, 3, 32, 32
TABLE = [[4, 1], [1, 4], [0, 0]]        # a permuted order, a slot shared across frames, a duplicate inside a frame


def _net(n_source=K, nb=1, seed=3, wscale=4.0):
    cfg = O.TSNetConfig(label_nc=2, n_blocks=nb, n_source=n_source, ngf=8, enc_blocks=2, fuse_ngf=128)
    sd = O.synth_state_dict(cfg, seed=seed, bias_std=0.02)
    return cfg, {k: (v * wscale if k.endswith("weight") else v) for k, v in sd.items()}     # non-trivial activations at width 8


def _pool(n, seed=4):
    """n distinct sources of batch 1 -- image, label map and (Bernoulli: all different) bounding box each -- as three lists"""
    cfg = O.TSNetConfig(label_nc=2, n_blocks=0, n_source=n, ngf=8, enc_blocks=2, fuse_ngf=128)
    return O.synth_inputs(cfg, 1, H, W, seed=seed, mask_mode="bernoulli")[:3]


class Case:
    """One net, seven distinct sources (six for the slots, one to replace with), three driving frames, and the one-shot references --
    computed once per (sources, frame) on an engine of their own, so that the bank under test is never disturbed."""

    def __init__(self, lib, operands="fp32"):
        self.lib, self.operands = lib, operands
        self.cfg, self.sd = _net()
        self.pool = _pool(7)
        self.tar_lbl, self.tar_bbox = O.synth_inputs(self.cfg, BMAX, H, W, seed=5, mask_mode="bernoulli")[3:]
        self.ref_eng = Hh.make_engine(self.cfg, self.sd, H, W, BMAX, "cpu", lib=lib, operands=operands)
        self._refs = {}

    def engine(self, **kw):
        return Hh.make_engine(self.cfg, self.sd, H, W, BMAX, "cpu", lib=self.lib, operands=self.operands, **kw)

    def src(self, ids):
        return tuple([part[i] for i in ids] for part in self.pool)

    def ref(self, ids, b):
        """one-shot forward at B = 1 on the sources `ids` (pool indices, in order) and driving frame b: (rec, flows)"""
        key = (tuple(ids), b)
        if key not in self._refs:
            self._refs[key] = Hh.run_engine(self.ref_eng, (*self.src(ids), self.tar_lbl[b:b + 1], self.tar_bbox[b:b + 1]), "cpu")
        return self._refs[key]

    def fill(self, eng, content=range(6)):
        """slot j <- source content[j], in two calls: slots 2-5, then 0-1"""
        content = list(content)
        eng.bank_put(2, *self.src(content[2:6]))
        eng.bank_put([0, 1], *self.src(content[0:2]))

    def check(self, eng, table, content, frames=None, want_flow=True):
        """forward_bank(table) on driving frames `frames`; every frame against its one-shot reference.  Returns (rec, flows)."""
        frames = list(range(len(table))) if frames is None else frames
        rec, flows = eng.forward_bank(table, self.tar_lbl[frames], self.tar_bbox[frames], return_flow=want_flow)
        assert rec.shape[0] == len(frames) and (not want_flow or len(flows) == len(table[0]))
        for i, b in enumerate(frames):
            r, f = self.ref([content[j] for j in table[i]], b)
            assert torch.equal(rec[i:i + 1], r), (i, b)
            if want_flow:
                assert all(torch.equal(x[i:i + 1], y) for x, y in zip(flows, f)), (i, b)
        return rec, flows

    def close(self):
        self.ref_eng.close()


@pytest.fixture(scope="module")
def case(emu_lib):
    c = Case(emu_lib)
    yield c
    c.close()


def test_mixed_table_equals_one_shot_forwards(case):
    """Six distinct sources in six slots, B = 3, the table [[4,1],[1,4],[0,0]].  Frames 0 and 1 name the same two slots in opposite order:
    the order is honoured if flow s of a frame is the flow of the s-th source it names, which differs from the flow of the other one.  (At
    K = 2 the image itself cannot tell the order: the mean is (0 + a) + b against (0 + b) + a, the same fp32 number.  The GPU tier's
    K = 3 table can.)"""
    eng = case.engine()
    assert eng.bank_capacity == K * BMAX == 6
    case.fill(eng)
    rec, flows = case.check(eng, TABLE, list(range(6)))
    for b, other in ((0, 1), (1, 0)):
        assert not torch.equal(rec[b:b + 1], case.ref(TABLE[other], other)[0])
        swapped = case.ref(TABLE[other], b)[1]                       # the same frame, the sources in the other frame's order
        assert not torch.equal(flows[0][b:b + 1], swapped[0]) and torch.equal(flows[0][b:b + 1], swapped[1])
    assert eng.stage("src_fea", "cpu").shape[0] == 6                 # every slot
    eng.close()


def test_tables_of_the_two_cache_modes(case):
    """The table s for every b is the shared cache; the table s*B + b, on sources put slot by slot, is the per-batch cache."""
    eng = case.engine()
    case.fill(eng)
    got = eng.forward_bank([[0, 1]] * BMAX, case.tar_lbl, case.tar_bbox, return_flow=True)
    case.ref_eng.set_sources(*case.src([0, 1]), shared=True)
    want = case.ref_eng.forward_target(case.tar_lbl, case.tar_bbox, return_flow=True)
    assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    for j in (3, 0, 5, 1, 4, 2):                                     # one slot per call, in no particular order
        eng.bank_put(j, *case.src([j]))
    got = eng.forward_bank([[s * BMAX + b for s in range(K)] for b in range(BMAX)], case.tar_lbl, case.tar_bbox, return_flow=True)
    batched = tuple([torch.cat(part[s * BMAX:(s + 1) * BMAX]) for s in range(K)] for part in case.src(range(6)))
    want = Hh.run_engine(case.ref_eng, (*batched, case.tar_lbl, case.tar_bbox), "cpu")
    assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    eng.close()


def test_replacing_a_slot_changes_only_its_readers(case):
    eng = case.engine()
    case.fill(eng)
    before, _ = case.check(eng, TABLE, list(range(6)))
    eng.bank_put(1, *case.src([6]))
    content = [0, 6, 2, 3, 4, 5]
    after, _ = case.check(eng, TABLE, content)                       # frames 0 and 1 read slot 1: they equal the new references
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])
    assert torch.equal(after[2], before[2])                          # frame 2 does not: same bits
    eng.close()


def test_ragged_batches_against_one_bank(case):
    eng = case.engine()
    case.fill(eng)
    case.check(eng, TABLE[1:2], list(range(6)), frames=[1])
    case.check(eng, [TABLE[2], TABLE[0]], list(range(6)), frames=[2, 0])
    case.check(eng, TABLE, list(range(6)), want_flow=False)
    eng.close()


def test_fewer_sources_than_the_engine_holds(case, emu_lib):
    """Kc = 1 on the engine with n_source = 2 equals an engine created with n_source = 1 (the means divide by Kc)."""
    eng = case.engine()
    case.fill(eng)
    rec, flows = eng.forward_bank([[3], [0]], case.tar_lbl[:2], case.tar_bbox[:2], return_flow=True)
    cfg1, sd1 = _net(n_source=1)
    one = Hh.make_engine(cfg1, sd1, H, W, 1, "cpu", lib=emu_lib)
    assert len(flows) == 1
    for b, j in enumerate((3, 0)):
        r, f = Hh.run_engine(one, (*case.src([j]), case.tar_lbl[b:b + 1], case.tar_bbox[b:b + 1]), "cpu")
        assert torch.equal(rec[b:b + 1], r) and torch.equal(flows[0][b:b + 1], f[0])
    one.close()
    eng.close()


@pytest.mark.parametrize("operands", ["bf16", "bf16s", "fp16"])
def test_operand_modes(emu_lib, operands):
    c = Case(emu_lib, operands)
    eng = c.engine()
    c.fill(eng)
    c.check(eng, TABLE, list(range(6)))
    eng.close()
    c.close()


def test_state_rules(case):
    eng = case.engine()
    tl, tb = case.tar_lbl, case.tar_bbox
    # no bank yet
    with pytest.raises(RuntimeError, match="no source bank"):
        eng.forward_bank([[0, 1]], tl[:1], tb[:1])
    # slots outside the bank, in a put and in a table; slots not filled
    with pytest.raises(RuntimeError, match=r"slots 5 \.\. 6 are outside the bank \(capacity 6\)"):
        eng.bank_put(5, *case.src([0, 1]))
    eng.bank_put(2, *case.src([2, 3]))
    with pytest.raises(RuntimeError, match=r"slot 6 is outside the bank \(capacity 6\)"):
        eng.forward_bank([[2, 6]], tl[:1], tb[:1])
    with pytest.raises(RuntimeError, match="slot -1 is outside the bank"):
        eng.forward_bank([[-1, 2]], tl[:1], tb[:1])
    with pytest.raises(RuntimeError, match="slot 4 is not filled"):
        eng.forward_bank([[2, 3], [3, 4]], tl[:2], tb[:2])
    # Kc and B out of range
    with pytest.raises(RuntimeError, match="sources per frame outside 1..n_source"):
        eng.forward_bank([[2, 3, 2]], tl[:1], tb[:1])
    with pytest.raises(RuntimeError, match="max_batch"):
        eng.forward_bank([[2, 3]] * 4, tl[[0, 1, 2, 0]], tb[[0, 1, 2, 0]])
    # the wrapper validates the index: shape and dtype
    with pytest.raises(ValueError, match=r"shape \(B, Kc\)"):
        eng.forward_bank([[2, 3]], tl[:2], tb[:2])
    with pytest.raises(ValueError, match=r"shape \(B, Kc\)"):
        eng.forward_bank([2, 3], tl[:2], tb[:2])
    with pytest.raises(ValueError, match="integers"):
        eng.forward_bank(torch.tensor([[2.0, 3.0]]), tl[:1], tb[:1])
    with pytest.raises(ValueError, match="named twice"):
        eng.bank_put([1, 1], *case.src([0, 1]))
    # forward_target after a put: the bank is no per-batch cache
    with pytest.raises(RuntimeError, match="batch differs from the cached sources"):
        eng.forward_target(tl[:1], tb[:1])
    # train_extras is refused after a bank forward, as after one on a shared source set
    case.check(eng, [[2, 3]], list(range(6)), frames=[0])
    with pytest.raises(RuntimeError, match="source bank"):
        eng.train_extras(case.pool[0][2:4], case.pool[0][2])
    # the legacy calls drop the bank (they overwrite its buffers); the first put afterwards starts an EMPTY one
    for drop in ("set_sources", "set_sources_shared", "set_source_divisors", "forward"):
        eng.bank_put(2, *case.src([2, 3]))
        if drop == "set_sources":
            eng.set_sources(*case.src([0, 1]))
        elif drop == "set_sources_shared":
            eng.set_sources(*case.src([0, 1]), shared=True)
        elif drop == "set_source_divisors":
            eng.set_source_divisors(None)
        else:
            Hh.run_engine(eng, (*case.src([0, 1]), tl[:1], tb[:1]), "cpu")
            eng.train_extras(case.pool[0][0:2], case.pool[0][0])         # ... and train_extras is accepted again after a one-shot forward
        with pytest.raises(RuntimeError, match="no source bank"):
            eng.forward_bank([[2, 3]], tl[:1], tb[:1])
        eng.bank_put(0, *case.src([0]))
        with pytest.raises(RuntimeError, match="slot 2 is not filled"):
            eng.forward_bank([[0, 2]], tl[:1], tb[:1])
    # per-source divisors of a put: what set_source_divisors is to the caches
    eng.bank_put([4, 5], *case.src([4, 5]), divisors=[1.0, 255.0])
    rec, _ = eng.forward_bank([[4, 5]], tl[:1], tb[:1])
    case.ref_eng.set_source_divisors([1.0, 255.0])
    want, _ = Hh.run_engine(case.ref_eng, (*case.src([4, 5]), tl[:1], tb[:1]), "cpu")
    case.ref_eng.set_source_divisors(None)
    assert torch.equal(rec, want) and not torch.equal(rec, case.ref([4, 5], 0)[0])
    with pytest.raises(RuntimeError, match="divisors must be positive"):
        eng.bank_put(0, *case.src([0]), divisors=[0.0])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# one operator at a time: B = 3 driving frames, K = 2 sources per frame, four source images; every pair names its image in a table
OB, OK, NSRC, OH, OW, OC = 3, 2, 4, 8, 8, 16
OP_TABLE = [2, 1, 3, 3, 1, 2]           # entry k*B + b: frames 0 and 2 read images 2 and 3 in opposite order, frame 1 reads image 1 twice, image 0 is idle


def _ints(v):
    return (C.c_int * len(v))(*v)


def _sel(t, table):
    return torch.index_select(t, 0, torch.tensor(table)).contiguous()


def test_op_warp_slots_equals_gathered_sibling(emu_lib):
    src, flow = oc.warp_k_inputs(OB, OK, OH, OW, OC, 1, seed=11)          # (K, C, h, w): replaced by a pool of NSRC images
    src = oc._rand(11, "pool", (NSRC, OC, OH, OW), -2, 2)
    want = oc.run_warp_k(emu_lib, "cpu", _sel(src, OP_TABLE), flow, OB, OK, OB)
    out = torch.full((OB, OH, OW, OC), float("nan"))
    rc = emu_lib.tsnet_op_warp_k_slots(oc.nhwc(src).data_ptr(), flow.data_ptr(), OB, OK, OH, OW, OC, out.data_ptr(), _ints(OP_TABLE), NSRC, None)
    assert rc == 0, emu_lib.tsnet_op_last_error().decode()
    assert torch.equal(oc.nchw(out), want)
    assert not torch.equal(oc.nchw(out), oc.run_warp_k(emu_lib, "cpu", _sel(src, [0, 1, 2, 3, 0, 1]), flow, OB, OK, OB))    # the table matters
    assert emu_lib.tsnet_op_warp_k_slots(oc.nhwc(src).data_ptr(), flow.data_ptr(), OB, OK, OH, OW, OC, out.data_ptr(), _ints([0, 1, 2, 3, 4, 0]), NSRC, None) == -1
    assert "slot 4 is outside the 4 source images" in emu_lib.tsnet_op_last_error().decode()


def test_op_fuse_tail_slots_equals_gathered_sibling(emu_lib):
    P = OH * OW
    _, tar, y2, al, be = oc.fuse_tail_inputs(OB, OK, P, OC, 1, seed=12)
    src = oc._rand(12, "pool", (NSRC, P, OC), -2, 2)
    want = oc.run_fuse_tail(emu_lib, "cpu", _sel(src, OP_TABLE), tar, y2, al, be, OB, OK, OB)
    z = torch.full((OB, P, 2 * OC), float("nan"))
    rc = emu_lib.tsnet_op_fuse_tail_slots(*[t.data_ptr() for t in (src, tar, y2, al, be)], OB, OK, P, OC, z.data_ptr(), _ints(OP_TABLE), NSRC, None)
    assert rc == 0, emu_lib.tsnet_op_last_error().decode()
    assert torch.equal(z, want)
    assert emu_lib.tsnet_op_fuse_tail_slots(*[t.data_ptr() for t in (src, tar, y2, al, be)], OB, OK, P, OC, z.data_ptr(), _ints([-1] * 6), NSRC, None) == -1


def test_op_add_stats_slots_equals_gathered_sibling(emu_lib):
    HW, N = OH * OW, OK * OB
    x = oc._rand(13, "pool", (NSRC, HW, OC), -2, 2)
    add = oc._rand(13, "add", (OB, HW, OC), -2, 2)

    def run(fn, *tail):
        y, al, be = torch.full((N, HW, OC), float("nan")), torch.full((N * OC,), float("nan")), torch.full((N * OC,), float("nan"))
        rc = fn(y.data_ptr(), al.data_ptr(), be.data_ptr(), *tail)
        assert rc == 0, emu_lib.tsnet_op_last_error().decode()
        return y, al, be
    xg = _sel(x, OP_TABLE)
    want = run(lambda *o: emu_lib.tsnet_op_add_stats(xg.data_ptr(), add.data_ptr(), OB, OB, N, HW, OC, *o, None))
    got = run(lambda *o: emu_lib.tsnet_op_add_stats_slots(x.data_ptr(), add.data_ptr(), OB, N, HW, OC, *o, _ints(OP_TABLE), NSRC, None))
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(got[0], xg + add.repeat(OK, 1, 1))                # one IEEE addition per element


def _flow_inputs(B, K, n_src, h, w, Cc, seed):
    Hh_, Ww = h * 8, w * 8
    tar = F.relu(oc._rand(seed, "tar", (B, Cc, h, w), -1, 1))
    src = oc._rand(seed, "pool", (n_src, Cc, h, w), -1, 1) * 3
    src.view(n_src, Cc, -1)[:, :, ::3] += 4.0 * tar.view(B, Cc, -1)[[i % B for i in range(n_src)]][:, :, ::3]     # some dominant sources
    return oc.nhwc(tar), oc.nhwc(src), prng.bernoulli(seed, "mt", (B, Hh_, Ww)), prng.bernoulli(seed, "ms", (n_src, Hh_, Ww))


def _flow_pair(lib, B, K, n_src, h, w, Cc, table, variant, seed=14):
    tar, src, mt, ms = _flow_inputs(B, K, n_src, h, w, Cc, seed)
    sg, mg = _sel(src, table), _sel(ms, table)
    want, got = torch.full((K * B, h, w, 2), float("nan")), torch.full((K * B, h, w, 2), float("nan"))
    rc = lib.tsnet_op_flow_k(tar.data_ptr(), sg.data_ptr(), mt.data_ptr(), mg.data_ptr(), B, K, h, w, Cc, h * 8, w * 8, want.data_ptr(), variant, 1, None, None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    rc = lib.tsnet_op_flow_k_slots(tar.data_ptr(), src.data_ptr(), mt.data_ptr(), ms.data_ptr(), B, K, h, w, Cc, h * 8, w * 8, got.data_ptr(), variant, 1, None,
                                   _ints(table), n_src, None)
    assert rc == 0, lib.tsnet_op_last_error().decode()
    return got, want


@pytest.mark.parametrize("variant", [0, 1])
def test_op_flow_slots_small_map_equals_gathered_sibling(emu_lib, variant):
    """flow_kernel's slot instantiation: the source planes AND the source mask of a pair come from its slot"""
    got, want = _flow_pair(emu_lib, OB, OK, NSRC, OH, OW, OC, OP_TABLE, variant)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    other, _ = _flow_pair(emu_lib, OB, OK, NSRC, OH, OW, OC, [0, 1, 2, 3, 0, 1], variant)
    assert not torch.equal(other, want)


def test_op_flow_slots_large_map_equals_gathered_sibling(emu_lib):
    """flow_kernel_p's slot instantiation (maps of >= 2048 positions): 32 x 64 positions, the smallest map the plan sends there"""
    assert emu_lib.tsnet_flow_plan(1, 32, 64, 8) >= 1
    got, want = _flow_pair(emu_lib, 1, 2, 3, 32, 64, 8, [2, 0], 0)
    assert torch.isfinite(want).all() and torch.equal(got, want)
    forced, _ = _flow_pair(emu_lib, 1, 2, 3, 32, 64, 8, [2, 0], 1)      # variant 1: flow_kernel on the same map, wherever the sibling can force it
    assert (forced - want).abs().max().item() < 5e-5
