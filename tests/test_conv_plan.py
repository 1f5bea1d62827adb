"""CPU tier: the convolution launch planner (wacv23_tsnet_amd/csrc/conv_plan.hpp) on its own, through a small host driver
(tests/emu/plan_driver.cpp) -- nothing is launched.

(a) every convolution the forward runs at BASELINE.json's configurations, B = 1, 2, 4, 8, on 256 CUs, plans as the committed table
    tests/golden/conv_plan_table.json says (captured from the forward and checked against the kernel traces of the previous launch logic
    on an MI355X);
(b) the choices a frame's bits depend on -- family, tile rows, statistics tiling -- are the same in every batch, and so are the tile width
    and wave grid outside conv_h2 / conv_h2r (whose one-group tiles give the same bits: tests/test_emu_ops.py, tests/test_gpu_ops.py);
(c) the packed integers of the ABI (tile codes, tsnet_bench_conv's variant bits, tsnet_op_head's flags) decode as documented and
    undocumented values are refused;
(d) what the planner accepts is what is built: it agrees with op_cases.REQUEST_GRID (which the emulator and the GPU walk through the
    operator) entry by entry, and refuses every layer geometry the kernels cannot index."""
import json
import os
import subprocess

import pytest

import op_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "plan_driver.cpp")
HDR = os.path.join(ROOT, "wacv23_tsnet_amd", "csrc", "conv_plan.hpp")
TABLE = os.path.join(ROOT, "tests", "golden", "conv_plan_table.json")

SHAPE_KEYS = ("ks", "stride", "pad", "reflect", "cin", "cout", "npad", "kpad", "form", "N", "H", "W", "csplit", "transform", "nprod", "fin_counter")
PLAN_KEYS = ("family", "rows", "width", "side_by_side", "sched", "w1_chunk", "w1_tab2", "xcd_gn", "tpi", "tiles_m", "tiles_n", "fin")
FAMILIES = ("H2R", "G64", "H2", "H2S", "H2S32", "H2D", "W1")
SCHEDS = ("plain", "deep", "two_groups")
KERNEL_OWN, KERNEL_GENERAL, KERNEL_PATCH = 0, 1, 2
PLAIN, DEEP, TWO_GROUPS = 0, 1, 2


@pytest.fixture(scope="module")
def plan():
    out = os.path.join(ROOT, "tests", "emu", "_build", "plan_driver")
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in (SRC, HDR))):
        cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "amdclang++", "clang++")
                    if (os.path.isabs(c) and os.path.exists(c)) or
                    (not os.path.isabs(c) and subprocess.call(["which", c], stdout=subprocess.DEVNULL) == 0)), None)
        if cxx is None:
            pytest.skip("no clang++ available for the planner driver")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", out])

    def run(queries):
        r = subprocess.run([out], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True)
        return r.stdout.splitlines()
    return run


def _ints(line):
    assert not line.startswith("ERR"), line
    return [int(v) for v in line.split()]


def _plan_dict(line):
    v = dict(zip(PLAN_KEYS, _ints(line)))
    v["family"] = FAMILIES[v["family"]]
    v["sched"] = SCHEDS[v["sched"]]
    for k in ("side_by_side", "fin"):
        v[k] = bool(v[k])
    return v


def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_plan_table_of_the_forward(plan):
    t = _table()
    assert t["cus"] == 256
    cases = t["layers"]
    assert {c["config"] for c in cases} == {"cfg0/cfg1", "cfg2", "cfg3", "cfg4"}
    queries = ["P " + " ".join(str(int(c["shape"][k])) for k in SHAPE_KEYS) + f" {t['cus']}" for c in cases]
    got = plan(queries)
    assert len(got) == len(cases)
    for c, line in zip(cases, got):
        assert _plan_dict(line) == c["plan"], (c["config"], c["B"], c["layer"], c["shape"])


def test_plan_batch_independence(plan):
    """Family, tile rows and statistics tiling do not depend on the batch; the w1 chunk, the deep schedule, conv_h2's / conv_h2r's tile
    width and wave grid (and the head's rows, test_head_rows) may."""
    by_layer = {}
    for c in _table()["layers"]:
        by_layer.setdefault((c["config"], c["layer"]), []).append(c)
    for cfg in {k[0] for k in by_layer}:
        counts = {len(v) for k, v in by_layer.items() if k[0] == cfg}
        assert len(counts) == 1, cfg                                    # every batch runs the same layer list
    seen_batches = set()
    for (cfg, layer), cs in by_layer.items():
        seen_batches |= {c["B"] for c in cs}
        keep = {(c["plan"]["family"], c["plan"]["rows"], c["plan"]["tpi"]) for c in cs}
        assert len(keep) == 1, (cfg, layer, keep)
        if cs[0]["plan"]["family"] not in ("H2", "H2R"):
            assert len({(c["plan"]["width"], c["plan"]["side_by_side"]) for c in cs}) == 1, (cfg, layer)
        # the two-K-group form is never the forward's: another association of the chains
        assert all(c["plan"]["sched"] != "two_groups" for c in cs)
    assert seen_batches == {1, 2, 4, 8}


def test_plan_follows_the_cu_count(plan):
    """The CU count enters the batch-following heuristics only: the 256 tiles of a ResnetBlock layer at B = 4 fill 128 CUs in whole rounds
    of two-tile chunks but not 256 CUs; a single frame's stride-2 layer (128 tiles) runs the deep schedule while that is at most two
    workgroups per CU.  Family, tile and statistics tiling stay."""
    res = "P 3 1 1 1 512 512 512 6144 1 4 32 32 0 1 3 1 {}"          # a ResnetBlock layer (Winograd form), 4 images of 32 x 32
    s2 = "P 3 2 1 0 128 256 256 1152 0 1 128 128 0 1 3 1 {}"          # the 128 -> 256 stride-2 layer, one image
    r256, r128, d256, d32 = (_plan_dict(line) for line in plan([res.format(256), res.format(128), s2.format(256), s2.format(32)]))
    assert (r256["w1_chunk"], r128["w1_chunk"]) == (1, 2)
    assert d256["sched"] == "deep" and d32["sched"] == "plain"
    for a, b in ((r256, r128), (d256, d32)):
        assert {k: v for k, v in a.items() if k not in ("w1_chunk", "w1_tab2", "sched")} == {k: v for k, v in b.items() if k not in ("w1_chunk", "w1_tab2", "sched")}


def test_tile_codes(plan):
    # (kernel, tile) -> (kernel, rows, width, alt, sched, chunk)
    want = {
        (0, 0): (KERNEL_OWN, 0, 0, 0, PLAIN, 0),
        (0, 32): (KERNEL_OWN, 0, 32, 0, PLAIN, 0), (2, 64): (KERNEL_PATCH, 0, 64, 0, PLAIN, 0), (1, 128): (KERNEL_GENERAL, 0, 128, 0, PLAIN, 0),
        (2, 2128): (KERNEL_PATCH, 2, 128, 0, PLAIN, 0),
        (0, 3128): (KERNEL_OWN, 0, 128, 1, PLAIN, 0), (1, 3064): (KERNEL_GENERAL, 0, 64, 1, PLAIN, 0), (1, 3128): (KERNEL_GENERAL, 0, 128, 1, PLAIN, 0),
        (2, 12128): (KERNEL_PATCH, 2, 128, 0, DEEP, 0),
        (2, 20032): (KERNEL_PATCH, 4, 32, 0, TWO_GROUPS, 0), (0, 20064): (KERNEL_OWN, 4, 64, 0, TWO_GROUPS, 0),
        (3, 0): (KERNEL_OWN, 0, 0, 0, PLAIN, 0), (3, 1): (KERNEL_OWN, 0, 0, 0, PLAIN, 1), (3, 3): (KERNEL_OWN, 0, 0, 0, PLAIN, 3),
    }
    got = plan([f"T {k} {t}" for k, t in want])
    for (k, t), line in zip(want, got):
        v = _ints(line)
        assert (v[0], v[1], v[2], v[3], v[4], v[5]) == want[(k, t)], (k, t, v)
        assert v[6:] == [3, 0, 0, -1], (k, t, v)                     # chunk cap, no masks, the planner's XCD grid
    bad = [(0, 1), (0, 16), (0, 96), (0, 2064), (0, 4128), (0, 2000), (0, 4000), (0, 10064), (0, 30064), (0, 20128), (0, -64), (3, 4), (3, 64), (4, 0), (-1, 0)]
    for (k, t), line in zip(bad, plan([f"T {k} {t}" for k, t in bad])):
        assert line.startswith("ERR"), (k, t, line)


def test_bench_variant_bits(plan):
    # tile | general << 12 | bf16 << 13 | patch << 14 | Winograd form << 15 | ablation << 16 | cold << 21 | opt 32 << 22 | two groups << 23 | opt << 24 | XCD << 28
    cases = {
        -1: ([0, 0, 0, 0, 0, 0, 3, 0, 0, -1], 3, 0, 0),
        4096 | 3064: ([1, 0, 64, 1, 0, 0, 3, 0, 0, -1], 3, 0, 0),
        8192 | 16384 | 2128: ([2, 2, 128, 0, 0, 0, 3, 0, 0, -1], 1, 0, 0),
        32768 | 2 | (1 << 21): ([0, 0, 0, 0, 0, 2, 3, 0, 0, -1], 3, 1, 1),
        64 | (7 << 16) | (1 << 23) | (8 << 24) | (1 << 22): ([0, 0, 64, 0, 0, 0, 3, 7, 8 | 16 | 32, -1], 3, 0, 0),
        128 | (1 << 28): ([0, 0, 128, 0, 0, 0, 3, 0, 0, 0], 3, 0, 0),
        128 | (5 << 28): ([0, 0, 128, 0, 0, 0, 3, 0, 0, 8], 3, 0, 0),
        # deep prefetch + two K groups alone is the product's two-group schedule, not an experiment; with an ablation it stays a mask
        64 | (1 << 23) | (8 << 24): ([0, 0, 64, 0, TWO_GROUPS, 0, 3, 0, 0, -1], 3, 0, 0),
        64 | (1 << 16) | (1 << 23) | (8 << 24): ([0, 0, 64, 0, 0, 0, 3, 1, 24, -1], 3, 0, 0),
    }
    for v, line in zip(cases, plan([f"V {v}" for v in cases])):
        req, nprod, form, cold = cases[v]
        assert _ints(line) == req + [nprod, form, cold], (v, line)
    for v in (6 << 28, 32768 | 64, 4096 | 1000, 2000):
        assert plan([f"V {v}"])[0].startswith("ERR"), v


def test_head_flags_and_rows(plan):
    ok = {0: [0, 0], 1: [1, 0], 8 << 8: [0, 8], (16 << 8) | 1: [1, 16], 32 << 8: [0, 32]}
    for code, line in zip(ok, plan([f"C {c}" for c in ok])):
        assert _ints(line) == ok[code], (code, line)
    for code in (2, 0x80, 4 << 8, 24 << 8, 64 << 8, -1):
        assert plan([f"C {code}"])[0].startswith("ERR"), code
    # head_conv3 on 256^2 (8 column tiles): 32 rows from B = 4 on, 16 at B = 2, 8 for one frame; other CU counts scale the thresholds
    q = [f"H {b} 8 256 {cus}" for cus in (256, 128) for b in (1, 2, 4, 8)]
    assert [int(v) for v in plan(q)] == [8, 16, 32, 32, 16, 32, 32, 32]


def _request_query(e, shape=None, request=None):
    """the R query of a REQUEST_GRID entry; `request`: (kernel, rows, width, alt, sched, chunk, xcd_gn) instead of the entry's tile code"""
    return "R " + " ".join(str(v) for v in (shape or oc.request_shape(e)) + list(request))


def _requests_of(plan, entries):
    """decode_tile_code of every entry -> its request fields (None where the code itself is refused)"""
    out = []
    for e, line in zip(entries, plan([f"T {e['kernel']} {e['tile']}" for e in entries])):
        v = None if line.startswith("ERR") else _ints(line)
        out.append(None if v is None else v[:6] + [v[9]])
    return out


def test_request_grid(plan):
    """the planner agrees with op_cases.REQUEST_GRID entry by entry, and the combinations that used to plan a kernel that is not built are
    refused, each for its own reason"""
    grid = oc.REQUEST_GRID
    assert len(grid) == 7 * 4 * 3 * 13 and sum(e["accepted"] for e in grid) == 217
    reqs = _requests_of(plan, grid)
    live = [(e, r) for e, r in zip(grid, reqs) if r is not None]
    assert all(not e["accepted"] for e, r in zip(grid, reqs) if r is None)
    why = {}
    for (e, r), line in zip(live, plan([_request_query(e, request=r) for e, r in live])):
        assert (not line.startswith("ERR")) == e["accepted"], (e, line)
        why[(e["layer"], e["kernel"], e["tile"], e["nprod"])] = line
    gaps = {   # (layer, kernel, tile, nprod): a word of the refusal
        ("s1_c32", 2, 12128, 3): "deep schedule",                 # 2 x 128 deep on a 3 x 3 / stride-1 layer
        ("s1_c48", 2, 20032, 3): "even number", ("s1_c48", 2, 20064, 1): "even number",      # two K groups on three slabs
        ("s1_c32", 2, 20064, 4): "products", ("s1_c32", 2, 32, 4): "products", ("s1_c32", 2, 2128, 4): "products",
        ("s2_c16", 2, 64, 4): "products", ("stem_c8", 2, 0, 4): "products", ("stem_c32", 0, 0, 4): "products",
        ("s1_c32", 1, 64, 4): "products", ("p1_c64", 1, 3064, 4): "products", ("s1_c32", 3, 0, 4): "products",
        ("s2_c16", 2, 32, 3): "4x64", ("s2_c16", 2, 12128, 1): "fp16 x 2",
        ("stem_c8", 1, 128, 3): "128-wide", ("p1_c16", 1, 128, 3): "128-wide", ("stem_c32", 1, 128, 1): "128-wide",
    }
    for k, word in gaps.items():
        assert why[k].startswith("ERR") and word in why[k], (k, why[k])
    # requests no tile code spells: two rows at the planner's width (2 x 64 is not built), the side-by-side grid on two rows,
    # a 1 x 1 layer with 8 input channels on the general kernel
    s1, s2 = dict(layer="s1_c32", kernel=2, nprod=3), dict(layer="s2_c16", kernel=2, nprod=3)
    s1_64 = oc.request_shape(s1)
    s1_64[5] = s1_64[6] = 64                                   # 64 output channels: the planner's width is 64
    s2_64 = oc.request_shape(s2)
    s2_64[5] = s2_64[6] = 64
    p1_8 = oc.request_shape(dict(layer="p1_c16", kernel=1, nprod=3))
    p1_8[4], p1_8[7] = 8, 32
    s1_8 = oc.request_shape(dict(layer="s1_c32", kernel=1, nprod=3))
    s1_8[4], s1_8[7] = 8, 96                                   # a 3 x 3 layer with 8 input channels: no 128-wide tile of the general kernel
    w1 = dict(layer="s1_c32", kernel=3, nprod=3)               # the Winograd form takes no schedule
    q = [_request_query(s1, s1_64, (KERNEL_PATCH, 2, 0, 0, PLAIN, 0, -1)), _request_query(s2, s2_64, (KERNEL_PATCH, 2, 0, 0, PLAIN, 0, -1)),
         _request_query(dict(layer="s1_c32", kernel=2, nprod=1), None, (KERNEL_PATCH, 2, 128, 1, PLAIN, 0, -1)),
         _request_query(None, p1_8, (KERNEL_GENERAL, 0, 64, 0, PLAIN, 0, -1)), _request_query(None, s1_8, (KERNEL_GENERAL, 0, 128, 0, PLAIN, 0, -1)),
         _request_query(w1, None, (KERNEL_OWN, 0, 0, 0, TWO_GROUPS, 0, -1))]
    for line, word in zip(plan(q), ("4x32, 4x64", "4x64 (four waves)", "bf16 4 x 128", "1x1 layers", "128-wide", "conv(w1)")):
        assert line.startswith("ERR") and word in line, line


def test_geometry_is_refused_by_the_planner(plan):
    """the layer / tensor checks of conv_plan.hpp's validate_conv (run_conv keeps only what depends on pointers): each refuses through the driver, by name"""
    ok = dict(ks=3, stride=1, pad=1, reflect=1, cin=64, cout=64, npad=64, kpad=576, form=0, N=1, H=8, W=8, csplit=0, transform=0, nprod=3, fin_counter=0)
    bad = [(dict(ks=5, kpad=1600), "kernel size"), (dict(cin=24, kpad=224), "input channels"), (dict(H=0), "empty"), (dict(N=0), "empty"),
           (dict(ks=7, pad=3, H=3, kpad=3136), "reflection pad"), (dict(pad=8), "reflection pad"), (dict(csplit=24), "channel split"),
           (dict(csplit=64), "channel split"), (dict(N=64, H=512, W=512, cin=32, kpad=288), "32-bit"), (dict(N=32, H=1024, W=1024, cin=8, kpad=96), "32-bit"),
           (dict(cin=4112, kpad=37024), "transform table"), (dict(stride=0), "stride"), (dict(nprod=2), "products")]
    q = ["P " + " ".join(str({**ok, **d}[k]) for k in SHAPE_KEYS) + " 256" for d, _ in [({}, "")] + bad]
    got = plan(q)
    assert not got[0].startswith("ERR"), got[0]
    for (d, word), line in zip(bad, got[1:]):
        assert line.startswith("ERR") and word in line, (d, line)
    # the second tensor of a concat has its own extent: 16 of 48 channels from x, 32 from x2 with x2_nmod images
    cat = " ".join(str({**ok, "cin": 48, "kpad": 448, "csplit": 16, "N": 2, "H": 512, "W": 512}[k]) for k in SHAPE_KEYS) + f" 256 {KERNEL_OWN} 0 0 0 {PLAIN} 0 -1"
    few, many = plan([f"R {cat} 1", f"R {cat} 64"])
    assert not few.startswith("ERR") and many.startswith("ERR") and "32-bit" in many, (few, many)
