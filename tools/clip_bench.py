"""GPU box: clip-mode throughput: the K source frames are encoded once
(tsnet_set_sources), every driving frame then costs only tsnet_forward_target.  Same cfg1 workload as bench.py.

    --shared            ONE source set of batch 1 for the B driving frames (tsnet_set_sources_shared): K encoded images instead of K * B
    --compare ROUNDS    one process, interleaved rounds of (a) the per-batch cache on replicated sources, (b) the shared cache, (c) a B = 1
                        loop over the same B frames; one JSON line with the per-round figures, their medians and the spread of (a)
    --bank [--lib2 SO [--lib2-first]] [--rounds R]
                        the source bank (tsnet_bank_put / tsnet_forward_bank), one process, interleaved rounds, one JSON line:
                        (1) with --lib2 (another build of the same ABI, e.g. the parent commit's): the one-shot forward, forward_target on the
                            per-batch and on the shared cache and forward_bank (frame b on source set b) on both libraries, with each library's
                            own spread over the rounds; every case must give equal bits on the two ("lib2_bit_identical");
                            [--size N] [--sources K] [--operands MODE]: another frame size, source count, operand mode (BASELINE.json configs[4]:
                            --batch 1 --size 512 --sources 5 --operands bf16, the shape that runs flow_kernel_p);
                        (2) forward_bank with the identity table against forward_target on the shared cache;
                        (3) bank_put of ONE slot against a full set_sources (K = 3 images), and four source sets x one driving frame as one
                            forward_bank(B = 4) against four forward_bank(B = 1) calls
    --compact [--rounds R]
                        the input hand-off of a driving frame in both forms -- float32 (one-hot labels, float masks) and compact (class-map and mask
                        bytes, tsnet_forward_target_u8) -- at the face shape (L = 2) and the pose shape (L = 25, composite), B = 1 and B = 4, one
                        process, interleaved rounds, one JSON line: (a) the host -> device copy of the frames' inputs from pinned memory alone,
                        (b) that copy + forward_target on the shared cache; per driving frame, median and spread (max - min) over the rounds"""
import os, sys, time, json, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wacv23_tsnet_amd import synth
from wacv23_tsnet_amd.engine import TSNetEngine
B, H, W = 4, 256, 256
NB = int(sys.argv[sys.argv.index("--n-blocks") + 1]) if "--n-blocks" in sys.argv else 0
if "--batch" in sys.argv:
    B = int(sys.argv[sys.argv.index("--batch") + 1])
if "--size" in sys.argv:
    H = W = int(sys.argv[sys.argv.index("--size") + 1])


def bank_bench():
    import ctypes
    from wacv23_tsnet_amd import _lib
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    lib2 = sys.argv[sys.argv.index("--lib2") + 1] if "--lib2" in sys.argv else None
    K = int(sys.argv[sys.argv.index("--sources") + 1]) if "--sources" in sys.argv else 3
    operands = sys.argv[sys.argv.index("--operands") + 1] if "--operands" in sys.argv else "fp32"

    def engine(lib=None):
        e = TSNetEngine(label_nc=2, n_blocks=NB, n_downsampling=3, n_source=K, height=H, width=W, max_batch=B, operands=operands, lib=lib)
        e.load_state_dict(synth.state_dict(e.param_shapes(), seed=0)); e.finalize("cuda")
        return e

    dev = lambda x: [t.cuda() for t in x] if isinstance(x, list) else x.cuda()
    si, sl, sb, tl, tb = [dev(x) for x in synth.inputs(K, 2, B, H, W, seed=1)]                 # per-batch sources + B driving frames
    one = lambda ts, b=0: [t[b:b + 1] for t in ts]                                              # source set b, batch 1
    sets = [(one(si, b), one(sl, b), one(sb, b)) for b in range(B)]                             # B source sets ("identities") of K images

    def ms(step, N=20, warm=3):
        for _ in range(warm): step()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(N): step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / N * 1e3

    def table(runs):
        """{name: [ms per round]} -> {name: {median, spread (max - min over the rounds)}}"""
        return {k: {"median_ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "per_round_ms": [round(x, 4) for x in v]} for k, v in runs.items()}

    out = {"batch": B, "n_blocks": NB, "size": H, "sources": K, "operands": operands, "rounds": rounds, "lib2_first": "--lib2-first" in sys.argv}
    ident = [list(range(K))] * B
    mixed = [[K * b + s for s in range(K)] for b in range(B)]                                   # frame b on source set b
    eng = engine()
    # (1) legacy paths, this library against --lib2
    if lib2:
        engs = {"this": eng, "lib2": engine(_lib.bind(ctypes.CDLL(lib2)))}
        if "--lib2-first" in sys.argv:                       # which library goes first in a round: an order effect shows as a sign change
            engs = dict(reversed(list(engs.items())))
        def put_all(e):
            for b in range(B):
                e.bank_put(K * b, *sets[b])
        cases = {"forward": (lambda e: None, lambda e: e.forward(si, sl, sb, tl, tb)),
                 "per-batch forward_target": (lambda e: e.set_sources(si, sl, sb), lambda e: e.forward_target(tl, tb)),
                 "shared forward_target": (lambda e: e.set_sources(*sets[0], shared=True), lambda e: e.forward_target(tl, tb)),
                 "forward_bank": (put_all, lambda e: e.forward_bank(mixed, tl, tb))}
        runs = {f"{w} {k}": [] for w in cases for k in engs}
        same2 = True
        for r in range(rounds + 1):
            for w, (prep, step) in cases.items():
                res = {}
                for k, e in engs.items():
                    prep(e)
                    t = ms(lambda: step(e))
                    if r: runs[f"{w} {k}"].append(t)
                    res[k] = step(e)[0].clone()
                same2 = same2 and bool(torch.equal(res["this"], res["lib2"]))
        out["legacy_this_vs_lib2"] = table(runs)
        out["lib2_bit_identical"] = same2
        for w in cases:
            a, b = out["legacy_this_vs_lib2"][f"{w} this"], out["legacy_this_vs_lib2"][f"{w} lib2"]
            out["legacy_this_vs_lib2"][f"{w}: this - lib2, % of lib2"] = round((a["median_ms"] - b["median_ms"]) / b["median_ms"] * 100, 3)
            out["legacy_this_vs_lib2"][f"{w}: lib2 spread, % of its median"] = round(b["spread_ms"] / b["median_ms"] * 100, 3)
        engs["lib2"].close()
    # (2) identity table against the shared cache, (3) the use cases
    runs = {n: [] for n in ("shared forward_target", "forward_bank identity", "set_sources shared (K images)", "bank_put one slot",
                            "forward_bank B=4, 4 source sets", "4 x forward_bank B=1")}
    same = True
    for r in range(rounds + 1):
        eng.set_sources(*sets[0], shared=True)
        t = {"shared forward_target": ms(lambda: eng.forward_target(tl, tb))}
        want = eng.forward_target(tl, tb)[0].clone()
        t["set_sources shared (K images)"] = ms(lambda: eng.set_sources(*sets[0], shared=True))
        for b in range(B):
            eng.bank_put(K * b, *sets[b])
        t["forward_bank identity"] = ms(lambda: eng.forward_bank(ident, tl, tb))
        same = same and bool(torch.equal(eng.forward_bank(ident, tl, tb)[0], want))
        t["bank_put one slot"] = ms(lambda: eng.bank_put(1, *[x[1:2] for x in sets[0]]))
        t["forward_bank B=4, 4 source sets"] = ms(lambda: eng.forward_bank(mixed, tl, tb))
        t["4 x forward_bank B=1"] = ms(lambda: [eng.forward_bank(mixed[b:b + 1], tl[b:b + 1], tb[b:b + 1]) for b in range(B)])
        a = eng.forward_bank(mixed, tl, tb)[0]
        same = same and all(bool(torch.equal(a[b:b + 1], eng.forward_bank(mixed[b:b + 1], tl[b:b + 1], tb[b:b + 1])[0])) for b in range(B))
        if r:
            for n, v in t.items(): runs[n].append(v)
    out["bank"] = table(runs)
    m = lambda n: out["bank"][n]["median_ms"]
    out["bank"]["identity - shared, % of shared"] = round((m("forward_bank identity") - m("shared forward_target")) / m("shared forward_target") * 100, 3)
    out["bank"]["shared spread, % of its median"] = round(out["bank"]["shared forward_target"]["spread_ms"] / m("shared forward_target") * 100, 3)
    out["bank"]["set_sources / bank_put one slot"] = round(m("set_sources shared (K images)") / m("bank_put one slot"), 3)
    out["bank"]["4 x B=1 / one B=4"] = round(m("4 x forward_bank B=1") / m("forward_bank B=4, 4 source sets"), 3)
    out["bit_identical"] = same
    print(json.dumps(out))


def compact_bench():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    K, mean = 3, [101.84807705937696, 112.10832843463207, 111.65973036298041]
    out = {"n_blocks": NB, "rounds": rounds, "unit": "us per driving frame", "shapes": {}}
    g = torch.Generator().manual_seed(1)
    for shape, L, pose in (("face", 2, False), ("pose", 25, True)):
        eng = TSNetEngine(label_nc=L, n_blocks=NB, n_downsampling=3, n_source=K, height=H, width=W, max_batch=4, pose_composite=pose)
        eng.load_state_dict(synth.state_dict(eng.param_shapes(), seed=0)); eng.finalize("cuda")
        rnd8 = lambda shp, hi: torch.randint(0, hi, shp, generator=g, dtype=torch.uint8)
        onehot = lambda c: torch.stack([(c == j) for j in range(L)], dim=1).float()
        si, sl, sb = [rnd8((1, 3, H, W), 256) for _ in range(K)], [rnd8((1, H, W), L) for _ in range(K)], [rnd8((1, H, W), 2) for _ in range(K)]
        eng.set_sources([t.cuda() for t in si], [t.cuda() for t in sl], [t.cuda() for t in sb], shared=True, mean=mean)
        res = {}
        for B in (1, 4):
            tl8, tb8 = rnd8((B, H, W), L), rnd8((B, H, W), 2)
            host = {"compact": (tl8.pin_memory(), tb8.pin_memory()), "float32": (onehot(tl8).pin_memory(), tb8.float().pin_memory())}
            devt = {k: tuple(torch.empty(t.shape, dtype=t.dtype, device="cuda") for t in v) for k, v in host.items()}
            nbytes = {k: sum(t.numel() * t.element_size() for t in v) // B for k, v in host.items()}

            def upload(k):
                for d, h_ in zip(devt[k], host[k]):
                    d.copy_(h_, non_blocking=True)

            def timed(step, N=200, warm=20):
                for _ in range(warm): step()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(N): step()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / N / B * 1e6
            legs = {(k, w): [] for k in host for w in ("upload", "upload + forward_target")}
            for r in range(rounds + 1):
                for k in host:
                    a_ = timed(lambda: upload(k))
                    b_ = timed(lambda: (upload(k), eng.forward_target(*devt[k])))
                    if r:
                        legs[(k, "upload")].append(a_); legs[(k, "upload + forward_target")].append(b_)
            upload("compact"); upload("float32")
            same = bool(torch.equal(eng.forward_target(*devt["compact"])[0], eng.forward_target(*devt["float32"])[0]))
            res[f"B={B}"] = {"bytes_per_frame": nbytes, "bit_identical": same,
                             **{f"{k}: {w}": {"median_us": round(statistics.median(v), 2), "spread_us": round(max(v) - min(v), 2)} for (k, w), v in legs.items()}}
        out["shapes"][shape] = res
        eng.close()
    print(json.dumps(out))


if "--bank" in sys.argv:
    bank_bench()
    sys.exit(0)
if "--compact" in sys.argv:
    compact_bench()
    sys.exit(0)
SHARED = "--shared" in sys.argv
ROUNDS = int(sys.argv[sys.argv.index("--compare") + 1]) if "--compare" in sys.argv else 0
eng = TSNetEngine(label_nc=2, n_blocks=NB, n_downsampling=3, n_source=3, height=H, width=W, max_batch=B)
eng.load_state_dict(synth.state_dict(eng.param_shapes(), seed=0)); eng.finalize("cuda")
inp = synth.inputs(3, 2, 1 if (SHARED or ROUNDS) else B, H, W, seed=1)
si, sl, sb, _, _ = [[t.cuda() for t in x] if isinstance(x, list) else x.cuda() for x in inp]
tl, tb = [x.cuda() for x in synth.inputs(3, 2, B, H, W, seed=1)[3:]]
rep = lambda ts: [t.repeat(B, *([1] * (t.dim() - 1))) for t in ts]
one_set = si[0].shape[0] == 1                                  # sources of batch 1: the one-shot forward takes them replicated
full, _ = eng.forward(*( (rep(si), rep(sl), rep(sb)) if one_set else (si, sl, sb) ), tl, tb)
full = full.clone()


def measure(mode, N=30, warm=5):
    """(set_sources ms, forward_target ms per B frames, result).  a: per-batch cache, b: shared cache, c: per-batch cache at B = 1, B calls"""
    src = (rep(si), rep(sl), rep(sb)) if (mode == "a" and one_set) else (si, sl, sb)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    eng.set_sources(*src, shared=mode == "b")
    torch.cuda.synchronize(); t_src = time.perf_counter() - t0
    if mode == "c":
        step = lambda: torch.cat([eng.forward_target(tl[i:i + 1], tb[i:i + 1])[0] for i in range(B)])
    else:
        step = lambda: eng.forward_target(tl, tb)[0]
    for _ in range(warm): out = step()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(N): out = step()
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / N
    return t_src * 1e3, dt * 1e3, out


if ROUNDS:
    measure("a", N=5); measure("b", N=5); measure("c", N=5)    # first-call costs out of the way
    res = {m: {"set_sources_ms": [], "forward_target_ms": []} for m in "abc"}
    same = True
    for _ in range(ROUNDS):
        for m in "abc":
            s, f, out = measure(m)
            res[m]["set_sources_ms"].append(round(s, 3)); res[m]["forward_target_ms"].append(round(f, 3))
            same = same and bool(torch.equal(out, full))
    med = {m: {k: round(statistics.median(v), 3) for k, v in res[m].items()} for m in "abc"}
    fa = res["a"]["forward_target_ms"]
    print(json.dumps({"batch": B, "n_blocks": NB, "rounds": ROUNDS,
                      "modes": {"a": "per-batch cache, replicated sources", "b": "shared cache", "c": f"B=1 loop over the same {B} frames"},
                      "per_round": res, "median": med, "spread_a_forward_target_ms": round(max(fa) - min(fa), 3),
                      "b_minus_a_forward_target_ms": round(med["b"]["forward_target_ms"] - med["a"]["forward_target_ms"], 3),
                      "frames_per_s": {m: round(B / med[m]["forward_target_ms"] * 1e3, 1) for m in "abc"},
                      "b_over_c": round(med["c"]["forward_target_ms"] / med["b"]["forward_target_ms"], 3),
                      "bit_identical_to_full_forward": same}))
else:
    t_src, dt, out = measure("b" if SHARED else "a")
    print(json.dumps({"batch": B, "n_blocks": NB, "shared": SHARED, "set_sources_ms": round(t_src, 3), "forward_target_ms": round(dt, 3),
                      "clip_frames_per_s": round(B / dt * 1e3, 1), "bit_identical_to_full_forward": bool(torch.equal(out, full))}))
