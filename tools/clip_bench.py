"""GPU box: clip-mode throughput: the K source frames are encoded once
(tsnet_set_sources), every driving frame then costs only tsnet_forward_target.  Same cfg1 workload as bench.py.

    --shared            ONE source set of batch 1 for the B driving frames (tsnet_set_sources_shared): K encoded images instead of K * B
    --compare ROUNDS    one process, interleaved rounds of (a) the per-batch cache on replicated sources, (b) the shared cache, (c) a B = 1
                        loop over the same B frames; one JSON line with the per-round figures, their medians and the spread of (a)"""
import os, sys, time, json, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wacv23_tsnet_amd import synth
from wacv23_tsnet_amd.engine import TSNetEngine
B, H, W = 4, 256, 256
NB = int(sys.argv[sys.argv.index("--n-blocks") + 1]) if "--n-blocks" in sys.argv else 0
if "--batch" in sys.argv:
    B = int(sys.argv[sys.argv.index("--batch") + 1])
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
