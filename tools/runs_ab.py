#!/usr/bin/env python3
"""DEV TOOL: several builds of the library in ONE process on the two headline geometries of the 1024-point "runs" kernel, interleaved:
  c2  64 batches x 4096 frames, mono, hop 512, tail-plane layout -- one strided dispatch covers the whole rotation
  c4  8 batches x 8 channels x 4096 frames, one column per channel (the C4 shard), same layout
    python tools/runs_ab.py [--cfg c2,c4] [--reps 48] [--rounds 9] libA.so libB.so ...
Every library gets its own copy of the Python package (its own handle and plan).  A round times `reps` back-to-back dispatches of every
library in turn (HIP events on one stream, two untimed dispatches first); round 0 lets the clocks settle and is dropped.  Printed per library:
every round's us per dispatch, median, spread (max - min), bit identity of its output against the first library's; and per pair with the first:
the median gain, and whether EVERY round of the one is faster than EVERY round of the other."""
import argparse, importlib.util, json, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import torch


def load(path, k):
    pkg = os.path.join(ROOT, "jadespectrogram_amd")
    spec = importlib.util.spec_from_file_location(f"jsg_ab{k}", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.capi.LIB_PATH = os.path.abspath(path)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="c2,c4")
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("libs", nargs="+")
    args = ap.parse_args()
    mods = [load(p, k) for k, p in enumerate(args.libs)]
    n, hop, F = 1024, 512, 4096
    st = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for cfg in args.cfg.split(","):
        K, C = (64, 1) if cfg == "c2" else (8, 8)
        g = torch.Generator(device="cuda"); g.manual_seed(1)
        d_in = torch.rand((K, C, F * hop + n - hop), device="cuda", generator=g) - 0.5
        per = C > 1
        shape = (K, C, F, 512) if per else (K, F, 512)
        outs = [torch.full(shape, -7.0, device="cuda") for _ in mods]
        tails = [torch.full((K, C, F), -7.0, device="cuda") for _ in mods]
        runs = []
        for m, o, t in zip(mods, outs, tails):
            plan = m.Plan(n, m.window(m.capi.WIN_HANN, n))
            kw = dict(feedblocks=2, mix_mode=m.capi.MIX_PER_CHANNEL if per else m.capi.MIX_ABSMEAN, d_tail=t, stream=st.cuda_stream)
            runs.append((lambda m, plan, o, kw: lambda: m.stft_db_strided(plan, d_in, hop, F, o, **kw))(m, plan, o, kw))
        times = [[] for _ in mods]
        for r in range(args.rounds + 1):
            for k, fn in enumerate(runs):
                with torch.cuda.stream(st):
                    fn(); fn()
                    e0.record(st)
                    for _ in range(args.reps):
                        fn()
                    e1.record(st)
                torch.cuda.synchronize()
                if r:
                    times[k].append(e0.elapsed_time(e1) * 1e3 / args.reps)
        algo = (4 * hop + 4 * 513) * F * K * C
        for k, p in enumerate(args.libs):
            t = sorted(times[k]); med = t[len(t) // 2]
            same = bool(torch.equal(outs[k], outs[0]) and torch.equal(tails[k], tails[0]))
            line = {"cfg": cfg, "lib": os.path.basename(p), "us_per_dispatch_median": round(med, 3), "spread_us": round(t[-1] - t[0], 3),
                    "frac_of_8TBs_median": round(algo / med / 8e6, 4), "identical_to_first": same, "rounds": [round(x, 3) for x in times[k]]}
            if k:
                t0 = sorted(times[0]); med0 = t0[len(t0) // 2]
                line["gain_vs_first_pct"] = round((med0 / med - 1) * 100, 3)
                line["every_round_faster_than_every_round_of_first"] = t[-1] < t0[0]
                line["gain_over_twice_the_spread"] = (med0 - med) > 2 * max(t[-1] - t[0], t0[-1] - t0[0])
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
