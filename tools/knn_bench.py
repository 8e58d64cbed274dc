#!/usr/bin/env python3
"""Time of the k nearest frames (jsgx_knn_launch, libjsgx.so) on a self-comparison of N = 4096 and 16384 frames of 20 features with
librosa's default k and width 1, euclidean and cosine, next to the two routes through the dense plane on the same GPU:
jsgx_cdist_launch followed by torch.topk(largest=False), and jsgx_cdist_launch alone.  HIP events around `inner` launches, warm-up first,
the three routes interleaved in every round (A, B, C, A, B, C, ...), medians and the best over the rounds.  Then the search at every
split, and the recurrence plane and nn_filter from its lists.  The fused lists are compared with the dense route (distances bit for bit;
indices wherever a row has no tie).  Writes profiles/knn_bench.md.

    python tools/knn_bench.py [--rounds R] [--inner I] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 20
SIZES = (4096, 16384)
METRICS = ("euclidean", "cosine")


def span(torch, fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleaved(torch, fns, rounds, inner):
    """{name: (median ms, best ms)} of the routes timed turn by turn."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(span(torch, fn, inner))
    return {name: (sorted(t)[len(t) // 2], min(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.md"))
    opt = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    assert torch.cuda.is_available(), "this benchmark needs the MI355X; there is no CPU route"
    torch.cuda.set_device(0)
    prop = torch.cuda.get_device_properties(0)
    n_cu = prop.multi_processor_count
    fmt = lambda t: f"{t[0]:.3f} ({t[1]:.3f})"
    rows, split_rows, rest_rows = [], [], []
    for N in SIZES:
        k = jsg.knn_default_k(N, 1)
        gen = torch.Generator(device="cuda").manual_seed(N)
        x = torch.randn((N, K), generator=gen, dtype=torch.float32, device="cuda")
        index = torch.empty((N, k), dtype=torch.int32, device="cuda")
        dist = torch.empty((N, k), dtype=torch.float32, device="cuda")
        cost = torch.empty((N, N), dtype=torch.float32, device="cuda")
        scratch = torch.empty((max(1, jsg.knn_scratch_bytes(x, x, index, dist, split=16) // 4),), dtype=torch.int32, device="cuda")
        for metric in METRICS:
            name, strip, S, threads, lds = jsg.knn_plan(N, N, K, k, metric=metric, n_cu=n_cu)
            per_cu = min(jsg.capix.KNN_LDS_LIMIT // lds, 2048 // threads)

            def fused():
                jsg.knn_launch(x, x, index, dist, width=1, metric=metric, d_scratch=scratch)

            def dense_topk():
                jsg.cdist_launch(x, x, cost, metric=metric)
                cost.diagonal().fill_(float("inf"))                 # width 1
                return torch.topk(cost, k, dim=1, largest=False)

            def dense():
                jsg.cdist_launch(x, x, cost, metric=metric)

            t = interleaved(torch, {"fused": fused, "topk": dense_topk, "dense": dense}, opt.rounds, opt.inner)
            fused()
            values, where = dense_topk()
            torch.cuda.synchronize()
            same_dist = bool((values.view(torch.int32) == dist.view(torch.int32)).all())
            untied = (values[:, 1:] != values[:, :-1]).all(dim=1)
            same_index = bool((where[untied].int() == index[untied]).all())
            rows.append(f"| {N} | {metric} | {k} | {S} | {lds} | {per_cu} ({per_cu * threads // 64} wavefronts) | {fmt(t['fused'])} | {fmt(t['topk'])} | {fmt(t['dense'])} | "
                        f"{t['topk'][0] / t['fused'][0]:.2f} | {t['fused'][0] / t['dense'][0]:.2f} | {'yes' if same_dist else 'NO'} / {'yes' if same_index else 'NO'} ({int(untied.sum())} rows without a tie) |")
            if metric == "euclidean":
                by_split = {}
                for split in (1, 2, 4, 8, 16):
                    by_split[f"S={split}"] = (lambda s: (lambda: jsg.knn_launch(x, x, index, dist, width=1, metric=metric, split=s, d_scratch=scratch)))(split)
                ts = interleaved(torch, by_split, opt.rounds, opt.inner)
                split_rows.append(f"| {N} | {k} | " + " | ".join(fmt(ts[f"S={s}"]) for s in (1, 2, 4, 8, 16)) + " |")
                rec = torch.empty((N, N), dtype=torch.float32, device="cuda")
                bw = torch.full((1,), 1.0, dtype=torch.float32, device="cuda")
                filt = torch.empty_like(x)
                fused()
                tr = interleaved(torch, {"conn": lambda: jsg.recurrence_launch(index, dist, rec), "mutual": lambda: jsg.recurrence_launch(index, dist, rec, mode="affinity", sym=True, d_bandwidth=bw),
                                         "fill": lambda: rec.fill_(0.0), "nnf": lambda: jsg.nn_filter_launch(x, index, filt)}, opt.rounds, opt.inner)
                rest_rows.append(f"| {N} | {k} | {fmt(tr['conn'])} | {fmt(tr['mutual'])} | {fmt(tr['fill'])} | {fmt(tr['nnf'])} |")
    lines = ["# k nearest frames, recurrence plane and nn_filter timing (tools/knn_bench.py)", "",
             f"Device: {prop.name}, {n_cu} compute units; HIP events around {opt.inner} launches, two warm-up calls per route, the routes interleaved in each of "
             f"{opt.rounds} rounds; ms per call, median (best) over the rounds.", "",
             f"A self-comparison (x == y) of N frames of {K} features, width 1, librosa's default k.  fused: `jsgx_knn_launch` (`knn_64`, split automatic).  dense + topk: "
             "`jsgx_cdist_launch` into an N x N plane, the diagonal set to +inf, `torch.topk(largest=False)`.  dense: `jsgx_cdist_launch` alone.  "
             "occupancy: workgroups per compute unit that the LDS of a workgroup allows (160 KiB per compute unit).", "",
             "| N | metric | k | S | LDS bytes per workgroup | workgroups per CU | fused ms | dense + topk ms | dense ms | dense + topk / fused | fused / dense | same distances / indices |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"] + rows + ["",
             "## Every split (euclidean)", "", "| N | k | S = 1 | S = 2 | S = 4 | S = 8 | S = 16 |", "|---|---|---|---|---|---|---|"] + split_rows + ["",
             "## The plane and the filter from the lists (euclidean lists)", "",
             "`recurrence_rows` writes N x N floats; `fill` is torch's fill of the same plane, the cost of writing it at all.", "",
             "| N | k | connectivity ms | affinity, mutual ms | fill ms | nn_filter (20 features) ms |", "|---|---|---|---|---|---|"] + rest_rows + [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(opt.out), exist_ok=True)
    with open(opt.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
