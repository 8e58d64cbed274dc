#!/usr/bin/env python3
"""Time of the agglomerative segmentation (jsgx_agglomerative_launch, libjsgx.so) at 1 x 16384 x 20 with k = 10 (MFCC frames of a track),
64 x 1024 x 128 with k = 12 (beat-synchronous mel) and 64 x 16384 x 128 with a boundary every 43 frames and 4 clusters a stretch
(subsegment): the whole launch with HIP events after warm-up calls, and the same launch with k = the frames (no merge step: the fixed
part), so that the difference over the steps of a stretch is the time of a merge step.  Against the host route (the plane copied to the
host, scikit-learn's AgglomerativeClustering in float64 on a chain, the copy included; for the subsegment shape one plane of the 64 is
run and the time scaled) and against the same greedy merge as a loop of torch operations on the GPU, every stretch of the launch in
one batch (run once).  The fixed part is also timed on the same bytes cut into planes of 64 frames, where "agglo_group" is not
launched, and a device-to-device copy of the plane beside it.  Also one stretch alone of 64, 1024 and 16384 frames: the latency of a step of either merge kernel.

    python tools/agglo_bench.py --run OUT.json [--reps R] [--no-host] [--no-torch]
    python tools/agglo_bench.py --report profiles/agglo_bench.md OUT.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, pairs, frames, features, k, a boundary every so many frames (0: none)
WORKLOADS = [("agglomerative, MFCC frames of a track", 1, 16384, 20, 10, 0), ("agglomerative, beat-synchronous mel", 64, 1024, 128, 12, 0),
             ("subsegment, a beat every 43 frames", 64, 16384, 128, 4, 43)]
ALONE = [(64, 20), (64, 128), (1024, 128), (16384, 20), (16384, 128)]          # one stretch, k = 1: frames, features


def timed(fn, reps, torch, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    times.sort()
    return times[0], times[len(times) // 2]


def torch_loop(torch, x, edges, k):
    """The greedy merge as torch operations: x [P][N][F], the stretches between `edges` (a list with 0 and N), all of them in one batch
    [B][L][F] padded to the longest.  Every step computes every cluster's mean and every cost again.  Returns the boundary mask [B][L]."""
    P, N, F = x.shape
    lens = torch.tensor([b - a for a, b in zip(edges[:-1], edges[1:])], device=x.device)
    L = int(lens.max())
    at = torch.tensor(edges[:-1], device=x.device)[:, None] + torch.arange(L, device=x.device)[None, :]
    inside = torch.arange(L, device=x.device)[None, :] < lens[:, None]
    X = x[:, torch.where(inside, at, torch.zeros_like(at))].reshape(-1, L, F) * inside.repeat(P, 1)[:, :, None]
    inside = inside.repeat(P, 1)
    B = X.shape[0]
    start = inside.clone()
    rows = torch.arange(B, device=x.device)
    inf = torch.full((), float("inf"), device=x.device)
    for _ in range(L - k):
        cid = torch.cumsum(start, 1) - 1          # the cluster of every frame (a padded frame: the last one's, to which it adds zeros)
        sums = torch.zeros((B, L, F), device=x.device).scatter_add_(1, cid[:, :, None].expand(-1, -1, F), X)
        cnt = torch.zeros((B, L), device=x.device).scatter_add_(1, cid, inside.float())
        n = start.sum(1)
        mean = sums / cnt.clamp(min=1)[:, :, None]
        d = ((mean[:, :-1] - mean[:, 1:]) ** 2).sum(2)
        cost = cnt[:, :-1] * cnt[:, 1:] / (cnt[:, :-1] + cnt[:, 1:]).clamp(min=1) * d
        live = (torch.arange(L - 1, device=x.device)[None, :] < (n - 1)[:, None]) & (n > k)[:, None]
        best = torch.where(live, cost, inf).argmin(1)          # the pair (best, best + 1) of clusters
        go = live.any(1)
        # the frame where cluster best + 1 starts: the first frame whose cluster id is best + 1
        first = ((cid == (best + 1)[:, None]) & start).float().argmax(1)
        start[rows[go], first[go]] = False
    return start


def run(out_path, reps, host=True, loop=True):
    import numpy as np
    import torch
    import jadespectrogram_amd as jsg
    assert torch.cuda.is_available(), "agglo_bench measures on the GPU"
    results, alone = [], []

    def launcher(x, d_b, k, S):
        P, N, _ = x.shape
        seg, ns, no = torch.empty((P, S + 1), dtype=torch.int32, device="cuda"), torch.empty((P,), dtype=torch.int32, device="cuda"), torch.empty((P,), dtype=torch.int32, device="cuda")
        out = torch.empty((P, min(N, S * k)), dtype=torch.int32, device="cuda")
        scratch = torch.empty((jsg.agglomerative_scratch_bytes(x, d_b, None, seg, ns, out, no, n_clusters=k),), dtype=torch.uint8, device="cuda")
        return (lambda: jsg.agglomerative_launch(x, d_b, None, seg, ns, out, no, n_clusters=k, d_scratch=scratch)), out, no

    for N, F in ALONE:
        x = torch.randn((1, N, F), dtype=torch.float32, device="cuda")
        full, _, _ = launcher(x, None, 1, 1)
        fixed, _, _ = launcher(x, None, N, 1)
        t, t0 = timed(full, reps, torch), timed(fixed, reps, torch)
        alone.append(dict(frames=N, features=F, kernel=jsg.agglomerative_plan(N, F)[0], launch_s=t, no_step_s=t0, steps=N - 1, us_per_step=(t[1] - t0[1]) / (N - 1) * 1e6))
        print(json.dumps(alone[-1]), flush=True)
    for name, P, N, F, k, every in WORKLOADS:
        x = torch.randn((P, N, F), dtype=torch.float32, device="cuda")
        b = np.arange(every, N, every, dtype=np.int32) if every else np.zeros(0, np.int32)
        edges = [0] + b.tolist() + [N]
        S = len(edges) - 1
        d_b = torch.from_numpy(b).cuda() if every else None
        full, out, no = launcher(x, d_b, k, S)
        fixed, _, _ = launcher(x, d_b, N, S)
        t, t0 = timed(full, reps, torch), timed(fixed, reps, torch)
        want = sum(min(k, c - a) for a, c in zip(edges[:-1], edges[1:]))
        assert no.cpu().tolist() == [want] * P
        steps = max(c - a - min(k, c - a) for a, c in zip(edges[:-1], edges[1:]))          # of the longest stretch: the dependent chain
        row = dict(name=name, pairs=P, frames=N, features=F, k=k, every=every, stretches=S, kernel="agglo_wave" if max(np.diff(edges)) <= 64 else "agglo_group",
                   launch_s=t, no_step_s=t0, steps_of_a_stretch=steps, us_per_step=(t[1] - t0[1]) / steps * 1e6)
        # the fixed part once more on the same bytes as planes of 64 frames, one stretch each, where "agglo_group" is not launched: what
        # its workgroups that find a short stretch and leave cost the launch above
        short, _, _ = launcher(x.view(P * N // 64, 64, F), None, 64, 1)
        other = torch.empty_like(x)
        row["no_step_without_group_s"], row["copy_s"] = timed(short, reps, torch), timed(lambda: other.copy_(x), reps, torch)
        del other, short
        ours = out.cpu().numpy()
        if host:
            from sklearn.cluster import AgglomerativeClustering
            from sklearn.feature_extraction.image import grid_to_graph
            planes = 1 if every else P          # the subsegment shape: one plane of the 64, scaled
            a = time.perf_counter()
            xh = x[:planes].cpu().numpy().astype(np.float64)
            copy = time.perf_counter() - a
            same = total = 0
            for p in range(planes):
                got = []
                for u0, u1 in zip(edges[:-1], edges[1:]):
                    if u1 - u0 == 1:          # the class wants two samples
                        got.append(u0)
                        continue
                    labels = AgglomerativeClustering(n_clusters=min(k, u1 - u0), linkage="ward", connectivity=grid_to_graph(u1 - u0, 1, 1)).fit(xh[p, u0:u1]).labels_
                    got += [u0] + (u0 + 1 + np.flatnonzero(np.diff(labels) != 0)).tolist()
                same += int((np.array(got) == ours[p, :len(got)]).sum())          # out holds k entries a stretch; a short stretch fills fewer
                total += len(got)
            spent = time.perf_counter() - a
            row["host"] = dict(planes_run=planes, copy_s=copy * P / planes, total_s=spent * P / planes, boundaries_equal=same, boundaries=total)
        if loop:
            torch.cuda.synchronize()
            a = time.perf_counter()
            start = torch_loop(torch, x, edges, k)
            torch.cuda.synchronize()
            row["torch_loop_s"] = time.perf_counter() - a
            got = start.reshape(P, S, -1)
            mine = torch.zeros_like(got)
            off = torch.tensor(edges[:-1], device="cuda")
            idx = out.long().reshape(P, S, -1) - off[None, :, None] if not any(c - a < k for a, c in zip(edges[:-1], edges[1:])) else None
            if idx is not None:
                mine.scatter_(2, idx, torch.ones_like(idx, dtype=torch.bool))
                row["torch_loop_masks_equal"] = float((mine == got).all(2).float().mean())
            del start, got, mine
        results.append(row)
        print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), reps=reps, alone=alone, results=results), f, indent=1)


def report(md_path, json_path):
    data = json.load(open(json_path))
    ms = lambda v: f"{v[1] * 1e3:.3f}"
    lines = ["# Agglomerative segmentation: measured times", "",
             f"`python tools/agglo_bench.py --run` on one MI355X (\"{data['device']}\" to torch): median of {data['reps']} launches (HIP events, after 2 warm-up calls).",
             "A launch is all its kernels: the segments, the copy of the plane into the scratch with the first costs, the offsets, and the merge",
             "kernels.  `no step`: the same launch with k = the frames, which merges nothing: the fixed part.  A merge step is the difference over",
             "the steps of the longest stretch, the dependent chain of the launch.  `host`: the plane copied to the host and scikit-learn's",
             "`AgglomerativeClustering(linkage=\"ward\", connectivity=grid_to_graph(n, 1, 1))` in float64 on every stretch, the copy included (the",
             "subsegment shape runs one plane of the 64 and the time is scaled by 64).  `torch loop`: the same greedy merge as a loop of torch",
             "operations on the same GPU, every stretch of the launch in one batch, every cost computed again in every step, run once.  No ratio",
             "was fixed in advance; the times are as measured.  `no step, no group`: the fixed part on the same bytes as planes of 64 frames of one",
             "stretch each, a launch without \"agglo_group\": the difference to `no step` is what that kernel's workgroups cost where they find a short",
             "stretch and leave (one a possible stretch, each declaring the LDS of the longest stretch the plane allows).  `copy`: a device-to-device",
             "copy of the plane, for scale: the fixed part reads the plane twice and writes it once.  Where a launch holds more stretches than",
             "the device runs wavefronts at a time (the subsegment shape: 24448), the microseconds a step are the launch's time over the steps",
             "of one stretch, several rounds of wavefronts deep, not the latency of a step; that latency is in the first table.", "",
             "## One stretch alone, k = 1", "", "| frames x features | kernel | launch (ms) | no step (ms) | steps | microseconds a step |", "|---|---|---|---|---|---|"]
    for r in data["alone"]:
        lines.append(f"| {r['frames']} x {r['features']} | {r['kernel']} | {ms(r['launch_s'])} | {ms(r['no_step_s'])} | {r['steps']} | {r['us_per_step']:.2f} |")
    lines += ["", "## The three shapes", "",
              "| shape | kernel | launch (ms) | no step (ms) | no step, no group (ms) | copy (ms) | steps of a stretch | microseconds a step | host (ms), of which copy | torch loop (ms) |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for r in data["results"]:
        h = r.get("host")
        host = f"{h['total_s'] * 1e3:.0f}, {h['copy_s'] * 1e3:.1f}" + (f" (from {h['planes_run']} plane of {r['pairs']})" if h['planes_run'] != r['pairs'] else "") if h else "not run"
        loop = f"{r['torch_loop_s'] * 1e3:.0f}" if "torch_loop_s" in r else "not run"
        lines.append(f"| {r['name']}: {r['pairs']} x {r['frames']} x {r['features']}, k = {r['k']}" + (f", every {r['every']}" if r["every"] else "") +
                     f" | {r['kernel']} | {ms(r['launch_s'])} | {ms(r['no_step_s'])} | {ms(r['no_step_without_group_s'])} | {ms(r['copy_s'])} | {r['steps_of_a_stretch']} | {r['us_per_step']:.2f} | {host} | {loop} |")
    lines += ["", "Agreement, for the record (float32 on the GPU against float64 on the host, on noise, where two costs can lie inside the rounding):", ""]
    for r in data["results"]:
        h = r.get("host")
        if h:
            lines.append(f"- {r['name']}: {h['boundaries_equal']} of {h['boundaries']} boundaries equal scikit-learn's" +
                         (f"; {100 * r['torch_loop_masks_equal']:.1f} % of the stretches equal the torch loop's" if "torch_loop_masks_equal" in r else ""))
    lines.append("")
    with open(md_path, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--report", nargs=2)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if a.run:
        run(a.run, a.reps, not a.no_host, not a.no_torch)
    if a.report:
        report(*a.report)
