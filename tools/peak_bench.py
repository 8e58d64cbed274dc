#!/usr/bin/env python3
"""Time of peak picking (jsgx_peak_launch, libjsgx.so) at 64 x 16384, 4096 x 1024 and 1 x 2^24 (rows x frames) of smooth noise, the
default reaches of onset_detect at 22050 / 512 (1, 0, 4, 4), delta 0.07, normalised, wait 1 and 30, backtracking on the envelope itself:
the whole launch with HIP events after warm-up calls, each of its kernels on its own (torch's profiler, a run of its own), and the route a
user has without it: the two window tests with torch.nn.functional.max_pool1d / avg_pool1d on the GPU, the flags copied to the host, the
wait rule as a loop over the candidates in Python.  And the same launches with builds of the library at other JSGX_PEAK_BLOCK.

    python tools/peak_bench.py --build-variants            (no GPU) builds tools/variants/libjsgx_peak{256,512,1024,2048}.so
    python tools/peak_bench.py --run OUT.json [--lib LIB] [--no-route] [--reps R]
    python tools/peak_bench.py --report profiles/peak_bench.md MAIN.json [BLOCK.json ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [(64, 16384), (4096, 1024), (1, 1 << 24)]          # rows, frames
WAITS = (1, 30)
REACHES = dict(pre_max=1, post_max=0, pre_avg=4, post_avg=4)
DELTA = 0.07
BLOCKS = (256, 512, 1024, 2048)
KERNELS = ("peak_single", "peak_stats", "peak_row", "peak_cand", "peak_carry", "peak_emit")


def build_variants():
    from jadespectrogram_amd import _build
    hipcc = _build._hipcc()
    vdir = os.path.join(ROOT, "tools", "variants")
    os.makedirs(vdir, exist_ok=True)
    _build.build_lib()
    for block in BLOCKS:
        objs = []
        for src in _build.SOURCES_X:
            o = os.path.join(_build.PKG, "build", os.path.splitext(src)[0] + ".o")
            if "peak" in src:
                o = os.path.join(vdir, f"{os.path.splitext(src)[0]}_block{block}.o")
                cmd = [hipcc, "-std=c++17", "-O3", "-fPIC", "-c", os.path.join(_build.CSRC, src), "-o", o, "-I", os.path.join(ROOT, "include"),
                       f"-DJSGX_PEAK_BLOCK={block}"] + _build.VISIBILITY
                cmd += [f"--offload-arch={_build.ARCH}"] + _build.HIP_FLAGS if src.endswith(".hip") else ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__"]
                subprocess.check_call(cmd)
            objs.append(o)
        out = os.path.join(vdir, f"libjsgx_peak{block}.so")
        subprocess.check_call([hipcc, "-shared", "-fPIC", f"--offload-arch={_build.ARCH}", "-o", out] + objs)
        print(out)


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


def kernel_times(torch, fn, reps):
    """Median device time in seconds of each of the launch's kernels over `reps` calls, from torch's profiler; None where it reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        found = {}
        for e in prof.events():
            for k in KERNELS:
                if k + "_kernel" in e.name:
                    t = getattr(e, "device_time", None) or getattr(e, "cuda_time", 0)
                    if t:
                        found.setdefault(k, []).append(t * 1e-6)
        return {k: sorted(v)[len(v) // 2] for k, v in found.items()} or None
    except Exception as err:          # the profiler is an extra: the report says so
        print("profiler:", err, flush=True)
        return None


def torch_route(torch, np, x, wait):
    """The window tests on the GPU with torch's pooling, the flags to the host, the wait rule in Python: (seconds on the GPU with the copy,
    seconds of the host loop, the peaks of every row)."""
    F = torch.nn.functional
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mn, mx = x.amin(1, keepdim=True), x.amax(1, keepdim=True)
    y = (x - mn) / (mx - mn)
    top = F.max_pool1d(F.pad(y, (REACHES["pre_max"], REACHES["post_max"]), value=float("-inf"))[:, None], REACHES["pre_max"] + REACHES["post_max"] + 1, 1)[:, 0]
    k = REACHES["pre_avg"] + REACHES["post_avg"] + 1
    total = F.avg_pool1d(F.pad(y, (REACHES["pre_avg"], REACHES["post_avg"]))[:, None], k, 1)[:, 0] * k
    count = F.avg_pool1d(F.pad(torch.ones_like(y[:1]), (REACHES["pre_avg"], REACHES["post_avg"]))[:, None], k, 1)[:, 0] * k
    flags = ((y >= top) & (y >= total / count + DELTA)).cpu().numpy()
    t1 = time.perf_counter()
    peaks = []
    for row in flags:
        out, e = [], 0
        for t in np.flatnonzero(row).tolist():
            if t >= e:
                out.append(t)
                e = t + wait + 1
        peaks.append(out)
    return t1 - t0, time.perf_counter() - t1, peaks


def run(args):
    import numpy as np
    import torch
    from jadespectrogram_amd import capix
    if args.lib:
        capix.LIB_PATH = os.path.abspath(args.lib)
    import jadespectrogram_amd as jsg
    assert torch.cuda.is_available(), "peak_bench measures on the GPU; there is nothing to report without one"
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    record = {"lib": args.lib or "product", "device": props.name, "cus": props.multi_processor_count, "reps": args.reps, "rows": []}
    for R, T in WORKLOADS:
        gen = torch.Generator(device="cuda").manual_seed(T)
        w = torch.randn((R, 1, T + 8), generator=gen, dtype=torch.float32, device="cuda")
        x = torch.nn.functional.conv1d(w, torch.hann_window(11, periodic=False, device="cuda")[None, None, 1:-1])[:, 0].contiguous()
        del w
        for wait in WAITS:
            most = 1 + (T - 1) // (wait + 1)
            peaks, back = torch.empty((2, R, most), dtype=torch.int32, device="cuda")
            n_peaks = torch.empty((R,), dtype=torch.int32, device="cuda")
            kw = dict(REACHES, delta=DELTA, wait=wait, normalise=True, d_energy=x, d_backtracked=back)
            scratch = torch.empty(max(4, jsg.peak_scratch_bytes(x, peaks, n_peaks, **kw)), dtype=torch.uint8, device="cuda")
            ours = lambda: jsg.peak_launch(x, peaks, n_peaks, d_scratch=scratch, **kw)
            best, med = timed(ours, args.reps, torch)
            parts = kernel_times(torch, ours, args.reps)
            row = {"rows": R, "frames": T, "wait": wait, "form": jsg.peak_plan(T, R, wait)[0], "best": best, "median": med, "kernels": parts,
                   "peaks": int(n_peaks.sum())}
            if not args.no_route:
                gpu_s, host_s, theirs = torch_route(torch, np, x, wait)
                gpu_s, host_s, theirs = torch_route(torch, np, x, wait)          # the second call: pools and copies warm
                n = n_peaks.cpu().numpy()
                mine = peaks.cpu().numpy()
                same = sum(mine[r, :n[r]].tolist() == theirs[r] for r in range(R))
                row.update(route_gpu=gpu_s, route_host=host_s, rows_equal=same)
            record["rows"].append(row)
            print(row, flush=True)
            del peaks, back, scratch
        del x
        torch.cuda.empty_cache()
    with open(args.run, "w") as f:
        json.dump(record, f, indent=1)


def report(args):
    main = json.load(open(args.files[0]))
    others = [json.load(open(f)) for f in args.files[1:]]
    ms = lambda s: f"{s * 1e3:.3f}"
    with open(args.report, "w") as f:
        f.write("# Peak picking: time of a launch\n\n")
        f.write(f"`python tools/peak_bench.py` on {main['device']} ({main['cus']} compute units).  Smooth noise (white noise under a 9-tap Hann window), the reaches "
                f"(1, 0, 4, 4), delta {DELTA}, normalised, backtracked on the envelope itself.  ms: best (median) of {main['reps']} timed calls after 2 warm-up calls, HIP "
                "events.  The kernels' own times are medians of torch's profiler over the same number of calls, a run of its own.  The route without this library: the "
                "window tests with `max_pool1d` / `avg_pool1d` on the GPU and the flags copied to the host (pool + copy, wall clock, second call), then the wait rule as a "
                "Python loop over `np.flatnonzero` of every row (host loop).  rows equal: the rows whose peaks equal that route's (its mean is another sum, so a "
                "threshold tie can fall the other way).\n\n")
        f.write("| rows x frames | wait | form | peaks | ms | kernels ms | pool + copy ms | host loop ms | route / this | rows equal |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in main["rows"]:
            k = "not reported" if not r["kernels"] else ", ".join(f"{n[5:]} {ms(t)}" for n, t in r["kernels"].items())
            route = (r["route_gpu"] + r["route_host"]) if "route_gpu" in r else None
            f.write(f"| {r['rows']} x {r['frames']} | {r['wait']} | {r['form']} | {r['peaks']} | {ms(r['best'])} ({ms(r['median'])}) | {k} | "
                    + ("- | - | - | - |\n" if route is None else f"{ms(r['route_gpu'])} | {ms(r['route_host'])} | {route / r['best']:.0f} | {r['rows_equal']} of {r['rows']} |\n"))
        if others:
            f.write("\n## JSGX_PEAK_BLOCK\n\nBuilds of the library with other block lengths (`--build-variants`), each in a process of its own: ms of the launch, and of its kernels.\n\n")
            f.write("| library | rows x frames | wait | form | ms | kernels ms |\n|---|---|---|---|---|---|\n")
            for rec in others:
                for r in rec["rows"]:
                    k = "not reported" if not r["kernels"] else ", ".join(f"{n[5:]} {ms(t)}" for n, t in r["kernels"].items())
                    f.write(f"| {os.path.basename(rec['lib'])} | {r['rows']} x {r['frames']} | {r['wait']} | {r['form']} | {ms(r['best'])} ({ms(r['median'])}) | {k} |\n")
    print("wrote", args.report)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--run", metavar="OUT.json")
    ap.add_argument("--lib")
    ap.add_argument("--no-route", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--report", metavar="FILE.md")
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    if args.run:
        return run(args)
    if args.report:
        return report(args)
    ap.error("one of --build-variants, --run, --report")


if __name__ == "__main__":
    main()
