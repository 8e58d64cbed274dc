#!/usr/bin/env python3
"""Time of the segment aggregation (jsgx_sync_launch, libjsgx.so) and of the time-delay embedding (jsgx_stack_memory_launch) at
64 x 16384 x 128 and 16 x 16384 x 1025 (pairs x frames x features) with a boundary every 43 frames and at 16 x 2^20 x 20 with 8 segments:
each of the four aggregates and the stacking at 5 steps, the whole launch with HIP events after warm-up calls, against what a user has in
torch on the same GPU: torch.segment_reduce for mean, min and max, a padded gather + torch.nanmedian for the median, torch.roll + cat for
the stacking.  For the mean and the stacking also the share of the copy roof measured in the same run (a device-to-device copy of a plane).

And the median alone with builds of the library that leave a form out: "noalone" (JSGX_SYNC_WAVE_MAX = 0: never a wavefront a segment,
always the four together) and "nostage" (also JSGX_SYNC_STAGE = 0: no segment staged in LDS, every pass reads through the caches).

    python tools/sync_bench.py --build-variants            (no GPU) builds tools/variants/libjsgx_sync_{noalone,nostage}.so
    python tools/sync_bench.py --run OUT.json [--reps R] [--lib LIB --median-only]
    python tools/sync_bench.py --report profiles/sync_bench.md OUT.json [VARIANT.json ...]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# pairs, frames, features, boundaries (without 0 and the end)
WORKLOADS = [(64, 16384, 128, "every 43"), (16, 16384, 1025, "every 43"), (16, 1 << 20, 20, "8 segments")]
AGGS = ("mean", "min", "max", "median")
STEPS, DELAY = 5, 1


VARIANTS = {"noalone": ["-DJSGX_SYNC_WAVE_MAX=0"], "nostage": ["-DJSGX_SYNC_WAVE_MAX=0", "-DJSGX_SYNC_STAGE=0"]}


def build_variants():
    from jadespectrogram_amd import _build
    hipcc = _build._hipcc()
    vdir = os.path.join(ROOT, "tools", "variants")
    os.makedirs(vdir, exist_ok=True)
    _build.build_lib()
    for name, defines in VARIANTS.items():
        objs = []
        for src in _build.SOURCES_X:
            o = os.path.join(_build.PKG, "build", os.path.splitext(src)[0] + ".o")
            if src == "jsgx_sync.hip":
                o = os.path.join(vdir, f"jsgx_sync_{name}.o")
                subprocess.check_call([hipcc, "-std=c++17", "-O3", "-fPIC", "-c", os.path.join(_build.CSRC, src), "-o", o, "-I", os.path.join(ROOT, "include"),
                                       f"--offload-arch={_build.ARCH}"] + defines + _build.VISIBILITY + _build.HIP_FLAGS)
            objs.append(o)
        out = os.path.join(vdir, f"libjsgx_sync_{name}.so")
        subprocess.check_call([hipcc, "-shared", "-fPIC", f"--offload-arch={_build.ARCH}", "-o", out] + objs)
        print(out)


def boundaries(np, N, how):
    return np.arange(43, N, 43, dtype=np.int32) if how == "every 43" else np.arange(N // 8, N, N // 8, dtype=np.int32)[:7]


def timed(fn, reps, torch, warm=3):
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


def run(out_path, reps, lib=None, median_only=False):
    import numpy as np
    import torch
    import jadespectrogram_amd as jsg
    if lib:
        jsg.capix.LIB_PATH = os.path.abspath(lib)
    assert torch.cuda.is_available(), "sync_bench measures on the GPU"
    results = []
    for P, N, F, how in WORKLOADS:
        x = torch.randn((P, N, F), dtype=torch.float32, device="cuda")
        b = boundaries(np, N, how)
        edges = np.concatenate(([0], b, [N]))
        S = len(edges) - 1
        lengths = torch.from_numpy(np.diff(edges).astype(np.int64)).cuda()
        d_b = torch.from_numpy(b).cuda()
        seg = torch.empty((P, S + 1), dtype=torch.int32, device="cuda")
        ns = torch.empty((P,), dtype=torch.int32, device="cuda")
        out = torch.empty((P, S, F), dtype=torch.float32, device="cuda")
        plane_bytes = 4 * P * N * F
        other = torch.empty_like(x)
        copy = timed(lambda: other.copy_(x), reps, torch)
        roof = 2 * plane_bytes / copy[1]          # bytes moved a second by a copy: read and written
        del other
        row = dict(pairs=P, frames=N, features=F, boundaries=how, segments=S, copy_s=copy, roof_bytes_per_s=roof, ours={}, torch={})
        for agg in ("median",) if median_only else AGGS:
            row["ours"][agg] = timed(lambda: jsg.sync_launch(x, d_b, None, seg, ns, out, aggregate=agg), reps, torch)
            assert ns.cpu().tolist() == [S] * P
        if median_only:
            results.append(row)
            print(json.dumps(row), flush=True)
            del x, out
            torch.cuda.empty_cache()
            continue
        row["mean_share_of_roof"] = (plane_bytes + 4 * P * S * F) / row["ours"]["mean"][1] / roof
        xt = x.transpose(0, 1).contiguous()          # segment_reduce along axis 0 of [frames][pairs][features]; the transpose is not timed
        for agg in ("mean", "min", "max"):
            try:
                row["torch"][agg] = timed(lambda: torch.segment_reduce(xt, agg, lengths=lengths, axis=0), max(3, reps // 4), torch)
            except Exception as err:
                row["torch"][agg] = str(err)[:120]
        del xt
        try:
            longest = int(lengths.max())
            at = torch.from_numpy(edges[:-1].astype(np.int64)).cuda()[:, None] + torch.arange(longest, device="cuda")[None, :]
            valid = torch.arange(longest, device="cuda")[None, :] < lengths[:, None]
            at = torch.where(valid, at, torch.zeros_like(at))

            def median():
                g = x[:, at]          # [pairs][segments][longest][features]
                g = torch.where(valid[None, :, :, None], g, torch.full((), float("nan"), device="cuda"))
                return torch.nanmedian(g, dim=2).values
            row["torch"]["median"] = timed(median, max(3, reps // 4), torch)
        except Exception as err:
            row["torch"]["median"] = str(err)[:120]
        del out
        torch.cuda.empty_cache()
        stacked = torch.empty((P, N, STEPS * F), dtype=torch.float32, device="cuda")
        row["ours"]["stack_memory"] = timed(lambda: jsg.stack_memory_launch(x, stacked, n_steps=STEPS, delay=DELAY), reps, torch)
        row["stack_share_of_roof"] = (1 + STEPS) * plane_bytes / row["ours"]["stack_memory"][1] / roof
        del stacked

        def rolled():
            parts = [x]
            for s in range(1, STEPS):
                r = torch.roll(x, s * DELAY, dims=1)
                r[:, :s * DELAY] = 0
                parts.append(r)
            return torch.cat(parts, dim=2)
        try:
            row["torch"]["stack_memory"] = timed(rolled, max(3, reps // 4), torch)
        except Exception as err:
            row["torch"]["stack_memory"] = str(err)[:120]
        results.append(row)
        print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        json.dump(dict(lib=os.path.basename(lib) if lib else "product", device=torch.cuda.get_device_name(0), reps=reps, results=results), f, indent=1)


def report(md_path, json_path, *variant_paths):
    data = json.load(open(json_path))
    ms = lambda v: f"{v[1] * 1e3:.3f}" if isinstance(v, list) else "failed"
    lines = ["# Segment aggregation and time-delay embedding: measured times", "",
             f"`python tools/sync_bench.py --run` on one MI355X (\"{data['device']}\" to torch): median of {data['reps']} launches (HIP events, after 3 warm-up calls), in",
             "milliseconds.  `torch`: `torch.segment_reduce` (mean, min, max; on a plane transposed to frames-first beforehand, not timed), a",
             "padded gather + `torch.nanmedian` (median), `torch.roll` + `cat` (stacking, 5 steps), on the same GPU in the same run.  The share of the",
             "copy roof is the bytes the operation must move (the plane read once, the output written once) over its time, against the bytes a",
             "second of a device-to-device copy of the same plane measured here; a stream that is almost all reads can pass 100 % of it.  The",
             "slower cases are in the tables as measured: the median of segments of 131072 frames is 17 times slower than torch's.", ""]
    for r in data["results"]:
        lines += [f"## {r['pairs']} x {r['frames']} x {r['features']}, {r['boundaries']} ({r['segments']} segments a plane)", "",
                  f"copy of the plane: {ms(r['copy_s'])} ms ({r['roof_bytes_per_s'] / 1e12:.2f} TB/s moved)", "",
                  "| operation | jsgx (ms) | torch (ms) | share of the copy roof |", "|---|---|---|---|"]
        for op in AGGS + ("stack_memory",):
            share = r["mean_share_of_roof"] if op == "mean" else r["stack_share_of_roof"] if op == "stack_memory" else None
            lines.append(f"| {op} | {ms(r['ours'][op])} | {ms(r['torch'].get(op))} | {'' if share is None else f'{100 * share:.0f} %'} |")
        lines.append("")
    if variant_paths:
        variants = [json.load(open(v)) for v in variant_paths]
        lines += ["## The median with a form left out", "",
                  "Builds with `-DJSGX_SYNC_WAVE_MAX=0` (`noalone`: never a wavefront a segment, always the four wavefronts together, staged in LDS up to",
                  "256 frames) and with `-DJSGX_SYNC_STAGE=0` on top (`nostage`: nothing staged, all 32 passes read the plane through the caches), the",
                  "same launches one process after the other, milliseconds.", "", "| shape | product | " + " | ".join(v["lib"] for v in variants) + " |", "|---|---|" + "---|" * len(variants)]
        for i, r in enumerate(data["results"]):
            lines.append(f"| {r['pairs']} x {r['frames']} x {r['features']}, {r['boundaries']} | {ms(r['ours']['median'])} | " + " | ".join(ms(v["results"][i]["ours"]["median"]) for v in variants) + " |")
        lines.append("")
    with open(md_path, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--report", nargs="+")
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--median-only", action="store_true")
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
    if a.run:
        run(a.run, a.reps, a.lib, a.median_only)
    if a.report:
        report(*a.report)
