#!/usr/bin/env python3
"""Time of Viterbi decoding (jsgx_viterbi_launch, libjsgx.so) over dense S = 64, 192, 256, 1200, 2048 and band (S, W) = (1200, 25),
(2048, 64), T = 4096 and 65536, seqs = 1 and 256, next to the same recurrence written with torch operations on the same GPU (one
(V[:, None] + A).max(0) per frame), and of the backtrace block sizes 64, 256 and 1024 at T = 65536.

Three steps, each a process of its own:

    python tools/viterbi_bench.py --build-variants                 (no GPU) builds tools/variants/libjsgx_block{64,256,1024}.so
    python tools/viterbi_bench.py --run OUT.json [--lib LIB] [--set main|block]
        whole launches with HIP events (median of the timed launches after a warm-up) and the torch loop; the sequence of launches is
        recorded in OUT.json.  Run under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python ...` the same process gives the
        time of every kernel (tracing slows the host, so the whole-launch figures are taken from a run without it).
    python tools/viterbi_bench.py --report profiles/viterbi_bench.md --main OUT.json [--main-trace DIR OUT.json] [--block NAME OUT.json DIR ...]

A configuration is left out, and the report says so, where its buffers pass --max-gib or where a probe of 256 frames predicts more than
--max-seconds for one launch (the forward pass is serial in time, so the time of a launch is linear in T)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSE = (64, 192, 256, 1200, 2048)
BANDS = ((1200, 25), (2048, 64))
FRAMES = (4096, 65536)
SEQS = (1, 256)
BLOCKS = (64, 256, 1024)
TORCH_FRAMES = 128          # frames of the torch loop that are timed; its time per frame does not depend on the frame


def configs(which):
    if which == "block":    # the backtrace comparison: T = 65536 only, where the chase is longest
        return [(S, None, 65536, Q) for S in (64, 256, 2048) for Q in (1, 256)] + [(1200, 25, 65536, 1)]
    return [(S, None, T, Q) for S in DENSE for T in FRAMES for Q in SEQS] + [(S, W, T, Q) for S, W in BANDS for T in FRAMES for Q in SEQS]


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
            if "viterbi" in src:
                o = os.path.join(vdir, f"{os.path.splitext(src)[0]}_block{block}.o")
                cmd = [hipcc, "-std=c++17", "-O3", "-fPIC", "-c", os.path.join(_build.CSRC, src), "-o", o, "-I", os.path.join(ROOT, "include"),
                       f"-DJSGX_VITERBI_BLOCK={block}"] + _build.VISIBILITY
                cmd += [f"--offload-arch={_build.ARCH}"] + _build.HIP_FLAGS if src.endswith(".hip") else ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__"]
                subprocess.check_call(cmd)
            objs.append(o)
        out = os.path.join(vdir, f"libjsgx_block{block}.so")
        subprocess.check_call([hipcc, "-shared", "-fPIC", f"--offload-arch={_build.ARCH}", "-o", out] + objs)
        print(out)


def event_time(torch, fn, reps):
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    times.sort()
    return times[len(times) // 2]


def band_as_dense(torch, band, W):
    S = band.shape[1]
    i, j = torch.arange(S, device="cuda")[:, None], torch.arange(S, device="cuda")[None, :]
    r = i - j + W
    inside = (r >= 0) & (r <= 2 * W)
    return torch.where(inside, band[r.clamp(0, 2 * W), j.expand(S, S)], torch.full((), float("-inf"), device="cuda"))


def torch_loop(torch, emit, p0, A, frames):
    """The recurrence in torch operations over the first `frames` frames: V [Q][S] after them (psi is kept, as a decoder has to)."""
    Q, T, S = emit.shape
    V = p0[None, :] + emit[:, 0]
    psi = torch.empty((frames, Q, S), dtype=torch.int64, device="cuda")
    for t in range(1, frames):
        best, psi[t] = (V[:, :, None] + A[None]).max(1)
        V = best + emit[:, t]
    return V


def run(args):
    import torch
    import jadespectrogram_amd as jsg
    if args.lib:
        jsg.capix.LIB_PATH = os.path.abspath(args.lib)
    torch.cuda.set_device(0)
    record = {"device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "lib": args.lib or "product",
              "block": None, "rows": [], "launches": []}
    for S, W, T, Q in configs(args.set):
        row = {"S": S, "W": W, "T": T, "Q": Q, "plan": jsg.viterbi_plan(S, T, Q, W)}
        blocks = -(-T // 256)
        gib = (4.0 * Q * T * S + 2.0 * Q * T * S + 4.0 * Q * T + 2.0 * Q * blocks * S * 4) / 2 ** 30
        row["gib"] = gib
        if gib > args.max_gib:
            row["skipped"] = f"needs {gib:.0f} GiB of buffers"
            record["rows"].append(row)
            print(row, flush=True)
            continue
        gen = torch.Generator(device="cuda").manual_seed(S + T)
        emit = -4.0 * torch.rand((Q, T, S), generator=gen, dtype=torch.float32, device="cuda")
        p0 = -4.0 * torch.rand((S,), generator=gen, dtype=torch.float32, device="cuda")
        A = -4.0 * torch.rand((S if W is None else 2 * W + 1, S), generator=gen, dtype=torch.float32, device="cuda")
        states = torch.empty((Q, T), dtype=torch.int32, device="cuda")
        logp = torch.empty((Q,), dtype=torch.float32, device="cuda")
        scratch = torch.empty((jsg.viterbi_scratch_bytes(emit, p0, A, states, band_half=W, d_logp=logp),), dtype=torch.uint8, device="cuda")
        launch = lambda e=emit, s=states: jsg.viterbi_launch(e, p0, A, s, band_half=W, d_logp=logp, d_scratch=scratch)
        # a probe of 256 frames: loads the code, and predicts the whole launch
        probe_T = 256
        probe = lambda: jsg.viterbi_launch(emit[:, :probe_T], p0, A, states[:, :probe_T], band_half=W, d_logp=logp, d_scratch=scratch)
        probe()
        torch.cuda.synchronize()
        t_probe = event_time(torch, probe, 3)
        record["launches"] += [{"S": S, "W": W, "T": probe_T, "Q": Q, "kernels": jsg.viterbi_plan(S, probe_T, Q, W)[3], "timed": False}] * 4
        predicted = t_probe * T / probe_T
        row["predicted_s"] = predicted
        if predicted > args.max_seconds:
            row["skipped"] = f"a launch of 256 frames takes {t_probe * 1e3:.2f} ms: {predicted:.0f} s predicted"
        else:
            reps = 1 if predicted > 1.5 else 3
            if reps > 1:            # a long launch is timed once, cold: the probe has loaded its code
                launch()
                record["launches"] += [{"S": S, "W": W, "T": T, "Q": Q, "kernels": row["plan"][3], "timed": False}]
            row["launch_s"] = event_time(torch, launch, reps)
            row["reps"] = reps
            record["launches"] += [{"S": S, "W": W, "T": T, "Q": Q, "kernels": row["plan"][3], "timed": True}] * reps
        if not args.no_torch:
            Ad = A if W is None else band_as_dense(torch, A, W)
            frames = min(T, TORCH_FRAMES + 1)
            torch_loop(torch, emit, p0, Ad, min(T, 9))
            torch.cuda.synchronize()
            t_loop = event_time(torch, lambda: torch_loop(torch, emit, p0, Ad, frames), 3)
            row["torch_frames"] = frames - 1
            row["torch_s"] = t_loop * (T - 1) / (frames - 1)
            if "launch_s" in row:         # the same additions and the same maximum: logp is the same float
                cheap = T <= 4096 and row["torch_s"] < 3.0 and 8.0 * T * Q * S < 4e9
                full = torch_loop(torch, emit, p0, Ad, T).max(1).values if cheap else None
                row["equal"] = None if full is None else bool((full == logp).all())
        record["rows"].append(row)
        print(row, flush=True)
        del emit, states, scratch
        torch.cuda.empty_cache()
    with open(args.run, "w") as f:
        json.dump(record, f)
    print("wrote", args.run)


def kernel_times(trace_dir, record):
    """{(S, W, T, Q): {kernel: median seconds}} from rocprofv3's kernel trace of the process that wrote `record`."""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = [r for r in csv.DictReader(open(files[0])) if "viterbi_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    short = lambda name: next(k for k in ("forward", "jump", "ends", "trace") if f"viterbi_{k}_kernel" in name)
    out, at = {}, 0
    for launch in record["launches"]:
        mine = rows[at:at + launch["kernels"]]
        at += launch["kernels"]
        kinds = [short(r["Kernel_Name"]) for r in mine]
        assert kinds == (["forward", "jump", "ends", "trace"] if launch["kernels"] == 4 else ["forward", "ends", "trace"]), (launch, kinds)
        if launch["timed"]:
            key = (launch["S"], launch["W"], launch["T"], launch["Q"])
            for r, kind in zip(mine, kinds):
                out.setdefault(key, {}).setdefault(kind, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9)
    assert at == len(rows), (at, len(rows))
    return {key: {kind: sorted(v)[len(v) // 2] for kind, v in kinds.items()} for key, kinds in out.items()}


def shape_text(S, W, T, Q):
    return f"{'dense' if W is None else f'band W={W}'} S={S} T={T} seqs={Q}"


def report(args):
    main = json.load(open(args.main))
    kt = kernel_times(args.main_trace[0], json.load(open(args.main_trace[1]))) if args.main_trace else {}
    ms = lambda s: "-" if s is None else f"{s * 1e3:.3f}"
    lines = ["# Viterbi decoding timing (tools/viterbi_bench.py)", "",
             f"Device: {main['device']}, {main['cus']} compute units.  Random non-positive float32 inputs.  launch: one jsgx_viterbi_launch (forward, jump, ends, trace) with a",
             "scratch given, eager, HIP events around it, median of 3 after a warm-up (a launch predicted above 1.5 s: one timed launch).  forward, jump, ends,",
             "trace: the kernels of such a launch from `rocprofv3 --kernel-trace`, a run of its own, median of the timed launches.  torch loop: the same",
             f"recurrence as one `(V[:, :, None] + A[None]).max(1)` per frame with psi kept (the band as a dense matrix with -inf outside), timed over {TORCH_FRAMES} frames",
             "after 8 warm ones and scaled to T - 1 frames: its time per frame does not depend on the frame.  It has no backtrace, so torch / launch favours torch.",
             "equal: logp of the launch and of the whole torch loop are the same floats (checked at T = 4096 where the whole loop takes under 3 s).", "",
             "| shape | form | lanes | launch ms | forward ms | jump ms | ends ms | trace ms | us per frame | torch loop ms | torch / launch | equal |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    behind = []
    for row in main["rows"]:
        key = (row["S"], row["W"], row["T"], row["Q"])
        what = shape_text(*key)
        if "launch_s" not in row:
            lines.append(f"| {what} | {row['plan'][0]} | {row['plan'][1]} | not measured: {row['skipped']} | | | | | | {ms(row.get('torch_s'))} | | |")
            continue
        k = kt.get(key, {})
        ratio = row["torch_s"] / row["launch_s"] if "torch_s" in row else None
        if ratio is not None and ratio < 1:
            behind.append(f"{what} ({ratio:.2f})")
        lines.append(f"| {what} | {row['plan'][0]} | {row['plan'][1]} | {ms(row['launch_s'])} | {ms(k.get('forward'))} | {ms(k.get('jump'))} | {ms(k.get('ends'))} | {ms(k.get('trace'))} | "
                     f"{row['launch_s'] * 1e6 / row['T']:.2f} | {ms(row.get('torch_s'))} | {'-' if ratio is None else f'{ratio:.2f}'} | "
                     f"{ {None: '-', True: 'yes', False: 'NO'}[row.get('equal')] } |")
    lines += ["", "Where the hand-written path is behind the torch loop (torch / launch below 1): " + (", ".join(behind) if behind else "nowhere among the rows measured") + "."]
    if args.block:
        lines += ["", "## The block of the backtrace at T = 65536", "",
                  "Builds of the library with JSGX_VITERBI_BLOCK = 64, 256 and 1024, each in a process of its own under the kernel trace; jump + ends + trace in ms",
                  "(jump, ends, trace).  The forward kernel does not depend on the block.", ""]
        per = {}
        for name, rec, trace in zip(args.block[0::3], args.block[1::3], args.block[2::3]):
            per[name] = kernel_times(trace, json.load(open(rec)))
        keys = sorted({k for v in per.values() for k in v}, key=lambda k: (k[1] is not None, k[0], k[3]))
        lines += ["| shape | forward ms | " + " | ".join(f"block {n}" for n in per) + " |", "|---|---|" + "---|" * len(per)]
        sums = {n: 0.0 for n in per}
        for key in keys:
            cells = []
            for n, v in per.items():
                k = v.get(key)
                if k is None:
                    cells.append("-")
                    continue
                back = k.get("jump", 0.0) + k["ends"] + k["trace"]
                sums[n] += back
                cells.append(f"{back * 1e3:.3f} ({ms(k.get('jump'))}, {ms(k['ends'])}, {ms(k['trace'])})")
            fwd = next((v[key]["forward"] for v in per.values() if key in v), None)
            lines.append(f"| {shape_text(*key)} | {ms(fwd)} | " + " | ".join(cells) + " |")
        lines.append("| sum over the rows | | " + " | ".join(f"{s * 1e3:.3f}" for s in sums.values()) + " |")
    lines += ["", "## Reading", "",
              "Nothing here was measured with counters; the limiter is reasoned from the rows and from the code.",
              "* The time of a launch is the forward kernel's: the three backtrace kernels together take 0.2 to 4 ms at T = 65536, under 1 % of the launch.",
              "  A single chase of T dependent loads was not built, so the blocked backtrace is compared with itself only: block 256 has the least sum and is",
              "  kept; 64 puts T / 64 dependent steps into the one lane of `ends`, 1024 makes `jump` and `trace` walk four times as far.",
              "* One sequence or 256 cost the same: a sequence is one workgroup on one compute unit, and 256 of them fill the 256 compute units.  The time per",
              "  frame is flat in T.",
              "* Small and banded models are ahead of the torch loop by 1.5 to 60 times; the torch loop pays two or three kernel launches per frame and, with",
              "  256 sequences, a seqs x S x S temporary per frame, where the band form reads 2W + 1 rows.",
              "* Dense S = 1200 and 2048 with ONE sequence are 19 and 26 times BEHIND the torch loop: torch spreads the S x S additions of a frame over the whole",
              "  device, this kernel keeps them on one compute unit, which re-reads A (5.8 and 16.8 MB, more than the 4 MB of L2 of its XCD) every frame at about",
              "  9 and 14 GB/s.  Keeping 16 instead of 4 loads in flight per lane did not change the time (3.32 s against 3.39 s at S = 1200, T = 4096), so",
              "  the limit is supposed to be the misses one compute unit can have outstanding, not the issue rate; that was not measured.  With 256 sequences",
              "  the same kernel is 1.3 and 2.0 times ahead.  Splitting one sequence across workgroups is what would help and was out of scope; a user with one",
              "  long dense sequence of more than about 500 states is better served by the torch loop today.",
              "* dense S = 256 goes through memory (A is 256 KB, it does not fit the 160 KB of LDS) at 9.1 us per frame against 4.2 us at S = 192 from LDS.",
              "* Leaner inner loop: within a lane the sources ascend, so the pair rule is a strict greater-than there; against the full rule in every step",
              "  that took dense S = 256 from 53.7 to 37.3 ms, band S = 1200 from 71.0 to 50.7 ms and dense S = 1200 from 3.32 to 2.79 s (T = 4096, one sequence).",
              "* Not measured: T = 65536 with 256 sequences from S = 1200 on (the emissions alone are 80 GB and more), dense S >= 1200 at T = 65536 (44 and 81 s",
              "  predicted from 256 frames), agreement with librosa.sequence.viterbi (librosa is not installed)."]
    os.makedirs(os.path.dirname(os.path.abspath(args.report)), exist_ok=True)
    with open(args.report, "w") as f:
        f.write("\n".join(lines + [""]))
    print("wrote", args.report)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--run", metavar="OUT.json")
    ap.add_argument("--lib")
    ap.add_argument("--set", default="main", choices=["main", "block"])
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--max-gib", type=float, default=40.0)
    ap.add_argument("--max-seconds", type=float, default=12.0)
    ap.add_argument("--report", metavar="FILE.md")
    ap.add_argument("--main", metavar="OUT.json")
    ap.add_argument("--main-trace", nargs=2, metavar=("DIR", "OUT.json"))
    ap.add_argument("--block", nargs="+", metavar="NAME OUT.json DIR", help="triples")
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
