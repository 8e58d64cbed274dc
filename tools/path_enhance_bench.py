#!/usr/bin/env python3
"""Time of path enhancement (jsgx_path_enhance_launch, libjsgx.so) with librosa's default bank at n = 51 (seven filters, about 3200 taps)
on 64 planes of 512 x 512, on one 4096 x 4096 and on one 16384 x 16384 affinity-like plane, interleaved with a torch route on the same GPU:
conv2d with the seven dense tables as output channels, then amax over the channels.  Medians of HIP-event timings; fused multiply-adds per
second against the vector peak.  Then the time-lag conversion (jsgx_lag_launch) in bytes per second against a device copy of the same bytes
measured in the same session.  Writes profiles/path_enhance_bench.md.

A plane with more rows than --tile-torch-above (4096) takes the torch route in tiles of that many rows and columns that overlap by the
reach, each one the conv2d call of the 4096 x 4096 workload: the first conv2d call of a shape searches for a solver for minutes (226 s at
4096 x 4096), and at 16384 x 16384 that search alone did not end in seven minutes.

    python tools/path_enhance_bench.py [--reps R] [--torch-reps R] [--out FILE] [--regs FILE] [--tile-torch-above N]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dtw_bench import replayed, timed  # noqa: E402

WORKLOADS = ((64, 512, 512), (1, 4096, 4096), (1, 16384, 16384))        # pairs, N, M
N_WINDOW = 51
CLOCK_HZ = 2.4e9            # the clock the peak figures are stated for


def dense_tables(np, tap_w, tap_at, first, ri, rj):
    """The bank as conv2d weights [F][1][2 ri + 1][2 rj + 1]: conv2d correlates, so the tap (di, dj) sits at [di + ri][dj + rj]."""
    import path_enhance_ref as pr
    di, dj = pr.unpack(tap_at)
    K = np.zeros((len(first) - 1, 1, 2 * ri + 1, 2 * rj + 1), np.float32)
    for f in range(len(first) - 1):
        s = slice(int(first[f]), int(first[f + 1]))
        K[f, 0, di[s] + ri, dj[s] + rj] = tap_w[s]
    return K


def timed_aloud(torch, fn, reps, what):
    """dtw_bench.timed with one warm-up run and a line of progress per run: a run of the torch route at the largest size takes seconds."""
    times = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        print(f"  {what}: run {k} {a.elapsed_time(b):.2f} ms" + (" (warm-up)" if k == 0 else ""), flush=True)
        if k > 0:
            times.append(a.elapsed_time(b) * 1e-3)
    times.sort()
    return times[len(times) // 2], times[0]


def plane(torch, P, N, M, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    R = torch.rand((P, N, M), generator=gen, dtype=torch.float32, device="cuda")
    return R * (torch.rand((P, N, M), generator=gen, dtype=torch.float32, device="cuda") < 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_enhance_bench.md"))
    ap.add_argument("--regs", help="the output of tools/kernel_regs.py for jsgx_path_enhance.o, copied into the report")
    ap.add_argument("--tile-torch-above", type=int, default=4096, help="the torch route of a plane with more rows than this runs in overlapping tiles of this size")
    args = ap.parse_args()
    import numpy as np
    import torch
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    peak_plain, peak_packed = cus * 64 * CLOCK_HZ, cus * 128 * CLOCK_HZ
    tap_w, tap_at, first, ri, rj = jsg.path_enhance_filters(N_WINDOW)
    T = len(tap_w)
    name, tr, tc, threads, lds = jsg.path_enhance_plan(ri, rj)
    d_w, d_at, d_first = (torch.from_numpy(a).cuda() for a in (tap_w, tap_at, first))
    d_K = torch.from_numpy(dense_tables(np, tap_w, tap_at, first, ri, rj)).cuda()
    dense = int(d_K[0].numel()) * d_K.shape[0]
    lines = ["# Path enhancement and time-lag conversion timing (tools/path_enhance_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}, {cus} compute units.  Kernel: median (best) of {args.reps} timed replays of a captured graph after 2 warm-up replays, HIP "
             f"events.  torch route: median (best) of {args.torch_reps} eager runs after 1 warm-up run, HIP events, interleaved with the kernel per workload.", "",
             f"Bank: `path_enhance_filters({N_WINDOW})`, {len(first) - 1} filters, {T} taps (filters of {', '.join(str(int(b - a)) for a, b in zip(first[:-1], first[1:]))}), reach "
             f"{ri} x {rj}.  Kernel `{name}`: tiles of {tr} x {tc}, {threads} lanes, {lds} bytes of LDS a workgroup.  Planes: uniform floats, 5 % of the cells non-zero.",
             f"torch route: `amax(conv2d(R[:, None], K, padding=({ri}, {rj})), dim=1)` with K the seven tables as dense {2 * ri + 1} x {2 * rj + 1} float32 channels "
             f"({dense} weights, {dense / T:.1f} x the taps).  A plane with more than {args.tile_torch_above} rows takes it in tiles of {args.tile_torch_above} x {args.tile_torch_above} inputs that "
             "overlap by the reach, each the conv2d call of the workload above it (the plane in a zeroed canvas built outside the timing; the cut and the copy of a tile are timed).",
             f"FMA/s counts the taps only ({T} a cell), for both routes.  Peaks at {CLOCK_HZ / 1e9:.1f} GHz: {peak_plain / 1e12:.1f} T FMA/s for v_fma_f32 (64 lanes a compute unit and "
             f"clock), {peak_packed / 1e12:.1f} T FMA/s for v_pk_fma_f32 (the 157 TFLOPS of the data sheet).", "",
             "| pairs x N x M | kernel ms | T FMA/s | of v_fma peak | torch ms | torch T FMA/s (taps) | torch / kernel | max abs difference | cells not equal in bits |",
             "|---|---|---|---|---|---|---|---|---|"]
    results = []
    for P, N, M in WORKLOADS:
        R = plane(torch, P, N, M, N)
        out = torch.empty_like(R)
        t_k = replayed(torch, lambda s: jsg.path_enhance_launch(R, d_w, d_at, d_first, out, reach_i=ri, reach_j=rj, stream=s), args.reps)
        fma = float(P) * N * M * T
        row = f"| {P} x {N} x {M} | {t_k[0] * 1e3:.3f} ({t_k[1] * 1e3:.3f}) | {fma / t_k[0] / 1e12:.2f} | {fma / t_k[0] / peak_plain:.1%} |"
        print(row, flush=True)
        conv = lambda x: torch.amax(torch.nn.functional.conv2d(x, d_K, padding=(ri, rj)), dim=1)
        if N <= args.tile_torch_above:
            route = lambda: torch.clamp_min(conv(R[:, None]), 0.0)
            how = ""
        else:
            # tiles of side x side inputs whose inner (side - 2 ri) x (side - 2 rj) outputs are kept; the plane sits in a zeroed canvas, built outside the timing
            side = args.tile_torch_above
            si, sj = side - 2 * ri, side - 2 * rj
            ni, nj = -(-N // si), -(-M // sj)
            canvas = torch.zeros((ni * si + 2 * ri, nj * sj + 2 * rj), dtype=torch.float32, device="cuda")
            canvas[ri:ri + N, rj:rj + M] = R[0]
            whole = torch.empty((ni * si, nj * sj), dtype=torch.float32, device="cuda")

            def route():
                for a in range(ni):
                    for b in range(nj):
                        x = canvas[a * si:a * si + side, b * sj:b * sj + side].contiguous()[None, None]
                        whole[a * si:(a + 1) * si, b * sj:(b + 1) * sj] = conv(x)[0, ri:ri + si, rj:rj + sj]
                return torch.clamp_min(whole[:N, :M], 0.0)[None]
            how = f" in {ni} x {nj} tiles"
        t_t = timed_aloud(torch, route, args.torch_reps, f"torch route {P} x {N} x {M}")
        ref = route()
        diff = float((ref - out).abs().max())
        unequal = int((ref.view(torch.int32) != out.view(torch.int32)).sum())
        del ref
        # the kernel again behind the torch route: the order does not matter
        t_k2 = replayed(torch, lambda s: jsg.path_enhance_launch(R, d_w, d_at, d_first, out, reach_i=ri, reach_j=rj, stream=s), args.reps)
        row += f" {t_t[0] * 1e3:.2f} ({t_t[1] * 1e3:.2f}){how} | {fma / t_t[0] / 1e12:.2f} | {t_t[0] / t_k[0]:.2f} | {diff:.2e} | {unequal} of {P * N * M} |"
        results.append((P, N, M, t_k, t_t, t_k2))
        if N > args.tile_torch_above:
            del canvas, whole
        lines.append(row)
        print(row, flush=True)
        del R, out
        torch.cuda.empty_cache()
    lines += ["", "The kernel a second time, behind the torch route of the same workload (ms): " +
              ", ".join(f"{P} x {N} x {M}: {t2[0] * 1e3:.3f}" for P, N, M, _, _, t2 in results if t2 is not None) + "."]
    # ---- single filters: what the run length is worth
    lines += ["", "## One filter alone (1 x 4096 x 4096)", "", "| filter | taps | kernel ms | T FMA/s |", "|---|---|---|---|"]
    R = plane(torch, 1, 4096, 4096, 7)
    out = torch.empty_like(R)
    for f in range(len(first) - 1):
        one = torch.tensor([int(first[f]), int(first[f + 1])], dtype=torch.int32, device="cuda")
        t1 = replayed(torch, lambda s: jsg.path_enhance_launch(R, d_w, d_at, one, out, reach_i=ri, reach_j=rj, stream=s), args.reps)
        taps = int(first[f + 1] - first[f])
        lines.append(f"| {f} | {taps} | {t1[0] * 1e3:.3f} | {4096.0 * 4096 * taps / t1[0] / 1e12:.2f} |")
        print(lines[-1], flush=True)
    none = torch.tensor([0, 0], dtype=torch.int32, device="cuda")
    t0 = replayed(torch, lambda s: jsg.path_enhance_launch(R, d_w, d_at, none, out, reach_i=ri, reach_j=rj, stream=s), args.reps)
    lines += ["", f"A filter without taps (the staging of the window and the store alone): {t0[0] * 1e3:.3f} ms."]
    del R, out
    # ---- the lag conversion against a copy
    lines += ["", "## Time-lag conversion (jsgx_lag_launch), pad on", "",
              "Bytes: the input plane once and the output plane once.  copy: `torch.Tensor.copy_` of as many bytes (half read, half written) in the same session.", "",
              "| pairs x N | form | ms | TB/s | copy ms | copy TB/s | of the copy |", "|---|---|---|---|---|---|---|"]
    for P, N in ((64, 512), (1, 4096), (1, 16384)):
        R = plane(torch, P, N, N, N + 1)
        for axis, inverse, form in ((1, False, "lag_columns to lag"), (1, True, "lag_columns from lag"), (0, False, "lag_rows to lag"), (0, True, "lag_rows from lag")):
            lag = torch.empty((P, 2 * N, N) if axis == 1 else (P, N, 2 * N), dtype=torch.float32, device="cuda")
            jsg.lag_launch(R, lag, axis=axis)
            back = torch.empty_like(R)
            a, b = (lag, back) if inverse else (R, lag)
            t = replayed(torch, lambda s: jsg.lag_launch(a, b, axis=axis, inverse=inverse, stream=s), args.reps)
            nbytes = 4.0 * (a.numel() + b.numel())
            src = torch.empty((int(nbytes // 8),), dtype=torch.float32, device="cuda")
            dst = torch.empty_like(src)
            t_c = timed(torch, lambda: dst.copy_(src), args.reps)
            lines.append(f"| {P} x {N} | {form} | {t[0] * 1e3:.3f} ({t[1] * 1e3:.3f}) | {nbytes / t[0] / 1e12:.2f} | {t_c[0] * 1e3:.3f} | {nbytes / t_c[0] / 1e12:.2f} | {t_c[0] / t[0]:.0%} |")
            print(lines[-1], flush=True)
            del lag, back, src, dst
        del R
    if args.regs and os.path.exists(args.regs):
        lines += ["", "## Registers and LDS (tools/kernel_regs.py on jsgx_path_enhance.o)", "", "```"] + open(args.regs).read().rstrip().splitlines() + ["```"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + [""]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
