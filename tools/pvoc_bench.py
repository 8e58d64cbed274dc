#!/usr/bin/env python3
"""Phase vocoder throughput (jsg_pvoc_launch) next to the same formula written in torch ops on the same device and next to a
jsg_calib_copy_launch that moves the same number of bytes.  Writes profiles/pvoc_bench.md.  HIP events around each dispatch; every
timed dispatch touches >= 1 GB of distinct data (input frames read once + output frames written once: the algorithmic bytes).

    python tools/pvoc_bench.py [--reps R] [--out FILE] [--gb G]
"""
import argparse
import ctypes as C
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(n, n // 4, rows, rate) for n, rows in ((1024, 1), (4096, 1), (1024, 16)) for rate in (0.5, 1.0, 2.0)]


def timed(fn, reps, torch):
    for _ in range(2):
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


def torch_formula(X, rate, hop, n):
    """torchaudio.functional.phase_vocoder's chain of torch ops on frame-major [rows][T][K] (float32 phase, cumsum along time)."""
    import torch
    import torch.nn.functional as Fn
    T, K = X.shape[1], X.shape[2]
    steps = torch.arange(0, T, rate, device=X.device, dtype=torch.float64)
    idx = steps.floor().long()
    alphas = (steps - idx).float()[None, :, None]
    Xp = Fn.pad(X, (0, 0, 0, 2))
    a0, a1 = Xp[:, idx], Xp[:, idx + 1]
    adv = (2 * math.pi * hop / n * torch.arange(K, device=X.device, dtype=torch.float64)).float()[None, None, :]
    ph = a1.angle() - a0.angle() - adv
    ph = ph - 2 * math.pi * torch.round(ph / (2 * math.pi)) + adv
    ph = torch.cat([X[:, :1].angle(), ph[:, :-1]], dim=1)
    mag = alphas * a1.abs() + (1 - alphas) * a0.abs()
    return torch.polar(mag, torch.cumsum(ph, dim=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gb", type=float, default=1.0, help="algorithmic bytes per dispatch, at least (GB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvoc_bench.md"))
    args = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    lib = jsg.capi.lib()
    torch.cuda.set_device(0)
    lines = ["# Phase vocoder throughput (tools/pvoc_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}; best (median) of {args.reps} timed dispatches after 2 warm-up dispatches, HIP events, "
             f"each dispatch >= {args.gb:g} GB of distinct data.",
             "Bytes: the input frames read once + the output frames written once, 8 bytes per bin (the library reads the input twice: once",
             "for the chunk sums, once for the output; that second read is in its time, not in its bytes).  copy = jsg_calib_copy_launch moving",
             "the same bytes (half read, half written).  torch = the same formula as a chain of torch ops (float32 cumsum along time).", "",
             "| n / hop | rows | rate | T -> T_out | GB | jsg ms | jsg TB/s | copy ms | copy TB/s | jsg / copy rate | torch ms | torch / jsg time |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, hop, rows, rate in CASES:
        K = n // 2 + 1
        T = int(args.gb * 1e9 / (8 * K * rows * (1 + 1 / rate))) + 1
        T_out = jsg.pvoc_frames(T, rate)
        nbytes = 8 * K * rows * (T + T_out)
        X = torch.view_as_complex(torch.randn((rows, T, K, 2), device="cuda"))
        out = torch.empty((rows, T_out, K), dtype=torch.complex64, device="cuda")
        a = jsg.spectrogram._pvoc_args(X, rate, hop, n, out, 0)
        sc = torch.empty(lib.jsg_pvoc_scratch_bytes(C.byref(a)) // 4, dtype=torch.int32, device="cuda")
        t_j, t_j_med = timed(lambda: jsg.phase_vocoder_launch(X, rate, hop, n, out, d_scratch=sc), args.reps, torch)
        half = nbytes // 2 // 16 * 16
        src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        t_c, t_c_med = timed(lambda: jsg.capi.check(lib.jsg_calib_copy_launch(src.data_ptr(), dst.data_ptr(), half, C.c_void_p(stream))), args.reps, torch)
        del src, dst
        t_t, t_t_med = timed(lambda: torch_formula(X, rate, hop, n), max(3, args.reps // 2), torch)
        gb = nbytes / 1e9
        lines.append(f"| {n} / {hop} | {rows} | {rate:g} | {T} -> {T_out} | {gb:.2f} | {t_j * 1e3:.3f} ({t_j_med * 1e3:.3f}) | {gb / t_j / 1e3:.2f} | "
                     f"{t_c * 1e3:.3f} ({t_c_med * 1e3:.3f}) | {2 * half / 1e9 / t_c / 1e3:.2f} | {(gb / t_j) / (2 * half / 1e9 / t_c):.2f} | "
                     f"{t_t * 1e3:.2f} ({t_t_med * 1e3:.2f}) | {t_t / t_j:.1f}x |")
        print(lines[-1], flush=True)
        del X, out, sc
        torch.cuda.empty_cache()
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
