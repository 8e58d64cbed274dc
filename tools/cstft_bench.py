#!/usr/bin/env python3
"""Complex STFT / inverse STFT throughput (jsg_cstft_launch, jsg_istft_launch) against torch.stft / torch.istft on the same device.
Writes profiles/cstft_bench.md.  HIP events around each dispatch; every timed dispatch moves >= 1 GB of distinct data.

Algorithmic bytes: forward = the input read once (rows * ((F-1) hop + n) floats) + 8 (n/2+1) bytes per frame; inverse = the reverse
(the bins read once + the output samples written once).  The roof is 8 TB/s.

    python tools/cstft_bench.py [--reps R] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8e12
CASES = [(1024, 512, 1), (1024, 512, 8), (2048, 480, 1), (4096, 1024, 1)]


def timed(fn, reps, torch):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cstft_bench.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    lines = ["# Complex STFT / inverse STFT throughput (tools/cstft_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}; best of {args.reps} timed dispatches (HIP events), each >= 1 GB of distinct data.",
             "Bytes: forward = input read once + 8 (n/2+1) per frame; inverse = the reverse.  Roof 8 TB/s.", "",
             "| direction | n / hop | rows | frames per row | GB | jsg time (ms) | jsg TB/s | of roof | torch time (ms) | torch TB/s | jsg / torch |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n, hop, rows in CASES:
        N1 = n // 2 + 1
        per_frame = 8 * N1 + 4 * hop
        F = int(1.0e9 / per_frame / rows) + 1
        L = (F - 1) * hop + n
        gb = (rows * L * 4 + rows * F * 8 * N1) / 1e9
        w = torch.hann_window(n)
        plan = jsg.CStftPlan(n, w.numpy())
        x = torch.randn((rows, L), device="cuda")
        X = torch.empty((rows, F, N1), dtype=torch.complex64, device="cuda")
        t_f = timed(lambda: jsg.cstft(plan, x, hop, F, X), args.reps, torch)
        wd = w.cuda()
        t_tf = timed(lambda: torch.stft(x, n, hop, window=wd, center=False, return_complex=True), args.reps, torch)
        lines.append(f"| forward | {n} / {hop} | {rows} | {F} | {gb:.2f} | {t_f * 1e3:.3f} | {gb / t_f / 1e3:.2f} | {gb * 1e9 / t_f / ROOF:.2f} | "
                     f"{t_tf * 1e3:.3f} | {gb / t_tf / 1e3:.2f} | {t_tf / t_f:.2f}x |")
        y = torch.empty((rows, L), device="cuda")
        sc = torch.empty(jsg.istft_scratch_floats(plan, X, hop, F, y), device="cuda")
        t_i = timed(lambda: jsg.istft_launch(plan, X, hop, F, y, d_scratch=sc), args.reps, torch)
        Xt = X.transpose(-1, -2)
        t_ti = timed(lambda: torch.istft(Xt, n, hop, window=wd, center=True), args.reps, torch)
        lines.append(f"| inverse | {n} / {hop} | {rows} | {F} | {gb:.2f} | {t_i * 1e3:.3f} | {gb / t_i / 1e3:.2f} | {gb * 1e9 / t_i / ROOF:.2f} | "
                     f"{t_ti * 1e3:.3f} | {gb / t_ti / 1e3:.2f} | {t_ti / t_i:.2f}x |")
        print(lines[-2], lines[-1], sep="\n", flush=True)
        del x, X, y, sc
        torch.cuda.empty_cache()
    lines += ["", "torch.istft runs with center=True (a Hann window fails its envelope check uncentred); the span it returns is n samples",
              "shorter, which the byte count ignores.  The inverse includes its scratch traffic (the windowed frames are written once and",
              "read back once per covering sample) in its time but not in its bytes.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
