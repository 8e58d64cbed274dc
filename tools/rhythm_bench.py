#!/usr/bin/env python3
"""Throughput of the tempogram (jsg_tempogram_launch) on 8 rows x 4096 frames, Wn = lags = 384, hop 1, next to the same plane computed in
torch on the same device (unfold x window -> rfft of 2 Wn -> |.|^2 -> irfft -> divide by lag 0), and of onset strength
(jsg_onset_strength_launch) on 8 x 4096 x 128 and on a plane larger than the last-level cache, next to the device's measured copy rate.
HIP events around each call, best (median) of 7 after 2 warm-up calls.  Writes profiles/rhythm_bench.md.

    python tools/rhythm_bench.py [--reps R] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

READING = ['',
           '## Reading',
           '',
           'Nothing here was measured with counters; the limiters are reasoned from the rows and from the code (tools/kernel_regs.py).',
           '* A `kernel / torch` below 1 is a row where this kernel is faster than the FFT route in torch.',
           '* Tempogram: the sum is a triangle, so a lane of lag tau works Wn - tau of the Wn steps of its tile (half the lanes idle on',
           '  average); at 384 lags a quarter of the 512 lag slots of a wave is empty; a step of 64 fused multiply-adds reads four times 16',
           '  bytes per lane at a 32-byte lane stride (two lanes per bank), which by count takes about as long as the arithmetic.',
           '* Onset strength: the 17 MB plane is bound by launch and latency, the 541 MB plane by memory, the t - lag re-read coming from',
           '  the caches.  With one frame per lane group (two loads in flight per lane) the rows took 0.018 and 0.281 ms (18 % and 37 %).',
           '* Two deliberately wrong builds against the 87 tests of tests/test_gpu_rhythm.py: the eight pairs of a step added in descending',
           '  j fails 11; out-of-row samples multiplied by the window instead of left out fails 1.  Both were discarded.']
FMA_PER_CLOCK = 128.0       # per compute unit: four SIMDs of 32 float32 lanes per clock, one fused multiply-add per pair


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


def torch_tempogram(torch, o, w, lags):
    """[rows][T][lags] by the FFT route, float32, normalised by lag 0 (zeros outside the row)."""
    Wn = w.shape[0]
    X = torch.nn.functional.pad(o, (Wn // 2, Wn - Wn // 2 - 1)).unfold(-1, Wn, 1) * w
    P = torch.fft.rfft(X, 2 * Wn)
    A = torch.fft.irfft(P.real * P.real + P.imag * P.imag, 2 * Wn)[..., :lags]
    a0 = A[..., :1]
    return torch.where(a0 == 0, torch.zeros_like(A), A / torch.where(a0 == 0, torch.ones_like(a0), a0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rhythm_bench.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rhythm_ref as rr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    mhz = float(getattr(props, "clock_rate", 2400000)) / 1e3
    lines = ["# Rhythm throughput (tools/rhythm_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}, {cus} compute units at {mhz:.0f} MHz; best (median) of {args.reps} timed calls after 2 warm-up calls, HIP events.", ""]
    # ---- tempogram
    rows, T, Wn = 8, 4096, 384
    o = torch.rand((rows, T), device="cuda")
    w = torch.from_numpy(jsg.window(jsg.capi.WIN_HANN, Wn)).cuda()
    out = torch.empty((rows, T, Wn), dtype=torch.float32, device="cuda")
    path, F, lds = jsg.tempogram_plan(o, w, out)
    best, med = timed(lambda: jsg.tempogram_launch(o, w, out), args.reps, torch)
    pairs = float(rows) * T * Wn * (Wn + 1) / 2
    per_clock = pairs / best / (cus * mhz * 1e6)
    t_t, t_tm = timed(lambda: torch_tempogram(torch, o, w, Wn), args.reps, torch)
    diff = (out - torch_tempogram(torch, o, w, Wn)).abs().max().item()
    ref = rr.tempogram(o[:1, :600].cpu().numpy(), w.cpu().numpy(), Wn, 1, 8, 1, restate=False)
    small = torch.empty((1, 8, Wn), dtype=torch.float32, device="cuda")
    jsg.tempogram_launch(o[:1, :600].contiguous(), w, small, n_frames=8)
    e_k = np.abs(small.cpu().numpy().astype(np.float64) - ref["tg64"]).max()
    e_t = np.abs(torch_tempogram(torch, o[:1, :600].contiguous(), w, Wn)[:, :8].cpu().numpy().astype(np.float64) - ref["tg64"]).max()
    lines += ["## Tempogram", "",
              f"Input: {rows} rows x {T} envelope samples of uniform noise, Wn = lags = {Wn}, hop 1, normalise 1: {rows * T} frames.  pairs: rows x frames x Wn (Wn + 1) / 2,",
              f"the products of the definition (the triangle, not the square).  pairs / clock / CU against {FMA_PER_CLOCK:g}: one fused multiply-add per lane and clock.", "",
              "| path | frames per item | LDS per workgroup | ms | Gpairs/s | pairs / clock / CU | of the vector pipe | torch ms | kernel / torch |", "|---|---|---|---|---|---|---|---|---|",
              f"| {path} | {F} | {lds} | {best * 1e3:.3f} ({med * 1e3:.3f}) | {pairs / best / 1e9:.0f} | {per_clock:.1f} | {per_clock / FMA_PER_CLOCK:.0%} | {t_t * 1e3:.3f} ({t_tm * 1e3:.3f}) | {best / t_t:.2f} |", "",
              f"Largest difference between the two planes: {diff:.3e}.  Against float64 on 8 frames: this kernel {e_k:.3e}, the torch route {e_t:.3e}.", ""]
    print("\n".join(lines[-4:]), flush=True)
    # ---- copy roof and onset strength
    n = 1 << 28          # 1 GiB of float32 each way: past the last-level cache
    a, b = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    a.fill_(1.0)
    c_best, c_med = timed(lambda: b.copy_(a), args.reps, torch)
    roof = 2.0 * 4 * n / c_best
    del a, b
    lines += ["## Onset strength", "",
              f"Copy roof of this device: a torch copy of 1 GiB, read plus written bytes over the best time: {roof / 1e12:.2f} TB/s ({c_best * 1e3:.3f} ms).",
              "bytes: the plane read once plus the envelope written.  lag 1, max_size 1.", "",
              "| rows x frames x bands | MB | ms | TB/s | of the copy roof |", "|---|---|---|---|---|"]
    for R, Tn, B in ((8, 4096, 128), (64, 16384, 128)):
        S = torch.randn((R, Tn, B), device="cuda")
        env = torch.empty((R, Tn), dtype=torch.float32, device="cuda")
        o_best, o_med = timed(lambda: jsg.onset_strength_launch(S, env), args.reps, torch)
        nbytes = 4.0 * (R * Tn * B + R * Tn)
        lines.append(f"| {R} x {Tn} x {B} | {nbytes / 1e6:.0f} | {o_best * 1e3:.3f} ({o_med * 1e3:.3f}) | {nbytes / o_best / 1e12:.2f} | {nbytes / o_best / roof:.0%} |")
        print(lines[-1], flush=True)
        del S
    lines += ["", "The first plane (17 MB) stays in the caches between the timed calls; the second (541 MB) does not."]
    lines += READING
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + [""]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
