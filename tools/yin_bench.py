#!/usr/bin/env python3
"""YIN throughput (jsg_yin_launch) on 8 rows x 4096 frames at hop 512, sr 22 050, for (w, tau_max) = (1024, 1024) and (2048, 512), f0 and
aper as outputs.  Per case: time per call, sample pairs per second, pairs per clock and compute unit next to what the blocking allows,
and a torch route on the same device: the difference function from a torch.fft autocorrelation (r(0) + r_tau(0) - 2 r(tau)) plus
cumulative sums, up to d' (the selection is left out).  Also the worst error of d' of both routes against float64 on the 330 Hz onset
signal of tests/yin_ref.py.  HIP events around each call, best of 7.  Writes profiles/yin_bench.md.

    python tools/yin_bench.py [--reps R] [--out FILE] [--rows N] [--frames T]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = [(1024, 1024), (2048, 512)]
PAIRS_PER_CLOCK = 64.0       # per compute unit: four SIMDs of 32 float32 lanes per clock, a subtraction and a fused multiply-add per pair


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


def torch_cmnd(torch, x, w, tau_max, hop, T):
    """d' [rows][T][tau_max + 1] by the autocorrelation route, float32."""
    X = x.unfold(-1, w + tau_max, hop)[:, :T]                       # [rows][T][w + tau_max]
    n = 1
    while n < 2 * w + tau_max:
        n *= 2
    head = X[..., :w]
    r = torch.fft.irfft(torch.fft.rfft(X, n) * torch.fft.rfft(head, n).conj(), n)[..., :tau_max + 1]        # r(tau) = sum x[j] x[j + tau]
    sq = torch.nn.functional.pad(torch.cumsum(X * X, dim=-1), (1, 0))
    energy = sq[..., w:w + tau_max + 1] - sq[..., :tau_max + 1]                                             # r_tau(0) = sum x[j + tau]^2
    d = energy[..., :1] + energy - 2.0 * r
    d[..., 0] = 0.0
    S = torch.cumsum(d, dim=-1)
    tau = torch.arange(tau_max + 1, device=x.device, dtype=torch.float32)
    out = torch.where(S == 0, torch.ones_like(d), d * tau / torch.where(S == 0, torch.ones_like(S), S))
    out[..., 0] = 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yin_bench.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import yin_ref as yr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    mhz = float(getattr(props, "clock_rate", 2400000)) / 1e3
    rows, T, hop, sr = args.rows, args.frames, 512, 22050.0
    lines = ["# YIN throughput (tools/yin_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}, {cus} compute units at {mhz:.0f} MHz; best (median) of {args.reps} timed calls after 2 warm-up calls, HIP events.",
             f"Input: {rows} rows of float32 noise at sr {sr:g}, hop {hop}, {T} frames; outputs f0 and aper (d' stays on the chip).  pairs: rows x frames x w x tau_max.",
             f"pairs / clock / CU against {PAIRS_PER_CLOCK:g}: what 128 float32 lanes per clock and compute unit (four SIMDs of 32) allow at a subtraction and a fused multiply-add per pair.",
             "torch: d' from a torch.fft autocorrelation and cumulative sums, no selection (3 timed calls).", "",
             "| w | tau_max | path | frames per item | LDS per workgroup | ms | Gpairs/s | pairs / clock / CU | of the blocking's | torch ms | x torch |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for w, hi in CASES:
        L = (T - 1) * hop + w + hi
        x = torch.randn((rows, L), device="cuda")
        f0, aper = (torch.empty((rows, T), dtype=torch.float32, device="cuda") for _ in range(2))
        path, F, lds = jsg.yin_plan(x, w, 8, hi, hop, T, 0.1, sr, d_f0=f0, d_aper=aper)
        best, med = timed(lambda: jsg.yin_launch(x, w, 8, hi, hop, T, 0.1, sr, d_f0=f0, d_aper=aper), args.reps, torch)
        pairs = float(rows) * T * w * hi
        per_clock = pairs / best / (cus * mhz * 1e6)
        t_t, _ = timed(lambda: torch_cmnd(torch, x, w, hi, hop, T), 3, torch)
        lines.append(f"| {w} | {hi} | {path} | {F} | {lds} | {best * 1e3:.3f} ({med * 1e3:.3f}) | {pairs / best / 1e9:.0f} | {per_clock:.1f} | {per_clock / PAIRS_PER_CLOCK:.0%} | "
                     f"{t_t * 1e3:.2f} | {best / t_t:.2f} |")
        print(lines[-1], flush=True)
        del x
    # the reason for the direct form, as a number: d' of both routes on the onset signal against float64
    i = yr.NAMES.index("onset")
    ref = yr.shared()
    n_frames = yr.frames(yr.L, yr.W, yr.TAU_MAX, yr.HOP)
    xo = torch.from_numpy(np.array(yr.signals()[i:i + 1])).cuda()
    cm = torch.empty((1, n_frames, yr.TAU_MAX + 1), dtype=torch.float32, device="cuda")
    jsg.yin_launch(xo, yr.W, yr.TAU_MIN, yr.TAU_MAX, yr.HOP, n_frames, yr.THRESHOLD, yr.SR, d_cmnd=cm)
    torch.cuda.synchronize()
    want = ref["dp64"][i]
    e_kernel = np.abs(cm.cpu().numpy()[0].astype(np.float64) - want)
    e_torch = np.abs(torch_cmnd(torch, xo, yr.W, yr.TAU_MAX, yr.HOP, n_frames).cpu().numpy()[0].astype(np.float64) - want)
    voiced = ref["aper64"][i] < yr.THRESHOLD
    lag = ref["tau64"][i]
    at_dip = lambda e: max(float(e[t, lag[t]] / want[t, lag[t]]) for t in np.flatnonzero(voiced))
    lines += ["", "## d' of both routes on the 330 Hz onset signal (tests/yin_ref.py: sr 8000, w 256, lags 8..200, hop 64), against float64", "",
              "| route | worst absolute error of d' | worst relative error of d' at the chosen lag of a voiced frame |", "|---|---|---|",
              f"| this kernel | {e_kernel.max():.3e} | {at_dip(e_kernel):.3e} |", f"| torch.fft autocorrelation, float32 | {e_torch.max():.3e} | {at_dip(e_torch):.3e} |"]
    lines += ["", "## Reading", "",
              "Nothing here was measured with counters; the limiter is reasoned from the rows and from the code (tools/kernel_regs.py).",
              "* A row where `x torch` is above 1 is one where the FFT route in torch is faster than this kernel.",
              "* Per 64 pairs a lane issues 128 vector instructions and 12 two-dword LDS reads (23 dwords, 8 of them one address for the whole",
              "  wave): by count the vector pipe is the limiter, with the LDS at about three quarters of its rate beside it.",
              "* Sizing the items for 80 KiB of LDS per workgroup (two waves per SIMD, 11 and 16 frames per item) took 1.826 / 1.517 ms on the",
              "  two rows; sizing them for 40 KiB (four waves per SIMD, 4 frames per item) gave the rows above: the waves wait on the LDS reads",
              "  at the head of each step, and more of them hide it.",
              "* Broadcasting x[j] with v_readlane from registers (8 LDS reads per 64 steps instead of 8 per step) was slower on four waves",
              "  per SIMD, 1.917 / 1.760 ms, and was dropped: eight more instructions per step on the pipe that is the limiter."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + [""]))
    print("\n".join(lines[-12:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
