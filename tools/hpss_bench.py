#!/usr/bin/env python3
"""Harmonic-percussive separation throughput (jsg_hpss_launch) at kernel size 31 / 31 on 1025 bins x 4096 frames x 8 rows of complex
frames, both outputs: time per call and bins/s, next to a jsg_calib_copy_launch that moves the same bytes, next to calls with a window
of 1 on either axis (what each median pass costs), and next to the same operation in torch ops on the same device (symmetric padding,
unfold, sort, gather, mask).  HIP events around each call.  Writes profiles/hpss_bench.md.

    python tools/hpss_bench.py [--reps R] [--out FILE] [--rows N] [--frames T] [--bins K]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def torch_hpss(X, W_t, W_f):
    """The definition of section 2f in torch ops on frame-major [rows][T][K]: power, symmetric padding, unfold, sort, gather, mask."""
    import torch
    P = X.real * X.real + X.imag * X.imag

    def median(P, W, dim):
        h = W // 2
        n = P.shape[dim]
        pad = torch.cat([P.narrow(dim, 0, h).flip(dim), P, P.narrow(dim, n - h, h).flip(dim)], dim=dim) if h else P
        return pad.unfold(dim, W, 1).sort(dim=-1).values[..., h]

    H, Cm = median(P, W_t, 1), median(P, W_f, 2)
    D = H + Cm
    zero = torch.zeros_like(D)
    M_h, M_p = torch.where(D > 0, H / D, zero), torch.where(D > 0, Cm / D, zero)
    return M_h, M_p, M_h[..., None] * torch.view_as_real(X), M_p[..., None] * torch.view_as_real(X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--bins", type=int, default=1025)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpss_bench.md"))
    args = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    lib = jsg.capi.lib()
    torch.cuda.set_device(0)
    rows, T, K = args.rows, args.frames, args.bins
    bins = rows * T * K
    X = torch.view_as_complex(torch.randn((rows, T, K, 2), device="cuda"))
    oh, op = (torch.empty((rows, T, K), dtype=torch.complex64, device="cuda") for _ in range(2))
    sc = torch.empty(jsg.hpss_scratch_bytes(X, d_harm=oh, d_perc=op) // 4 + 4, dtype=torch.float32, device="cuda")
    nbytes = 24 * bins          # the input read once (8 bytes per bin), two outputs written once: the algorithmic bytes
    lines = ["# Harmonic-percussive separation throughput (tools/hpss_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}; best (median) of {args.reps} timed calls after 2 warm-up calls, HIP events.",
             f"Input: {rows} rows x {T} frames x {K} bins of complex64 noise, out_h and out_p requested, no masks.  Algorithmic bytes: 24 per",
             "bin (input read once, two outputs written once); the library also writes and reads 4 bytes per bin of scratch (the frequency",
             "medians) and re-reads input frames from cache (the halo of the frequency pass, the frame that leaves the time window, the centre).", "",
             "| call | ms | Gbins/s | algorithmic TB/s |", "|---|---|---|---|"]
    t_full = None
    for name, W in (("jsg hpss 31 / 31", (31, 31)), ("jsg hpss W_t 31, W_f 1", (31, 1)), ("jsg hpss W_t 1, W_f 31", (1, 31)),
                    ("jsg hpss 1 / 1", (1, 1)), ("jsg hpss 63 / 63", (63, 63)), ("jsg hpss 17 / 17", (17, 17))):
        best, med = timed(lambda: jsg.hpss_launch(X, d_harm=oh, d_perc=op, kernel_size=W, d_scratch=sc), args.reps, torch)
        t_full = t_full or best
        lines.append(f"| {name} | {best * 1e3:.3f} ({med * 1e3:.3f}) | {bins / best / 1e9:.2f} | {nbytes / best / 1e12:.2f} |")
        print(lines[-1], flush=True)
    half = nbytes // 2 // 16 * 16
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    t_c, t_c_med = timed(lambda: jsg.capi.check(lib.jsg_calib_copy_launch(src.data_ptr(), dst.data_ptr(), half, C.c_void_p(stream))), args.reps, torch)
    del src, dst
    lines.append(f"| jsg_calib_copy_launch, the same bytes | {t_c * 1e3:.3f} ({t_c_med * 1e3:.3f}) | {bins / t_c / 1e9:.2f} | {2 * half / t_c / 1e12:.2f} |")
    print(lines[-1], flush=True)
    t_t, t_t_med = timed(lambda: torch_hpss(X, 31, 31), 3, torch)
    lines.append(f"| torch ops 31 / 31 (unfold, sort, gather, mask) | {t_t * 1e3:.2f} ({t_t_med * 1e3:.2f}) | {bins / t_t / 1e9:.3f} | {nbytes / t_t / 1e12:.3f} |")
    print(lines[-1], flush=True)
    # the two routes agree on the selection: count the mask elements whose bits differ (the division and the order of rounding may)
    mh, mp = (torch.empty((rows, T, K), dtype=torch.float32, device="cuda") for _ in range(2))
    jsg.hpss_launch(X, d_mask_h=mh, d_mask_p=mp, d_scratch=sc)
    t_mh, t_mp = torch_hpss(X, 31, 31)[:2]
    differ = int((mh.view(torch.int32) != t_mh.view(torch.int32)).sum() + (mp.view(torch.int32) != t_mp.view(torch.int32)).sum())
    lines += ["", f"jsg 31 / 31 is {t_c and t_full / t_c:.2f} x the copy's time and {t_t / t_full:.1f} x faster than the torch route.  Mask elements whose bits differ",
              f"between the two routes at this size: {differ} of {2 * bins}.", ""]
    print("\n".join(lines[-3:]))
    lines += ['## Reading',
              '',
              'Nothing here was measured with counters; the limiters below are read from the differences between the rows and from the resource',
              'use of the kernels (tools/kernel_regs.py).',
              '* 1 / 1 is the cost of the structure with no selection work: the frequency pass stages 64 frames x (64 + halo) bins through LDS and',
              '  writes the scratch plane, the time pass walks a chunk frame by frame.  The time pass waits for one memory round trip per step (the',
              '  loads of the next step are requested a step ahead, the centre loads in the step that uses them) with about 4200 one-wave items on',
              '  256 compute units; the frequency pass holds 6 one-wave workgroups per compute unit (24.7 KB of LDS each at W_f = 31).  Both are',
              '  bound by latency at low occupancy, not by HBM: the copy moves the same bytes in a quarter of the time.',
              '* W_t 31 over 1 / 1 is what the time median adds, W_f 31 over 1 / 1 what the frequency median adds.  The frequency median is the',
              '  larger part: its window work (about 6 x 31 vector operations a step in registers, 94 steps for 64 outputs) runs at 1.5 waves per',
              '  SIMD, so its dependent compare / min / max chains are exposed.  Limiter: vector issue latency at low occupancy.',
              '* 17 / 17 and 63 / 63 take the window in LDS ([W][64], 2 W reads and 2 W writes per step).  Limiter: the latency of dependent LDS',
              "  passes; at 63 the frequency pass holds 48.6 KB per workgroup (3 per compute unit) and does twice the steps' work, hence the jump.",
              '']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
