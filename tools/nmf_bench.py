#!/usr/bin/env python3
"""Time per iteration of the non-negative matrix factorisation (jsgx_nmf_launch, libjsgx.so) on planes of 16384 x 1025 and 16384 x 128
at r = 8, 32, 64 and on 64 problems of 512 x 128, interleaved with a torch route on the same GPU: the same multiplicative updates as
matrix products, A *= (V @ C.T) / (A @ (C @ C.T)) and C *= (A.T @ V) / ((A.T @ A) @ C), with scikit-learn's zero-denominator rule.  Both
routes are captured into a graph of ITERS iterations and the replay is timed with HIP events: medians over the repetitions, the two routes
alternating.  Fused multiply-adds per second against the float32 matrix peak (64 FLOP a clock a SIMD, the vector peak as well) and the
bytes of V an iteration reads twice against the memory bandwidth.  The two routes' results are compared (the torch route sums in another
order: a relative difference, not bits).  Writes profiles/nmf_bench.md.

    python tools/nmf_bench.py [--reps R] [--iters N] [--out FILE] [--regs FILE] [--quick]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = [(1, 16384, 1025, r) for r in (8, 32, 64)] + [(1, 16384, 128, r) for r in (8, 32, 64)] + [(64, 512, 128, r) for r in (8, 32, 64)]   # P, T, K, r
CLOCK_HZ = 2.4e9            # the clock the peak figures are stated for
HBM_BYTES_PER_S = 8.0e12


def fma_per_iteration(P, T, K, r, update=True):
    """The multiply-adds the definition needs: N and G and D, then N2, G2 and D2."""
    a = T * K * r + r * r * K + T * r * r
    c = T * K * r + r * r * T + r * r * K
    return P * (a + (c if update else 0))


def timed_pair(torch, ours, theirs, reps):
    """Medians (ours, theirs) in seconds, the two alternating after two warm-up runs each."""
    times = ([], [])
    for k in range(reps + 2):
        for which, fn in enumerate((ours, theirs)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k >= 2:
                times[which].append(a.elapsed_time(b) * 1e-3)
    return tuple(sorted(t)[len(t) // 2] for t in times)


def captured(torch, fn):
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn(side.cuda_stream)                 # warm: code objects loaded, algorithms picked, before the capture
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            fn(side.cuda_stream)
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="iterations in one timed graph")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf_bench.md"))
    ap.add_argument("--regs", help="the output of tools/kernel_regs.py for jsgx_nmf.o, copied into the report")
    ap.add_argument("--quick", action="store_true", help="the first and the last workload only")
    args = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    from jadespectrogram_amd import capix
    assert torch.cuda.is_available(), "nmf_bench measures on the GPU; there is nothing to report without one"
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    peak_fma = cus * 4 * 32 * CLOCK_HZ       # 64 FLOP a clock a SIMD = 32 multiply-adds
    eps = capix.NMF_EPSILON
    rows = []
    for P, T, K, r in ([WORKLOADS[0], WORKLOADS[-1]] if args.quick else WORKLOADS):
        gen = torch.Generator(device="cuda").manual_seed(T + K + r)
        V = torch.rand((P, T, K), generator=gen, dtype=torch.float32, device="cuda") ** 4
        A0 = torch.rand((P, T, r), generator=gen, dtype=torch.float32, device="cuda") + 0.01
        C0 = torch.rand((P, r, K), generator=gen, dtype=torch.float32, device="cuda") + 0.01
        A, C, At, Ct = A0.clone(), C0.clone(), A0.clone(), C0.clone()
        scratch = torch.empty(jsg.nmf_scratch_bytes(V, A, C) // 4, dtype=torch.float32, device="cuda")

        def ours(stream):
            jsg.nmf_launch(V, A, C, n_iter=args.iters, d_scratch=scratch, stream=stream)

        def theirs(stream):
            for _ in range(args.iters):
                den = At @ (Ct @ Ct.transpose(-1, -2))
                At.mul_((V @ Ct.transpose(-1, -2)) / torch.where(den == 0, eps, den))
                den = (At.transpose(-1, -2) @ At) @ Ct
                Ct.mul_((At.transpose(-1, -2) @ V) / torch.where(den == 0, eps, den))

        # results first: both routes from the same start, ITERS iterations
        ours(None), theirs(None)
        torch.cuda.synchronize()
        diff = max(float(((A - At).abs().amax() / At.abs().amax())), float(((C - Ct).abs().amax() / Ct.abs().amax())))
        g_ours, g_theirs = captured(torch, ours), captured(torch, theirs)
        t_ours, t_theirs = timed_pair(torch, g_ours.replay, g_theirs.replay, args.reps)
        per_ours, per_theirs = t_ours / args.iters, t_theirs / args.iters
        fma = fma_per_iteration(P, T, K, r)
        v_bytes = 2 * 4 * P * T * K
        rows.append((P, T, K, r, per_ours, per_theirs, fma / per_ours, fma / per_ours / peak_fma, v_bytes / per_ours, diff))
        print(f"P {P} T {T} K {K} r {r}: {per_ours * 1e3:.3f} ms an iteration, torch {per_theirs * 1e3:.3f} ms ({per_theirs / per_ours:.2f} x), "
              f"{fma / per_ours / 1e12:.2f} T FMA/s ({100 * fma / per_ours / peak_fma:.1f} % of the matrix peak), V twice at {v_bytes / per_ours / 1e12:.2f} TB/s, "
              f"largest relative difference of the factors after {2 * args.iters + 2} iterations {diff:.2e}", flush=True)
        del V, A0, C0, A, C, At, Ct, scratch, g_ours, g_theirs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Non-negative matrix factorisation: time per iteration\n\n")
        f.write(f"`python tools/nmf_bench.py --reps {args.reps} --iters {args.iters}` on {props.name} ({cus} compute units).  Both routes are graphs of {args.iters} iterations, "
                f"replayed {args.reps} times after two warm-up replays, alternating; medians of HIP-event timings, divided by the iterations.  The torch route is "
                "`A *= (V @ C.T) / (A @ (C @ C.T))`, `C *= (A.T @ V) / ((A.T @ A) @ C)` with the zero-denominator rule.  Chunk lengths "
                f"{capix.NMF_CHUNK_K} (bins) and {capix.NMF_CHUNK_T} (frames).  FMA/s counts the multiply-adds of the definition (both Gram matrices and both small chains "
                f"included) against {peak_fma / 1e12:.1f} T FMA/s, the float32 matrix peak at {CLOCK_HZ / 1e9:.1f} GHz; the bandwidth column is two reads of V an iteration "
                f"over the time (HBM: {HBM_BYTES_PER_S / 1e12:.0f} TB/s; a plane of 67 MB fits the Infinity Cache).\n\n")
        f.write("| problems | frames | bins | r | this library, ms | torch, ms | torch / this | T FMA/s | % of matrix peak | V twice, TB/s | factors: largest relative difference |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for P, T, K, r, o, t, rate, share, bw, diff in rows:
            f.write(f"| {P} | {T} | {K} | {r} | {o * 1e3:.3f} | {t * 1e3:.3f} | {t / o:.2f} | {rate / 1e12:.2f} | {100 * share:.1f} | {bw / 1e12:.2f} | {diff:.1e} |\n")
        if args.regs and os.path.exists(args.regs):
            f.write("\n## The kernels' resources (tools/kernel_regs.py)\n\n```\n" + open(args.regs).read() + "```\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
