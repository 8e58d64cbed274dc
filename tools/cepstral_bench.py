#!/usr/bin/env python3
"""Throughput of the projection (jsg_mfcc_launch) on 8 x 4096 x 128 -> 20, 64 x 16384 x 128 -> 20 and the square 64 x 16384 x 128 ->
128, and of delta (jsg_delta_launch) on 64 x 16384 x 20 with width 9, each next to the device's copy rate measured in the same process
and next to the same result from torch on the same device (matmul against the table; conv1d with the weights over the interior).  HIP
events around each call, best (median) of 7 after 2 warm-up calls.  Writes profiles/cepstral_bench.md.

    python tools/cepstral_bench.py [--reps R] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# Recorded text, not derived by a run: the register counts, the earlier steps and the wrong-build check below belong to the build that
# added the unit (tools/kernel_regs.py prints the current counts); a run of this tool renews the tables above them only.
READING = ['',
           '## Reading (recorded with the build that added csrc/jsg_cepstral.hip; a later run of the tool renews only the tables above)',
           '',
           'Nothing here was measured with counters; the limiters are reasoned from the rows and from the code object (tools/kernel_regs.py).',
           '* A `kernel / torch` below 1 is a row where this kernel is faster than torch; above 1, slower.  torch.matmul and conv1d run',
           '  through rocBLAS / MIOpen, which may use the matrix cores and state no order of summation; these kernels may not.',
           '* 128 -> 20 (mfcc_block5, 166 VGPRs, no scratch, 48 KB of LDS: three workgroups per compute unit).  By count the LDS array, not',
           '  the vector pipe, is what competes with memory: per tile of 64 frames the four waves issue 16 steps of 4 ds_read2_b32 and 10',
           '  ds_read_b128 at 4 cycles each (3.6 k cycles; the table reads are broadcasts, which cost their full width), the staging adds',
           '  about 1 k (the four 4-byte writes of a 16-byte piece meet a four-way bank conflict), the 20 x 128 v_fmac of a lane 2.6 k per',
           '  SIMD, and the 38 KB of the tile take about 4.3 k cycles per compute unit at the copy roof.  The three resident workgroups overlap',
           '  their phases only in part, hence about half the roof.  The 19 MB plane is bound by launch and latency (it stays in the caches).',
           '* 128 -> 128 (mfcc_block16, 294 VGPRs; the 64 KB table leaves one workgroup per compute unit: four waves, one per SIMD): 16 384',
           '  multiply-adds per frame against 1 KB of traffic; bound by the table reads from LDS (8 blocks x 32 steps x 16 ds_read_b128 per',
           '  tile, 16 k cycles) and their latency at one wave per SIMD, not by memory.  A dense square table is the matrix cores\' case.',
           '* Delta (34 VGPRs, 1 KB of LDS for the weights): lanes run along the coefficients and on across frames, every X is read once',
           '  from memory and eight more times from the caches (no staged tile); the nine dependent multiply-adds of an element wait for',
           '  their loads four at a time.',
           '* Steps on the way, same cases, ms (128 -> 20 large, 128 -> 128, delta): one register set per step, reads waited for in the',
           '  step: 0.247, 3.050, 0.096; two sets in turn: 0.260, 1.623, 0.106 (delta items of 1024 instead of 4096 elements: slower, undone);',
           '  and the next tile through registers one item ahead: 0.244, 1.382, 0.097.  These three asked for up to eight workgroups',
           '  per compute unit wherever the LDS allowed; the grid is now cut to what the registers hold as well (three for mfcc_block5),',
           '  which is the build of the tables above.',
           '* A deliberately wrong build against the 39 tests of tests/test_gpu_cepstral.py, discarded: the four multiply-adds of a step',
           '  taken in descending b fail 13 (the bit identities where B is a multiple of 4, the table-limit and path cases, the NaN',
           '  pattern, mfcc_audio, the captured chain; the round trips stay inside their bounds and pass); the interp window one frame',
           '  short at the right edge fails 13 (every delta bit identity, the NaN pattern under interp, the slope of a line, the captured',
           '  chain).  Both defects were in one build: 25 of 39 failed, the captured chain through either.']
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cepstral_bench.md"))
    args = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    mhz = float(getattr(props, "clock_rate", 2400000)) / 1e3
    lines = ["# Cepstral throughput (tools/cepstral_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}, {cus} compute units at {mhz:.0f} MHz; best (median) of {args.reps} timed calls after 2 warm-up calls, HIP events.", ""]
    n = 1 << 28          # 1 GiB of float32 each way: past the last-level cache
    a, b = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    a.fill_(1.0)
    c_best, c_med = timed(lambda: b.copy_(a), args.reps, torch)
    roof = 2.0 * 4 * n / c_best
    del a, b
    lines += [f"Copy roof of this device: a torch copy of 1 GiB, read plus written bytes over the best time: {roof / 1e12:.2f} TB/s ({c_best * 1e3:.3f} ms).", "",
              "## Projection", "",
              "bytes: the plane read once plus the coefficients written (the table is not counted).  fma / clock / CU against 128: one fused multiply-add per lane and clock.",
              "torch: `torch.matmul(S, table.T)` on the same plane.", "",
              "| rows x frames x bands -> coefficients | path | frames per item | LDS per workgroup | MB | ms | TB/s | of the copy roof | fma / clock / CU | of the vector pipe | torch ms | kernel / torch | largest difference |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for R, T, B, M in ((8, 4096, 128, 20), (64, 16384, 128, 20), (64, 16384, 128, 128)):
        S = -40.0 + 12.0 * torch.randn((R, T, B), device="cuda")
        D = torch.from_numpy(jsg.mfcc_table(B, M)).cuda()
        out = torch.empty((R, T, M), dtype=torch.float32, device="cuda")
        path, F, lds = jsg.mfcc_plan(S, D, out)
        best, med = timed(lambda: jsg.mfcc_launch(S, D, out), args.reps, torch)
        Dt = D.t().contiguous()
        t_best, t_med = timed(lambda: torch.matmul(S, Dt), args.reps, torch)
        diff = (out - torch.matmul(S, Dt)).abs().max().item()
        nbytes = 4.0 * R * T * (B + M)
        per_clock = float(R) * T * B * M / best / (cus * mhz * 1e6)
        lines.append(f"| {R} x {T} x {B} -> {M} | {path} | {F} | {lds} | {nbytes / 1e6:.0f} | {best * 1e3:.3f} ({med * 1e3:.3f}) | {nbytes / best / 1e12:.2f} | {nbytes / best / roof:.0%} | "
                     f"{per_clock:.1f} | {per_clock / FMA_PER_CLOCK:.0%} | {t_best * 1e3:.3f} ({t_med * 1e3:.3f}) | {best / t_best:.2f} | {diff:.3e} |")
        print(lines[-1], flush=True)
        del S, out
    lines += ["", "The first plane (19 MB) stays in the caches between the timed calls; the others (621 MB, 1074 MB) do not.", "",
              "## Delta", "",
              "bytes: the plane read once plus the plane written.  width 9, order 1, mode interp.  torch: `conv1d` of the [rows * coefficients][1][frames] transpose with the",
              "weights (the interior frames only; the transposes are not timed).", "",
              "| rows x frames x coefficients | MB | ms | TB/s | of the copy roof | torch ms | kernel / torch | largest difference (interior) |", "|---|---|---|---|---|---|---|---|"]
    R, T, M = 64, 16384, 20
    X = torch.randn((R, T, M), device="cuda")
    w = torch.from_numpy(jsg.delta_weights(9, 1)).cuda()
    out = torch.empty_like(X)
    best, med = timed(lambda: jsg.delta_launch(X, w, out), args.reps, torch)
    Xt = X.transpose(1, 2).reshape(R * M, 1, T).contiguous()
    kern = w.reshape(1, 1, 9)       # conv1d correlates: sum over j of w[j] x[t + j]
    t_best, t_med = timed(lambda: torch.nn.functional.conv1d(Xt, kern), args.reps, torch)
    inner = torch.nn.functional.conv1d(Xt, kern).reshape(R, M, T - 8).transpose(1, 2)
    diff = (out[:, 4:-4] - inner).abs().max().item()
    nbytes = 8.0 * R * T * M
    lines.append(f"| {R} x {T} x {M} | {nbytes / 1e6:.0f} | {best * 1e3:.3f} ({med * 1e3:.3f}) | {nbytes / best / 1e12:.2f} | {nbytes / best / roof:.0%} | {t_best * 1e3:.3f} ({t_med * 1e3:.3f}) | "
                 f"{best / t_best:.2f} | {diff:.3e} |")
    print(lines[-1], flush=True)
    lines += READING
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + [""]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
