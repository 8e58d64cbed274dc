#!/usr/bin/env python3
"""Time of the per-channel energy normalisation (jsgx_pcen_launch, libjsgx.so) on mel-like planes of 64 x 16384 x 128, 8 x 4096 x 128,
8 x 4096 x 40 and 16 x 16384 x 1025 (rows x frames x bands) of random data, with HIP events after warm-up calls: the whole launch, each of
its three kernels on its own (from torch's profiler, a run of its own), the bytes of its three plane passes (read twice, written once)
against the copy roof measured on the same device, and two torch routes on the same GPU: the same recurrence as a loop over the frames
(S[t] = a S[t-1] + b M[t], two kernels a frame) followed by the elementwise powers, and the elementwise half alone on a precomputed S.  The
results of the routes are compared (torch's pow is another routine: a relative difference, not bits).  Writes profiles/pcen_bench.md.

    python tools/pcen_bench.py [--reps R] [--out FILE] [--quick]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [(64, 16384, 128), (8, 4096, 128), (8, 4096, 40), (16, 16384, 1025)]          # rows, frames, bands
PARAMS = dict(gain=0.98, bias=2.0, power=0.5, eps=1e-6)
KERNELS = ("pcen_scan", "pcen_carry", "pcen_apply")


def timed(fn, reps, torch, warm=2):
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


def kernel_times(torch, fn, reps):
    """Median device time in seconds of each of the launch's kernels over `reps` calls, from torch's profiler; None where it reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        found = {k: [] for k in KERNELS}
        for e in prof.events():
            for k in KERNELS:
                if k + "_kernel" in e.name:
                    t = getattr(e, "device_time", None) or getattr(e, "cuda_time", 0)
                    if t:
                        found[k].append(t * 1e-6)
        if not all(found.values()):
            return None
        return {k: sorted(v)[len(v) // 2] for k, v in found.items()}
    except Exception as err:          # the profiler is an extra: the report says so
        print("profiler:", err, flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcen_bench.md"))
    ap.add_argument("--quick", action="store_true", help="the second and third workload only")
    args = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    assert torch.cuda.is_available(), "pcen_bench measures on the GPU; there is nothing to report without one"
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    cus = props.multi_processor_count
    b = jsg.pcen_coefficient(0.4, 22050, 512)
    a = 1.0 - b
    d_decay = torch.from_numpy(jsg.pcen_decay(b)).cuda()
    n = 1 << 28          # 1 GiB of float32 each way: past the last-level cache
    x, y = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    x.fill_(1.0)
    c_best, _ = timed(lambda: y.copy_(x), args.reps, torch)
    roof = 2.0 * 4 * n / c_best
    del x, y
    print(f"copy roof {roof / 1e12:.2f} TB/s", flush=True)
    rows = []
    for R, T, B in (WORKLOADS[1:3] if args.quick else WORKLOADS):
        gen = torch.Generator(device="cuda").manual_seed(T + B)
        M = torch.rand((R, T, B), generator=gen, dtype=torch.float32, device="cuda") ** 4
        out, S = torch.empty_like(M), torch.empty_like(M)
        scratch = torch.empty(max(1, jsg.pcen_scratch_bytes(M, d_decay, out, b=b, **PARAMS) // 4), dtype=torch.float32, device="cuda")
        ours = lambda: jsg.pcen_launch(M, d_decay, out, b=b, d_scratch=scratch, **PARAMS)
        best, med = timed(ours, args.reps, torch)
        parts = kernel_times(torch, ours, args.reps)
        jsg.pcen_launch(M, d_decay, out, b=b, d_smooth=S, d_scratch=scratch, **PARAMS)

        def powers(St):
            return (M * (PARAMS["eps"] + St) ** -PARAMS["gain"] + PARAMS["bias"]) ** PARAMS["power"] - PARAMS["bias"] ** PARAMS["power"]

        St = torch.empty_like(M)

        def loop():
            s = M[:, 0]
            for t in range(T):
                s = a * s + b * M[:, t]
                St[:, t] = s
            return powers(St)

        e_best, e_med = timed(lambda: powers(S), args.reps, torch)
        l_best, l_med = timed(loop, 2, torch, warm=1)
        want = loop()
        diff = float(((out - want).abs() / (want + PARAMS["bias"] ** PARAMS["power"])).amax())
        nbytes = 3.0 * 4 * R * T * B
        rows.append((R, T, B, best, med, parts, nbytes, l_best, e_best, diff))
        split = "not reported by the profiler" if parts is None else ", ".join(f"{k} {parts[k] * 1e3:.3f} ms" for k in KERNELS)
        print(f"{R} x {T} x {B}: {best * 1e3:.3f} ms (median {med * 1e3:.3f}), {nbytes / best / 1e12:.2f} TB/s = {nbytes / best / roof:.0%} of the copy roof; {split}; "
              f"torch loop {l_best * 1e3:.1f} ms ({l_best / best:.0f} x), torch powers alone {e_best * 1e3:.3f} ms ({e_best / best:.2f} x); difference {diff:.2e}", flush=True)
        del M, out, S, St, scratch, want
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Per-channel energy normalisation: time of a launch\n\n")
        f.write(f"`python tools/pcen_bench.py --reps {args.reps}` on {props.name} ({cus} compute units).  Random planes (uniform^4), librosa's default parameters "
                f"(b = {b:.5f}).  Best (median) of {args.reps} timed calls after 2 warm-up calls, HIP events.  Copy roof of this device: a torch copy of 1 GiB, read plus "
                f"written bytes over the best time: {roof / 1e12:.2f} TB/s.  bytes: three passes over the plane (read by the scan, read and written by the apply pass; the "
                "scratch is 1/256 of a plane).  The kernels' own times are medians of torch's profiler over the same number of calls, a run of its own.  torch loop: "
                "`s = a * s + b * M[:, t]; S[:, t] = s` over the frames, then the powers; torch powers: `(M * (eps + S) ** -gain + bias) ** power - bias ** power` "
                "on a precomputed S, which is the elementwise half alone.  The difference is the largest |out - torch| / (torch + bias^power).\n\n")
        f.write("| rows x frames x bands | MB a pass | ms | TB/s | of the copy roof | scan ms | carry ms | apply ms | torch loop ms | loop / this | torch powers ms | powers / this | difference |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for R, T, B, best, med, parts, nbytes, l, e, diff in rows:
            k = ["not reported"] * 3 if parts is None else [f"{parts[name] * 1e3:.3f}" for name in KERNELS]
            f.write(f"| {R} x {T} x {B} | {nbytes / 3e6:.0f} | {best * 1e3:.3f} ({med * 1e3:.3f}) | {nbytes / best / 1e12:.2f} | {nbytes / best / roof:.0%} | {k[0]} | {k[1]} | {k[2]} | "
                    f"{l * 1e3:.1f} | {l / best:.0f} | {e * 1e3:.3f} | {e / best:.2f} | {diff:.1e} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
