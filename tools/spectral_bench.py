#!/usr/bin/env python3
"""Throughput of the spectral shape kernel (jsg_spectral_shape_launch, include/jsg.h section 2l) on 8 x 4096 x 1025 (stays in the
caches), 16 x 16384 x 1025 (about 1 GB) and 64 x 16384 x 128 mel bands, with all seven outputs and with the centroid alone, each next
to the device's copy rate measured in the same process and next to a torch route that computes the same outputs on the same plane (sum,
matmul with f, cumsum with searchsorted, the mean of the logarithms, amax).  HIP events around each call, best (median) of 7 after 2
warm-up calls.  Writes profiles/spectral_bench.md.

    python tools/spectral_bench.py [--reps R] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def torch_all(torch, S, f, roll):
    K = S.shape[-1]
    E = S.sum(-1)
    c = torch.matmul(S, f) / E
    spread = torch.sqrt((((f - c[..., None]) ** 2) * S).sum(-1) / E)
    cum = S.cumsum(-1)
    k = torch.searchsorted(cum, roll * cum[..., -1:]).squeeze(-1).clamp_(max=K - 1)
    flat = (10.0 * torch.log10(S + 1e-11)).mean(-1) - 10.0 * torch.log10(E / K + 1e-11)
    crest = S.amax(-1) / (E / K)
    return E, c, spread, f[k], k, flat, crest


def torch_centroid(torch, S, f):
    return torch.matmul(S, f) / S.sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    props = torch.cuda.get_device_properties(0)
    lines = ["# Spectral shape throughput (tools/spectral_bench.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}, {props.multi_processor_count} compute units; best (median) of {args.reps} timed calls after 2 warm-up calls, HIP events.", ""]
    n = 1 << 28          # 1 GiB of float32 each way: past the last-level cache
    a, b = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    a.fill_(1.0)
    c_best, _ = timed(lambda: b.copy_(a), args.reps, torch)
    roof = 2.0 * 4 * n / c_best
    del a, b
    lines += [f"Copy roof of this device: a torch copy of 1 GiB, read plus written bytes over the best time: {roof / 1e12:.2f} TB/s ({c_best * 1e3:.3f} ms).", "",
              "bytes: the plane read once (the outputs, a few floats per frame, and the table are not counted).  torch, all outputs: sum, matmul with f, the",
              "weighted second moment, cumsum with searchsorted, the mean of log10, amax, on the same plane; centroid only: matmul and sum.  The torch",
              "routes state no order of summation and write whole-plane temporaries.", "",
              "| rows x frames x bins | outputs | path | lanes | frames in flight | MB read | ms | TB/s read | of the copy roof | torch ms | kernel / torch | largest relative difference of the centroid |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for R, T, K in ((8, 4096, 1025), (16, 16384, 1025), (64, 16384, 128)):
        S = torch.rand((R, T, K), device="cuda") ** 4
        f = torch.from_numpy(np.linspace(0.0, 11025.0, K).astype(np.float32)).cuda()
        outs = {name: torch.empty((R, T), dtype=torch.int32 if name == "rolloff_bin" else torch.float32, device="cuda")
                for name in ("energy", "centroid", "spread", "rolloff", "rolloff_bin", "flatness_db", "crest")}
        kw = {"d_" + k: v for k, v in outs.items()}
        path, lanes, frames, _ = jsg.spectral_shape_plan(S, f, **kw)
        nbytes = 4.0 * R * T * K
        for what, launch, route in (("all seven", lambda: jsg.spectral_shape_launch(S, f, **kw), lambda: torch_all(torch, S, f, 0.85)),
                                    ("centroid only", lambda: jsg.spectral_shape_launch(S, f, d_centroid=outs["centroid"]), lambda: torch_centroid(torch, S, f))):
            best, med = timed(launch, args.reps, torch)
            t_best, t_med = timed(route, args.reps, torch)
            launch()
            ref = torch_centroid(torch, S, f)
            diff = ((outs["centroid"] - ref).abs() / ref.abs()).max().item()
            lines.append(f"| {R} x {T} x {K} | {what} | {path} | {lanes} | {frames} | {nbytes / 1e6:.0f} | {best * 1e3:.3f} ({med * 1e3:.3f}) | {nbytes / best / 1e12:.2f} | "
                         f"{nbytes / best / roof:.0%} | {t_best * 1e3:.3f} ({t_med * 1e3:.3f}) | {best / t_best:.3f} | {diff:.2e} |")
            print(lines[-1], flush=True)
        del S, outs, kw
    lines += ["", "of the copy roof: bytes read per second over the copy's bytes read plus written per second.  The first plane (134 MB) stays in the last-level",
              "cache between the timed calls; the others (1075 MB, 537 MB) do not.  A `kernel / torch` below 1 is a row where this kernel is faster than the torch route.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
