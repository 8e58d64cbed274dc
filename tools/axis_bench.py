#!/usr/bin/env python3
"""Display frequency axes: jsg_colormap_axis_launch against jsg_colormap_launch on the same dB ring (HIP events, median of repeated
launches).  Geometry of the C5 image: 4096 points, 1875 columns.  Bytes moved = the dB values the launch reads (the bins its row tiles
span) + the ARGB pixels it writes; the rate is stated against the MI355X's 8 TB/s.  Two timings per case: "warm" relaunches back to back
(ring and image, 10-30 MB, stay in the 256 MB Infinity Cache), "cold" writes a 1 GiB buffer before every launch, outside the timed
events, so that the launch reads its ring from HBM.

    python tools/axis_bench.py [--reps 200] [--md profiles/axis_bench.md]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, W, FS = 4096, 1875, 48000.0
CASES = [("identity (LINEAR 0-24 kHz)", 1, 2049, 0.0, 24000.0), ("LOG 20 Hz-20 kHz", 2, 1080, 20.0, 20000.0),
         ("LINEAR 0-4 kHz", 1, 1080, 0.0, 4000.0), ("MEL 0-24 kHz", 3, 256, 0.0, 24000.0)]


def median_us(torch, fn, reps, flush=None):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        if flush is not None:
            flush.zero_()                                                    # evicts ring and image from the Infinity Cache
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    H = N // 2 + 1
    rng = np.random.default_rng(0)
    d_db = torch.zeros((W, 2080), dtype=torch.float32, device="cuda")          # the engine's pitch: n/2+1 rounded up to 32 floats
    d_db[:, :H] = torch.from_numpy(rng.normal(-50.0, 20.0, (W, H)).astype(np.float32)).cuda()
    d_lut = torch.from_numpy(jsg.colormap_lut(256, jsg.capi.CM_JADE)).cuda()
    img_pitch = (W + 31) // 32 * 32
    base_img = torch.zeros((H, img_pitch), dtype=torch.int32, device="cuda")
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")          # 1 GiB

    def timed(fn):
        return median_us(torch, fn, args.reps), median_us(torch, fn, args.reps, flush)

    base_us, base_cold = timed(lambda: jsg.colormap(d_db, d_lut, -90.0, 10.0, d_argb=base_img[:, :W], height=H))
    base_bytes = W * H * 4 * 2
    rows = [{"case": "jsg_colormap_launch (bins)", "rows": H, "us": base_us, "cold_us": base_cold, "bytes": base_bytes}]
    for name, scale, h, lo, hi in CASES:
        ax = jsg.FreqAxis(N, FS, h, lo, hi, scale)
        first, count, _, _ = ax.rows()
        end = np.where(count > 0, first + count, first + 2)
        span = int(end.max() - first.min())
        img = torch.zeros((h, img_pitch), dtype=torch.int32, device="cuda")
        us, cold = timed(lambda: jsg.colormap_axis(d_db, d_lut, -90.0, 10.0, ax, d_argb=img[:, :W]))
        rows.append({"case": name, "rows": h, "us": us, "cold_us": cold, "bytes": W * span * 4 + W * h * 4, "bins_read": span})
    for r in rows:
        r["TBps"] = r["bytes"] / (r["us"] * 1e-6) / 1e12
        r["cold_TBps"] = r["bytes"] / (r["cold_us"] * 1e-6) / 1e12
        r["cold_of_8TBps"] = r["cold_TBps"] / 8.0
        r["vs_colormap"] = r["us"] / base_us
        r["cold_vs_colormap"] = r["cold_us"] / base_cold
        print(json.dumps(r))
    if args.md:
        with open(args.md, "w") as f:
            f.write(f"# Display frequency axes: jsg_colormap_axis_launch vs jsg_colormap_launch\n\n"
                    f"{N} points, {W} columns (C5 image width), 256 colours, ARGB only; HIP events, median of {args.reps} launches "
                    f"(tools/axis_bench.py).  Bytes = dB values read (the bins the row tiles span) + pixels written.  Warm: back-to-back "
                    f"launches, ring and image resident in the 256 MB Infinity Cache (a cache rate, not an HBM rate).  Cold: a 1 GiB buffer "
                    f"is written before every launch (outside the timed events), so the ring comes from HBM; only this column is "
                    f"compared with the 8 TB/s of HBM.\n\n"
                    "| case | rows | MB moved | warm us | warm TB/s | warm vs colormap | cold us | cold TB/s | cold of 8 TB/s | cold vs colormap |\n"
                    "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
            for r in rows:
                f.write(f"| {r['case']} | {r['rows']} | {r['bytes'] / 1e6:.2f} | {r['us']:.2f} | {r['TBps']:.2f} | {r['vs_colormap']:.2f} | "
                        f"{r['cold_us']:.2f} | {r['cold_TBps']:.2f} | {100 * r['cold_of_8TBps']:.0f} % | {r['cold_vs_colormap']:.2f} |\n")


if __name__ == "__main__":
    main()
