#!/usr/bin/env python3
"""Accuracy of YIN (jsg_yin_launch, include/jsg.h section 2i) on the cases of tests/yin_ref.py: the six shared signals (w 256, lags
8..200, hop 64) and a few shapes on noise and a tone.  Per case and row: the error of d' of the float32 numpy restatement and of the GPU
against the float64 evaluation in units of the per-element cap (2 w + tau + 12) 2^-24 d' (bound (b) allows 1), their ratio (bound (a)
of tests/test_gpu_yin.py allows YARDSTICKS), the f0 errors on decided frames and their ratio, the d' whose bits differ from the
restatement's, the decided frames and the kernel path.  Writes profiles/yin_accuracy.md.

    python tools/yin_accuracy.py [--out FILE]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 1, 1, 1), (63, 1, 65, 7), (65, 1, 200, 64), (256, 8, 200, 5000), (1000, 20, 1000, 64), (2048, 50, 2048, 300)]       # w, tau_min, tau_max, hop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yin_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import yin_ref as yr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    cases = [("shared signals: " + ", ".join(yr.NAMES), np.array(yr.signals()), yr.W, yr.TAU_MIN, yr.TAU_MAX, yr.HOP, yr.frames(yr.L, yr.W, yr.TAU_MAX, yr.HOP),
              yr.THRESHOLD, yr.SR, yr.shared())]
    for w, lo, hi, hop in SHAPES:
        T = 5 if hop < 5000 else 3
        n = (T - 1) * hop + w + hi
        rng = np.random.default_rng(w + hi)
        x = np.stack([rng.standard_normal(n), 0.5 * np.sin(2 * np.pi * np.arange(n) / 23.5)]).astype(np.float32)
        cases.append((f"noise, tone: w {w}, lags {lo}..{hi}", x, w, lo, hi, hop, T, 0.15, 4000.0, yr.evaluate(x, w, lo, hi, hop, T, 0.15, 4000.0)))
    rows, worst, worst_cap, total_diff, total = [], 0.0, 0.0, 0, 0

    def ratio_of(g, r):
        return float(np.max(np.where(r > 0, g / np.where(r > 0, r, 1.0), np.where(g > 0, np.inf, 0.0))))

    for name, x, w, lo, hi, hop, T, thr, sr, ref in cases:
        d_in = torch.from_numpy(x).cuda()
        R = x.shape[0]
        f0, aper = (torch.empty((R, T), dtype=torch.float32, device="cuda") for _ in range(2))
        cm = torch.empty((R, T, hi + 1), dtype=torch.float32, device="cuda")
        path = jsg.yin_kernel_name(d_in, w, lo, hi, hop, T, thr, sr, d_f0=f0, d_aper=aper, d_cmnd=cm)
        jsg.yin_launch(d_in, w, lo, hi, hop, T, thr, sr, d_f0=f0, d_aper=aper, d_cmnd=cm)
        torch.cuda.synchronize()
        cmn, f0n = cm.cpu().numpy(), f0.cpu().numpy()
        e_gpu, e_ref = yr.cap_units(cmn, ref), yr.cap_units(ref["dp32"], ref)
        ok = ref["decided"]
        f_gpu = np.array([np.abs(f0n[r][ok[r]].astype(np.float64) - ref["f064"][r][ok[r]]).max(initial=0.0) for r in range(R)])
        f_ref = np.array([np.abs(ref["f032"][r][ok[r]].astype(np.float64) - ref["f064"][r][ok[r]]).max(initial=0.0) for r in range(R)])
        ratio = max(ratio_of(e_gpu, e_ref), ratio_of(f_gpu, f_ref))
        diff = int((cmn.view(np.uint32) != np.ascontiguousarray(ref["dp32"]).view(np.uint32)).sum())
        worst, worst_cap, total_diff, total = max(worst, ratio), max(worst_cap, float(e_gpu.max())), total_diff + diff, total + cmn.size
        rows.append(f"| {name} | {hop} | {T} | {path} | {e_ref.max():.4f} | {e_gpu.max():.4f} | {f_ref.max():.2e} | {f_gpu.max():.2e} | {ratio:.3f} | {diff} of {cmn.size} | "
                    f"{int(ok.sum())} of {ok.size} |")
        print(rows[-1], flush=True)
    yard = math.ceil(1.25 * worst * 2.0) / 2.0
    lines = ["# YIN accuracy (tools/yin_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Signals: tests/yin_ref.py.  reference: the definition of include/jsg.h section 2i evaluated in",
             "float64.  restatement: the same in float32 in the library's stated orders, the fused multiply-add emulated exactly.  Columns 5 and 6: the",
             "worst |d' - reference| over the per-element cap (2 w + tau + 12) 2^-24 d' (bound (b): at most 1).  Columns 7 and 8: the worst |f0 - reference|",
             "in Hz over the decided frames.  Column 9: the worst row's GPU error over the restatement's, of d' and of f0 (bound (a)).  Column 10: d' whose",
             "bits differ from the restatement's.  Column 11: frames whose lag no change of d' within the cap can move.", "",
             "| case | hop | T | path | d' restatement / cap | d' GPU / cap | f0 restatement (Hz) | f0 GPU (Hz) | GPU / restatement | bits that differ | decided |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += rows
    lines += ["", f"Worst GPU / restatement ratio: {worst:.3f}.  YARDSTICKS = 1.25 x that, rounded up to the next half: {yard:g} (tests/yin_ref.py).",
              f"Worst GPU error over the cap: {worst_cap:.4f} (bound 1).  d' that differ from the restatement: {total_diff} of {total}.",
              "Agreement with librosa.yin was not measured (librosa is not installed here; its difference function comes from an FFT autocorrelation).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines[-4:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
