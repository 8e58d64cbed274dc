#!/usr/bin/env python3
"""The error of jsgx_exp (include/jsgx.h, the smoothing weights of the beat tracker) against exp in double over every (P, k) with
P <= 1024, from the numpy restatement tests/beat_ref.py.  CPU only.  Writes profiles/beat_accuracy.md.

    python tools/beat_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beat_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import beat_ref as br
    worst, count, below, n_below = br.exp_accuracy()
    per = []
    for P in (1, 4, 47, 100, 511, 1024):
        x = br.gauss_arg(P)
        inside = x >= np.float32(-87.0)
        g, want = br.exp32(x).astype(np.float64), np.exp(x.astype(np.float64))
        per.append((P, int(inside.sum()), float(np.max(np.abs(g[inside] - want[inside]) / want[inside]))))
    lines = ["# Beat tracker: the exp routine of the smoothing weights (tools/beat_accuracy.py)", "",
             "g[k] = jsgx_exp(-0.5f * (32 k / P)^2), k = 0..P, is evaluated on the device by the float32 routine that include/jsgx.h states operation by",
             "operation (range reduction by ln 2 in two parts, a degree-7 polynomial in Horner form with fmaf, the power of two through the exponent bits).",
             "tests/beat_ref.py restates it in numpy; the GPU's local score equals the restatement's bit for bit (tests/test_gpu_beat.py), so the figures",
             "below, computed on the CPU from the restatement, are the device's.  Reference: numpy's exp in float64 of the same float32 argument.", "",
             f"* Every (P, k) with 1 <= P <= 1024, 0 <= k <= P: {count + n_below} points.",
             f"* {count} points have an argument >= -87: the worst relative error is **{worst:.3e}** ({worst / 2.0 ** -24:.2f} units of 2^-24).",
             f"  include/jsgx.h states JSGX_EXP_REL_BOUND = {br.EXP_REL_BOUND:.1e}, which tests/test_beat_ref.py asserts.",
             f"* {n_below} points have an argument below -87: the routine returns +0 there; the largest exp among them is {below:.3e} (the absolute error).",
             "", "| P | points with x >= -87 | worst relative error |", "|---|---|---|"]
    lines += [f"| {P} | {n} | {e:.3e} |" for P, n, e in per]
    lines += ["", "Agreement of the beat positions with librosa.beat.beat_track was not measured; the",
              "definition differs from it on purpose (an integer period, Ellis' end rule, no trimming; include/jsgx.h)."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines + [""]))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
