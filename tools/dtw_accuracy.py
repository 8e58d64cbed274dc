#!/usr/bin/env python3
"""The error of the pairwise cost (include/jsgx.h section 2) against float64 and of the DTW total (section 3) against an independent
float64 DTW, from the numpy restatement tests/dtw_ref.py, next to the bounds the header derives.  CPU only.  Writes
profiles/dtw_accuracy.md.

    python tools/dtw_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_accuracy.md"))
    args = ap.parse_args()
    import dtw_ref as dr
    try:
        import scipy
        reference = f"scipy.spatial.distance.cdist {scipy.__version__} on the same inputs in float64"
    except ImportError:
        reference = "numpy in float64 on the same inputs"
    u = 2.0 ** -24
    lines = ["# Pairwise cost and DTW total against float64 (tools/dtw_accuracy.py)", "",
             "The device computes the cost and the recurrence with the float32 operations that include/jsgx.h states; tests/dtw_ref.py restates them in",
             "numpy and the GPU equals the restatement bit for bit (tests/test_gpu_dtw.py), so the figures below, computed on the CPU from the",
             f"restatement, are the device's.  Reference of the cost: {reference}.  Errors in units of u = 2^-24: relative for sqeuclidean and",
             "euclidean (bound (K + 3) u), absolute for cosine (bound (K + 5) u); 24 x 20 frames of standard normal features, their absolute values, and",
             "near-duplicates (Y a selection of X scaled by 1 + 2^-12).  tests/test_dtw_ref.py asserts the bounds on these cases.", "",
             "| metric | data | K | worst error / u | bound / u |", "|---|---|---|---|---|"]
    worst_of = {}
    for metric in dr.METRICS:
        for kind in ("normal", "positive", "near-duplicate"):
            for K in (1, 12, 128, 1024):
                worst, bound = dr.cost_errors(metric, kind, K)
                worst_of[metric] = max(worst_of.get(metric, (0.0, 0)), (worst, K))
                lines.append(f"| {metric} | {kind} | {K} | {worst:.2f} | {bound} |")
    lines += ["", "Worst found: " + "; ".join(f"{m} {w:.2f} u at K = {K} (bound {K + (5 if m == 'cosine' else 3)} u)" for m, (w, K) in worst_of.items()) + ".",
              "", "## The total", "",
              "Euclidean costs of 12 normal features, the restatement's total against a cell-by-cell float64 DTW of the same float32 costs; the bound is",
              "3 (N + M) u (non-negative costs and weights: min is monotone, every sum is of non-negative terms).", "",
              "| N x M | weights | subseq | relative error / u | bound / u |", "|---|---|---|---|---|"]
    for N, M in ((40, 40), (30, 77), (90, 25), (300, 300)):
        for seed, (wm, wa) in enumerate(((None, None), ((1, 1.5, 0.75), (0, 0.25, 0.5)))):
            for subseq in (False, True):
                X, Y = dr.cost_data("normal", N, M, 12, seed)
                C = dr.cost32(X, Y, "euclidean")
                _, total = dr.backtrace32(dr.dtw32(C, wm, wa, subseq), C, wm, wa, subseq)
                _, total64, _ = dr.dtw64(C, wm, wa, subseq)
                lines.append(f"| {N} x {M} | {'1, 1, 1 + 0' if wm is None else '1, 1.5, 0.75 + 0, 0.25, 0.5'} | {int(subseq)} | {abs(float(total) - total64) / total64 / u:.2f} | {3 * (N + M)} |")
    lines += ["", "Agreement with librosa.sequence.dtw was not measured (librosa is not installed where this ran); the definition differs from it as",
              "include/jsgx.h says (the three unit steps only, an integer band rule, stated tie and NaN rules, 1 for the cosine of a zero vector)."]
    with open(args.out, "w") as f:
        f.write("\n".join(lines + [""]))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
