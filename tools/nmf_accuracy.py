#!/usr/bin/env python3
"""The float32 restatement of the factorisation (tests/nmf_ref.py, whose bits the GPU gives: tests/test_gpu_nmf.py) against scikit-learn's
float64 factors after 25 and 200 iterations, and the Frobenius loss per iteration of both.  CPU only.  Writes profiles/nmf_accuracy.md.

    python tools/nmf_accuracy.py [--out FILE]
"""
import argparse
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPE = (70, 33, 5)         # frames, bins, components: the shape of the 25-iteration GPU test
MARKS = (1, 2, 5, 10, 25, 50, 100, 200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import sklearn
    from sklearn.decomposition import non_negative_factorization
    import nmf_ref as nr
    V, A0, C0 = nr.problem(*SHAPE)
    V64 = np.array(V, np.float64)
    loss = lambda A, C: float(np.linalg.norm(V64 - np.asarray(A, np.float64) @ np.asarray(C, np.float64)))
    A, C = np.array(A0), np.array(C0)
    loss32, at = [], {}
    for it in range(1, MARKS[-1] + 1):
        A, C = nr.nmf32(V, A, C, 1)
        loss32.append(loss(A, C))
        if it in (25, 200):
            at[it] = (A.copy(), C.copy())
    loss64 = []
    nr.nmf64(V, A0, C0, MARKS[-1], losses=loss64)
    lines = ["# Non-negative matrix factorisation: float32 against scikit-learn's float64\n",
             f"`python tools/nmf_accuracy.py`: {SHAPE[0]} frames x {SHAPE[1]} bins, r = {SHAPE[2]}, the seeded plane (`random ** 4`) and start of `tests/nmf_ref.py`; "
             f"scikit-learn {sklearn.__version__}, `non_negative_factorization(init=\"custom\", solver=\"mu\", beta_loss=\"frobenius\", tol=0)`.  The float32 column is the "
             f"numpy restatement of include/jsgx.h section 12 (chunks of {nr.CHUNK_K} bins and {nr.CHUNK_T} frames), which the GPU equals bit for bit.  The float64 form of "
             "the definition equals scikit-learn exactly (tests/test_nmf_ref.py), so its losses below are scikit-learn's.  librosa is not installed: not measured.\n",
             "## The factors\n", "| iterations | activations: largest relative difference | components: largest relative difference |", "|---|---|---|"]
    for it in (25, 200):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            W, H, _ = non_negative_factorization(V64, W=np.array(A0, np.float64), H=np.array(C0, np.float64), n_components=SHAPE[2], init="custom", solver="mu",
                                                 beta_loss="frobenius", tol=0, max_iter=it)
        rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
        lines.append(f"| {it} | {rel(at[it][0], W):.2e} | {rel(at[it][1], H):.2e} |")
    lines += ["\nRelative to the largest entry of the factor.  The iteration is not contracting along every direction, so rounding differences of 1e-7 an update grow "
              "over the iterations; the losses do not show them.\n", "## The Frobenius loss ||V - A C||\n", "| iteration | float32 restatement | float64 (scikit-learn's form) |",
              "|---|---|---|"]
    lines += [f"| {it} | {loss32[it - 1]:.9f} | {loss64[it - 1]:.9f} |" for it in MARKS]
    rises32 = sum(b > a for a, b in zip(loss32, loss32[1:]))
    rises64 = sum(b > a for a, b in zip(loss64, loss64[1:]))
    lines.append(f"\nIterations at which the loss rose: {rises32} of {len(loss32) - 1} in float32, {rises64} in float64.  The test asserts only that the loss after 50 "
                 "iterations is below the loss after the first.")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
