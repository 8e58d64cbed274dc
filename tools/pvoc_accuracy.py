#!/usr/bin/env python3
"""Accuracy of the phase vocoder kernels (jsg_pvoc_launch) against the float64 reference, next to the float32 numpy restatement of the
same arithmetic (tests/pvoc_ref.py defines the reference, the restatement, the bounds and the cases).  Writes
profiles/pvoc_accuracy.md: per case the restatement's worst relative error (the yardstick), the GPU's, their ratio (the GPU tests
allow pvoc_ref.YARDSTICKS) and the GPU's worst ratio to the per-frame cap.

    python tools/pvoc_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvoc_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import pvoc_ref as pr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    rows, worst_ratio, worst_cap = [], 0.0, 0.0
    for case in [c + ("noise",) for c in pr.accuracy_cases()] + pr.edge_cases():
        n, hop, rate, T, kind = case
        X = pr.edge_input(case)
        out = torch.empty((1, jsg.pvoc_frames(T, rate), n // 2 + 1), dtype=torch.complex64, device="cuda")
        jsg.phase_vocoder_launch(torch.from_numpy(np.array(X)).cuda(), rate, hop, n, out)
        torch.cuda.synchronize()
        f = pr.accuracy_figures(X, out[0].cpu().numpy(), rate, hop, n)
        ratio = f["worst"] / f["yardstick"]
        worst_ratio, worst_cap = max(worst_ratio, ratio), max(worst_cap, f["cap_ratio"])
        rows.append(f"| {kind} | {n} | {hop} | {rate:.10g} | {T} | {out.shape[1]} | {f['yardstick']:.3e} | {f['worst']:.3e} | {ratio:.2f} | {f['cap_ratio']:.4f} | "
                    f"{f['n_zero']} / {'yes' if f['zeros_exact'] else 'NO'} |")
        print(rows[-1], flush=True)
    lines = ["# Phase vocoder accuracy (tools/pvoc_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Reference R: the definition of include/jsg.h section 2e in float64 (tests/pvoc_ref.py).",
             "Error of an element: |Y - R| / max(|R|, 2^-100).  Yardstick: the worst error of the float32 numpy restatement of the library's",
             f"arithmetic on the same case.  The GPU tests require GPU worst <= {pr.YARDSTICKS:g} x yardstick (a) and, per output frame i, error <=",
             "2^-20 + (i+1) 3 2^-20 (b); the last column counts the elements with R = 0 and says whether the GPU wrote exact zeros there.", "",
             "Input: noise = the Hann-windowed STFT of seeded noise plus a tone with exact zeros (make_input); special = signed zeros, angles",
             "that are multiples of pi / 4 and moduli from 2^-91 to 2^126 (special_input).  First the cases of accuracy_cases(), then edge_cases().", "",
             "| input | n | hop | rate | T | T_out | yardstick | GPU worst | GPU / yardstick | worst error / cap (b) | zero elements / exact |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    lines += rows
    lines += ["", f"Worst GPU / yardstick over the cases: {worst_ratio:.2f} (allowed: {pr.YARDSTICKS:g}).  Worst error / cap (b): {worst_cap:.4f} (allowed: 1).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print(lines[-2])
    print("wrote", args.out)


if __name__ == "__main__":
    main()
