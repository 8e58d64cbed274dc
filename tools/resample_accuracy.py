#!/usr/bin/env python3
"""Accuracy of band-limited resampling (jsg_resample_launch, include/jsg.h section 2g) on the case list of tests/resample_ref.py: three
tables x eleven steps, three rows each (noise, a tone, one impulse).  Per case: the error of the float32 numpy restatement and of the
GPU against the float64 evaluation of the definition, both relative to the row's peak in units of 2^-24 (worst row), their ratio
(bound (a) of tests/test_gpu_resample.py allows YARDSTICKS), the GPU's error over the per-sample cap (bound (b) allows 1), the number
of outputs whose bits differ from the restatement's, and the kernel path.  Writes profiles/resample_accuracy.md.

    python tools/resample_accuracy.py [--out FILE]
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import resample_ref as rr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    U = 2.0 ** -24
    rows, worst_ratio, worst_cap, total_diff, total = [], 0.0, 0.0, 0, 0
    for name, step_name in rr.CASES:
        Z, P, win = rr.table(name)
        rs = jsg.Resampler.from_table(win, Z, P)
        L, step = rr.case_length(step_name), rr.STEPS[step_name]
        ref = rr.case(name, step_name)
        d_in = torch.from_numpy(np.array(rr.inputs(L))).cuda()
        d_out = torch.empty((3, ref["T"]), dtype=torch.float32, device="cuda")
        path = jsg.resample_kernel_name(rs, d_in, step, d_out)
        jsg.resample_launch(rs, d_in, step, d_out)
        torch.cuda.synchronize()
        y = d_out.cpu().numpy()
        e_gpu, e_ref = rr.peak_error(y, ref["y64"]), rr.peak_error(ref["y32"], ref["y64"])
        ratio = float(np.max(np.where(e_ref > 0, e_gpu / np.where(e_ref > 0, e_ref, 1.0), np.where(e_gpu > 0, np.inf, 0.0))))
        over = float((np.abs(y.astype(np.float64) - ref["y64"]) / np.maximum(ref["cap"], 1e-300)).max())
        diff = int((y.view(np.uint32) != ref["y32"].view(np.uint32)).sum())
        worst_ratio, worst_cap, total_diff, total = max(worst_ratio, ratio), max(worst_cap, over), total_diff + diff, total + y.size
        rows.append(f"| {name} | {step_name} | {L} | {ref['T']} | {path} | {e_ref.max() / U:.2f} | {e_gpu.max() / U:.2f} | {ratio:.3f} | {over:.3f} | {diff} of {y.size} |")
        print(rows[-1], flush=True)
        rs.close()
    yard = math.ceil(1.25 * worst_ratio * 2.0) / 2.0
    lines = ["# Band-limited resampling accuracy (tools/resample_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Inputs: three rows per case (seeded noise, a tone at 0.05 cycles per sample, one impulse;",
             "tests/resample_ref.py).  reference: the definition of include/jsg.h section 2g evaluated in float64.  restatement: the same in",
             "float32 with the library's order of summation, fmaf emulated as a float64 multiply-add rounded to float32.  Columns 6 and 7: the",
             "worst row's max |y - reference| relative to the row's peak, in units of 2^-24.  Column 8: the worst row's GPU error over the",
             "restatement's.  Column 9: the worst |y - reference| over the per-sample cap (N_i + 4) 2^-24 scale sum |w x|.  Column 10: outputs",
             "whose bits differ from the restatement's (not a requirement: the emulated fmaf may round twice).", "",
             "| table | step | L | T | path | restatement (2^-24) | GPU (2^-24) | GPU / restatement | GPU error / cap | bits that differ |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    lines += rows
    lines += ["", f"Worst GPU / restatement ratio: {worst_ratio:.3f}.  YARDSTICKS = 1.25 x that, rounded up to the next half: {yard:g} (tests/resample_ref.py).",
              f"Worst GPU error over the cap: {worst_cap:.3f} (bound 1).  Outputs that differ from the restatement: {total_diff} of {total}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines[-3:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
