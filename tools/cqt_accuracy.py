#!/usr/bin/env python3
"""Accuracy of the constant-Q spectrogram (jsg_cqt_launch, include/jsg.h section 2h) on the cases of tests/cqt_ref.py: the synthetic basis
(half lengths 0 .. 1000) at five hops on three rows (noise, a tone, one impulse), the 24-bin standard basis with and without the scale on
noise and a tone, and one bin of 80 001 taps (the tap-pass path).  Per case: the error of the float32 numpy restatement and of the GPU
against the float64 evaluation of the definition, both relative to the row's peak in units of 2^-24 (worst row), their ratio (bound (a)
of tests/test_gpu_cqt.py allows YARDSTICKS), the GPU's error over the per-element cap (bound (b) allows 1), the number of components whose
bits differ from the restatement's, and the kernel path.  Writes profiles/cqt_accuracy.md.

    python tools/cqt_accuracy.py [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cqt_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import cqt_ref as cr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    U = 2.0 ** -24
    cases = []
    half, taps = cr.synthetic_basis()
    for hop in cr.HOPS:
        cases.append((f"synthetic, h = {', '.join(map(str, cr.SYNTH_HALF))}", half, taps, np.array(cr.inputs(cr.L)), hop, cr.frames(cr.L, hop), cr.case(hop)))
    for scale in (True, False):
        h, _, _, _, t = cr.standard_basis(scale)
        cases.append((f"standard, 24 bins from C1{'' if scale else ', no scale'}", h, t, np.array(cr.standard_inputs()), cr.STANDARD_HOP,
                      cr.frames(cr.STANDARD_L, cr.STANDARD_HOP), cr.standard_case(scale)))
    h, t = cr.synthetic_basis((40000,), 5)
    x = np.random.default_rng(5).standard_normal((2, 100001)).astype(np.float32)
    cases.append(("one bin, h = 40000", h, t, x, 3000, cr.frames(100001, 3000), cr.evaluate(x, h, t, 3000, cr.frames(100001, 3000))))
    rows, worst_ratio, worst_cap, total_diff, total = [], 0.0, 0.0, 0, 0
    for name, h, t, x, hop, T, ref in cases:
        b = jsg.CqtBasis.from_tables(h, t)
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.empty((x.shape[0], T, b.n_bins), dtype=torch.complex64, device="cuda")
        path = jsg.cqt_kernel_name(b, d_in, hop, T, d_out)
        jsg.cqt_launch(b, d_in, hop, T, d_out)
        torch.cuda.synchronize()
        C = d_out.cpu().numpy()
        e_gpu, e_ref = cr.peak_error(C, ref["C64"]), cr.peak_error(ref["C32"], ref["C64"])
        ratio = float(np.max(np.where(e_ref > 0, e_gpu / np.where(e_ref > 0, e_ref, 1.0), np.where(e_gpu > 0, np.inf, 0.0))))
        d = C.astype(np.complex128) - ref["C64"]
        over = max(float((np.abs(d.real) / np.maximum(ref["cap_re"], 1e-300)).max()), float((np.abs(d.imag) / np.maximum(ref["cap_im"], 1e-300)).max()))
        diff = int((C.view(np.uint32) != np.ascontiguousarray(ref["C32"]).view(np.uint32)).sum())
        worst_ratio, worst_cap, total_diff, total = max(worst_ratio, ratio), max(worst_cap, over), total_diff + diff, total + 2 * C.size
        rows.append(f"| {name} | {x.shape[1]} | {hop} | {T} | {path} | {e_ref.max() / U:.2f} | {e_gpu.max() / U:.2f} | {ratio:.3f} | {over:.3f} | {diff} of {2 * C.size} |")
        print(rows[-1], flush=True)
        b.close()
    yard = math.ceil(1.25 * worst_ratio * 2.0) / 2.0
    lines = ["# Constant-Q spectrogram accuracy (tools/cqt_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Inputs and bases: tests/cqt_ref.py.  reference: the definition of include/jsg.h section 2h",
             "evaluated in float64 on the float32 taps.  restatement: the same in float32 with the library's order of summation, fmaf emulated as",
             "a float64 multiply-add rounded to float32.  Columns 6 and 7: the worst row's max |C - reference| (the larger component) relative to",
             "the row's peak, in units of 2^-24.  Column 8: the worst row's GPU error over the restatement's.  Column 9: the worst",
             "|C - reference| over the per-element cap (N_live + 4) 2^-24 sum |c x| per component.  Column 10: components whose bits differ from",
             "the restatement's (not a requirement: the emulated fmaf may round twice).", "",
             "| basis | L | hop | T | path | restatement (2^-24) | GPU (2^-24) | GPU / restatement | GPU error / cap | bits that differ |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    lines += rows
    lines += ["", f"Worst GPU / restatement ratio: {worst_ratio:.3f}.  YARDSTICKS = 1.25 x that, rounded up to the next half: {yard:g} (tests/cqt_ref.py).",
              f"Worst GPU error over the cap: {worst_cap:.3f} (bound 1).  Components that differ from the restatement: {total_diff} of {total}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines[-3:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
