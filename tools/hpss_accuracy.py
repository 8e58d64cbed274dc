#!/usr/bin/env python3
"""Accuracy of harmonic-percussive separation (jsg_hpss_launch, include/jsg.h section 2f).  Per geometry: the float32 numpy restatement
(tests/hpss_ref.py, `mirror`) against librosa's definition evaluated in float64 on magnitudes, in units of u = 2^-24, and the GPU
against the restatement, as the number of elements whose bits differ over the two masks and the two outputs (the GPU tests require
0).  Then the round trip of hpss_audio at margins 1.  Writes profiles/hpss_accuracy.md.

    python tools/hpss_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MARGINS = [(1.0, 1.0), (2.0, 1.0), (1.0, 3.5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpss_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import hpss_ref as hr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    rows, worst_u, total_diff = [], 0.0, 0
    for T, K, W_t, W_f in hr.GEOMETRIES + [(1000, 1025, 31, 31)]:
        for m in MARGINS:
            X = hr.make_input(T, K)
            want = hr.mirror(X, W_t, W_f, *m)
            R_h, R_p = hr.reference64(X, W_t, W_f, *m)
            e = max(np.abs(want[0].astype(np.float64) - R_h).max(), np.abs(want[1].astype(np.float64) - R_p).max()) / hr.U
            d_X = torch.from_numpy(np.array(X)).cuda()
            mh, mp = (torch.empty(d_X.shape, dtype=torch.float32, device="cuda") for _ in range(2))
            oh, op = (torch.empty(d_X.shape, dtype=torch.complex64, device="cuda") for _ in range(2))
            jsg.hpss_launch(d_X, d_harm=oh, d_perc=op, d_mask_h=mh, d_mask_p=mp, kernel_size=(W_t, W_f), margin=m)
            torch.cuda.synchronize()
            diff = sum(int((np.ascontiguousarray(g.cpu().numpy()).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum())
                       for g, w in zip((mh, mp, oh, op), want))
            worst_u, total_diff = max(worst_u, e), total_diff + diff
            rows.append(f"| {T} | {K} | {W_t} | {W_f} | {m[0]:g}, {m[1]:g} | {e:.3f} | {diff} of {6 * T * K} |")
            print(rows[-1], flush=True)
    # the round trip of tests/test_gpu_hpss.py
    rng = np.random.default_rng(5)
    L, n_fft, hop = 16000, 1024, 256
    s = np.arange(L)
    x = torch.from_numpy((0.2 * rng.standard_normal(L) + np.sin(2 * np.pi * 0.031 * s) + 2.0 * (s % 1500 == 700)).astype(np.float32)).cuda()
    y_h, y_p = jsg.hpss_audio(x, n_fft, hop)
    y_id = jsg.istft(jsg.stft(x, n_fft, hop, None, jsg.capi.WIN_HANN), n_fft, hop, None, jsg.capi.WIN_HANN, length=L)
    span = slice(n_fft, L - n_fft)
    e = float((y_h.double() + y_p.double() - y_id.double())[span].abs().max())
    e_id = float((y_id.double() - x.double())[span].abs().max())
    lines = ["# Harmonic-percussive separation accuracy (tools/hpss_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Input: complex normal values times 10^U(-6, 3), seeded (tests/hpss_ref.py make_input).",
             "mirror: the float32 numpy restatement of include/jsg.h section 2f.  reference: librosa.decompose.hpss(|X|, power=2, mask=True) on",
             "float64 magnitudes.  Column 6: the worst |mirror mask - reference mask| over both masks in units of u = 2^-24 (the CPU tests allow",
             "4).  Column 7: elements of the GPU's two masks and two complex outputs (6 float32 per bin) whose bits differ from the mirror's (the",
             "GPU tests require 0).", "",
             "| T | K | W_t | W_f | margins h, p | mirror vs float64 (u) | GPU bits that differ |", "|---|---|---|---|---|---|---|"]
    lines += rows
    lines += ["", f"Worst mirror error: {worst_u:.3f} u.  Elements that differ between GPU and mirror over all cases: {total_diff}.", "",
              "## Round trip", "",
              f"hpss_audio at margins 1, n_fft {n_fft}, hop {hop}, Hann, {L} samples of noise + a tone + clicks, over samples {n_fft}..{L - n_fft}:",
              f"e = max |y_h + y_p - y_id| = {e:.3e}, e_id = max |y_id - x| = {e_id:.3e} (y_id = istft(stft(x))), e / e_id = {e / e_id:.3f}"
              " (the GPU test requires <= 4).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines[-7:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
