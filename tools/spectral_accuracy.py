#!/usr/bin/env python3
"""Accuracy of the spectral shape kernel (jsg_spectral_shape_launch, include/jsg.h section 2l) on the planes of tests/spectral_ref.py
over every path of jsg_spectral_shape_plan: per case whether the GPU's bits equal the float32 restatement's, the worst observed fraction
of each stated bound (energy, centroid) for the GPU, and the spread's measured relative error against float64 on a narrow and on a broad
spectrum.  Writes profiles/spectral_accuracy.md.

    python tools/spectral_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import spectral_ref as sr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)

    def gpu(S, f, roll=0.85):
        out = jsg.spectral_shape(torch.from_numpy(np.array(S)).cuda(), freqs=np.array(f), roll_percent=roll)
        return {k: v.cpu().numpy() for k, v in out.items()}

    lines = ["# Spectral shape accuracy (tools/spectral_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Planes: tests/spectral_ref.py (3 rows x 64 frames: exponential values under a tilt, a row with a peak 40 dB",
             "above the rest, a row scaled by 1e-6), FFT bin frequencies of 22 050 Hz, roll_percent 0.85.  reference: the sums of include/jsg.h section 2l in float64 on the",
             "float32 inputs; the fractions are the worst |error| / (bound x |reference|) over the case's frames, the bounds (n + 1) u for the energy and (2n + 4) u for the",
             "centroid with n = ceil(K / W) + log2 W.", "",
             "| bins | path | elements differing in bits from the restatement (all outputs) | energy: fraction of the bound | centroid: fraction of the bound | rolloff bins differing from float64 |",
             "|---|---|---|---|---|---|"]
    for K in (1, 5, 33, 64, 128, 257, 513, 1025, 2049, 4097, 8193, 65536):
        T = 64 if K < 60000 else 4
        S, f = sr.planes(3, T, K), sr.freqs(K)
        got, want, w64, bound = gpu(S, f), sr.shape32(S, f), sr.shape64(S, f), sr.bounds(K)
        differ = sum(int((sr.raw(np.nan_to_num(got[n])) != sr.raw(np.nan_to_num(want[n]))).sum()) if n != "rolloff_bin" else int((got[n] != want[n]).sum()) for n in sr.OUTPUTS)
        frac = {}
        for n in ("energy", "centroid"):            # a reference of zero (silence, or f = 0 alone) must be met exactly
            err, den = np.abs(got[n].astype(np.float64) - w64[n]), bound[n] * np.abs(w64[n])
            frac[n] = float(np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err > 0, np.inf, 0.0)).max())
        lines.append(f"| {K} | {sr.plan(K)[0]} | {differ} of {7 * got['energy'].size} | {frac['energy']:.3f} | {frac['centroid']:.3f} | "
                     f"{int((got['rolloff_bin'] != w64['rolloff_bin']).sum())} of {got['rolloff_bin'].size} |")
        print(lines[-1], flush=True)
    lines += ["", "## The spread (no bound is stated)", "",
              "relative error of the GPU's spread against float64, worst and median over 64 frames of 1025 bins.  narrow: a Gaussian line 1.5 bins wide (standard",
              "deviation) at a centre that moves over the band, on a floor 120 dB below it, so d = f - centroid cancels where the energy is; broad: the planes above.", "",
              "| spectrum | worst relative error | median | in units of u = 2^-24 (worst) | bits equal to the restatement |", "|---|---|---|---|---|"]
    K, T = 1025, 64
    f = sr.freqs(K)
    k = np.arange(K)[None, :]
    centre = np.linspace(20.0, K - 20.0, T)[:, None]
    narrow = (np.exp(-0.5 * ((k - centre) / 1.5) ** 2) + 1e-12).astype(np.float32)
    for what, S in (("narrow", narrow[None]), ("broad", sr.planes(3, T, K))):
        got, want, w64 = gpu(S, f), sr.shape32(S, f), sr.shape64(S, f)
        rel = np.abs(got["spread"].astype(np.float64) - w64["spread"]) / w64["spread"]
        lines.append(f"| {what} | {rel.max():.3e} | {np.median(rel):.3e} | {rel.max() / sr.U:.1f} | {'yes' if sr.same_but_nan(got['spread'], want['spread']) else 'no'} |")
        print(lines[-1], flush=True)
    lines += ["", "Agreement with librosa was not measured (librosa is not installed here; the definitions differ as section 2l of include/jsg.h says).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
