#!/usr/bin/env python3
"""Accuracy of the float32 routines of pYIN (include/jsgx.h section 5), on the CPU:

  - L (jsgx::log_pos, the shipped routine, built from csrc/jsgx_internal.h by tools/pyin_log_sweep.cpp) against log in double over every
    float32 in (0, 1]: the figure behind JSGX_LOG_ABS_BOUND;
  - the float32 restatement of the observation (tests/pyin_ref.py, which the GPU equals bit for bit) against the independent float64
    reading, on frames without bin collisions; and logp of the restated decoder against float64.

    python tools/pyin_accuracy.py [--threads N] [--out profiles/pyin_accuracy.md]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
U = 2.0 ** -24


def log_sweep(threads):
    exe = os.path.join(tempfile.gettempdir(), "pyin_log_sweep")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "include"), "-I",
                           os.path.join(ROOT, "jadespectrogram_amd", "csrc"), os.path.join(ROOT, "tools", "pyin_log_sweep.cpp"), "-o", exe])
    return subprocess.check_output([exe, str(threads)], text=True)


def observation():
    from scipy import stats
    import pyin_ref as pr
    rng = np.random.default_rng(11)
    sr, fmin, bps, P, N, lam, ntp, tau_min, tau_max = 22050.0, 65.40639132514966, 10, 601, 100, 2.0, 0.01, 10, 338
    prior = np.diff(stats.beta.cdf(np.linspace(0, 1, N + 1), 2, 18)).astype(np.float32)
    decay, norm = pr.boltzmann_tables(lam, pr.max_troughs(tau_min, tau_max))
    edges, _ = pr.bins_tables(sr, fmin, bps, P)
    frames, worst, worst_voiced = 0, 0.0, 0.0
    for _ in range(200):
        h = pr.frame_of(rng, tau_max, int(rng.integers(1, 6)), 1.2)
        emit, obs, voiced = pr.observe32(h, tau_min, tau_max, prior, decay, norm, edges, ntp)
        bins32 = [pr.bin_of(pr.period32(h, tau), edges, P) for tau in pr.troughs_of(h, tau_min, tau_max)]
        obs64, voiced64, bins64, _ = pr.observe64(h, tau_min, tau_max, N, (2, 18), lam, sr, fmin, bps, P, ntp)
        if len(set(bins32)) != len(bins32) or bins32 != bins64:
            continue
        frames += 1
        live = obs64 > 0
        worst = max(worst, float((np.abs(obs[live] - obs64[live]) / obs64[live]).max()))
        worst_voiced = max(worst_voiced, abs(float(voiced) - voiced64) / voiced64)
    return frames, worst / U, worst_voiced / U


def decoder():
    import pyin_ref as pr
    rows = []
    for P, W, T in ((5, 2, 50), (33, 8, 300), (601, 50, 64), (64, 128, 100), (601, 50, 1024)):
        inp = pr.decode_inputs("floats", T, P, W, P + T)
        logp = pr.decode32(*inp)[3]
        want = pr.decode64(*inp)
        rows.append((P, W, T, abs(float(logp) - want) / abs(want) / U, 4 * T + 2))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyin_accuracy.md"))
    args = ap.parse_args()
    sweep = log_sweep(args.threads)
    count = int(re.search(r"count (\d+)", sweep).group(1))
    scaled = re.search(r"worst_scaled (\S+) at (\S+) \((\S+)\)", sweep).groups()
    ulps = re.search(r"worst_ulps (\S+) at (\S+) \((\S+)\)", sweep).groups()
    hdr = open(os.path.join(ROOT, "include", "jsgx.h")).read()
    bound = float(re.search(r"#define JSGX_LOG_ABS_BOUND (\S+)", hdr).group(1))
    frames, worst, worst_voiced = observation()
    out = ["# pYIN: accuracy of the float32 routines", "", "`tools/pyin_accuracy.py`, on the CPU.  The GPU equals the float32 restatement bit for bit (tests/test_gpu_pyin.py), so these",
           "figures are the device's.", "", "## L, the logarithm of include/jsgx.h section 5b", "",
           f"Against `log` in double over every float32 in (0, 1], denormals included ({count} values; the shipped routine, `jsgx::log_pos`):", "",
           f"- the largest |L(x) - ln x| / max(1, |ln x|): **{float(scaled[0]):.3e}** at x = {scaled[2]} (bits {scaled[1]})",
           f"- the largest error in units of the last place of the result: {float(ulps[0]):.3f} ulp at x = {ulps[2]} (bits {ulps[1]})",
           f"- `JSGX_LOG_ABS_BOUND` = {bound:g}: {bound / float(scaled[0]):.2f} times the measured value (at most 1.5 is allowed)", "",
           "## The observation against float64", "",
           f"{frames} synthetic frames without bin collisions at librosa's defaults (P = 601, tau 10..338, N = 100, Beta(2, 18), lambda = 2): the float32",
           "restatement with the tables rounded once, against the independent float64 reading (scipy's beta and Boltzmann distributions).", "",
           f"- the largest relative error of obs[b]: {worst:.2f} u (u = 2^-24); the derived bound that tests/test_pyin_ref.py asserts is 18 u",
           f"- the largest relative error of voiced_prob: {worst_voiced:.2f} u; the derived bound is 34 u", "",
           "## logp of the decoder against float64", "", "| P | W | T | relative error, u | derived bound (4T + 2), u |", "|---|---|---|---|---|"]
    out += [f"| {P} | {W} | {T} | {e:.2f} | {b} |" for P, W, T, e, b in decoder()]
    open(args.out, "w").write("\n".join(out) + "\n")
    print("\n".join(out))
    assert float(scaled[0]) <= bound <= 1.5 * float(scaled[0])


if __name__ == "__main__":
    main()
