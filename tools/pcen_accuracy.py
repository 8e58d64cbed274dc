#!/usr/bin/env python3
"""The accuracy record of the per-channel energy normalisation (include/jsgx.h section 13), on the CPU:
  - E and L (jsgx::exp_any and jsgx::log_pos, the shipped routines, built from csrc/jsgx_internal.h by tools/pcen_accuracy.cpp) against exp
    and log in double over every float32 of their ranges, and the bits of E against section 1's routine over every float32 in [-87, 0];
  - the float32 restatement of the definition (tests/pcen_ref.py, which the GPU equals bit for bit: tests/test_gpu_pcen.py) against the
    float64 route through scipy.signal.lfilter and numpy powers, over planes at three scales with a silent stretch and three parameter sets:
    the relative error of S and |out32 - out64| / (out64 + bias^power), the worst over the seeds.
Writes profiles/pcen_accuracy.md.

    python tools/pcen_accuracy.py [--seeds N] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def errors(pr, np, M, params, state=None):
    """(worst relative error of S, worst |out32 - out64| / (out64 + bias^power)) of one plane; where the denominator is 0 (a silent frame
    without bias) both outputs have to be 0."""
    o32, S32, _ = pr.pcen32(M, state=state, **params)
    o64, S64, _ = pr.pcen64(M, state=state, **params)
    den = o64 + float(np.float32(params["bias"])) ** float(np.float32(params["power"]))
    assert (S64 > 0).all() and (o32[den == 0] == 0).all() and np.isfinite(o32).all()
    live = den > 0
    return float(np.max(np.abs(S32 - S64) / S64)), float(np.max(np.abs(o32[live] - o64[live]) / den[live]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcen_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import pcen_ref as pr
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pcen_accuracy")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-march=native", "-pthread", "-I", os.path.join(ROOT, "include"), "-I",
                               os.path.join(ROOT, "jadespectrogram_amd", "csrc"), os.path.join(ROOT, "tools", "pcen_accuracy.cpp"), "-o", exe])
        sweep = subprocess.run([exe], capture_output=True, text=True)
    assert sweep.returncode == 0, sweep.stdout + sweep.stderr
    T, B = 1000, 40
    lines = ["# Per-channel energy normalisation: accuracy (tools/pcen_accuracy.py)", "", "## The two routines, every float32 of their ranges", "", sweep.stdout.rstrip(), "",
             "## The definition in float32 against float64", "",
             f"tests/pcen_ref.py (the restatement the GPU equals bit for bit) against scipy.signal.lfilter and numpy powers in double, on planes of {T} frames x {B} bands "
             f"(squared noise times a band profile and a slow level, silent over frames {T // 2} to {T // 2 + T // 5 - 1}), {args.seeds} seeds each; eps = 1e-6 at every scale.  "
             "S: the largest |S32 - S64| / S64.  out: the largest |out32 - out64| / (out64 + bias^power).  A silent frame gave exactly +0 in every run.", "",
             "| scale | parameters | S, worst | S, seed to seed | out, worst | out, seed to seed |", "|---|---|---|---|---|---|"]
    worst_s = worst_o = 0.0
    for scale in pr.SCALES:
        for name, params in pr.PARAMS:
            e = [errors(pr, np, pr.plane(T, B, seed, scale), params) for seed in range(args.seeds)]
            s, o = [x[0] for x in e], [x[1] for x in e]
            worst_s, worst_o = max(worst_s, max(s)), max(worst_o, max(o))
            lines.append(f"| {scale:g} | {name}: " + ", ".join(f"{k} {v:.5g}" for k, v in params.items()) + f" | {max(s):.2e} | {min(s):.2e} .. {max(s):.2e} | {max(o):.2e} | "
                         f"{min(o):.2e} .. {max(o):.2e} |")
            print(lines[-1], flush=True)
    lines += ["", f"Worst over everything: S {worst_s:.2e}, out {worst_o:.2e}.  tests/test_pcen_ref.py asserts four times these (pcen_ref.S_BOUND, pcen_ref.OUT_BOUND): the error of "
              "a recurrence varies with the signal by about that much from seed to seed.", "",
              "The error of S is the recurrence's: about 1 / b frames of memory, one rounding of a, b M and the sum per frame, and a = fl(1 - b) itself, which is off the "
              "double 1 - b by up to 2^-25 and enters every frame of the memory.  The output's is that of two L and two E (within 1e-7 each, times the size of the "
              "logarithm they are applied to) and does not grow with the frames.", "", "Agreement with librosa.pcen itself: not measured (librosa is not installed here)."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + [""]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
