#!/usr/bin/env python3
"""Accuracy of the tempogram (jsg_tempogram_launch, include/jsg.h section 2j) on the cases of tests/rhythm_ref.py and on the window
sizes where the kernel changes its path: per case and normalise value the worst error of the GPU and of the float32 restatement
against the float64 evaluation in units of cap (b), their ratio (what bound (a) of tests/test_gpu_rhythm.py allows YARDSTICKS), the
elements whose bits differ from the restatement's, and the kernel path.  Also the bits of onset strength and tempo against their
restatements.  Writes profiles/rhythm_accuracy.md.

    python tools/rhythm_accuracy.py [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rhythm_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import rhythm_ref as rr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    raw = lambda a: np.ascontiguousarray(a).view(np.uint32)
    rng = np.random.default_rng(11)
    signed = rng.standard_normal((2, 1200)).astype(np.float32)
    cases = [("shared envelopes", rr.envelopes(), 64, 64, 1, 600), ("shared envelopes", rr.envelopes(), 384, 384, 1, 28), ("shared envelopes", rr.envelopes(), 100, 100, 7, 86),
             ("shared envelopes", rr.envelopes(), 300, 200, 3, 60), ("signed noise", signed, 384, 384, 50, 24), ("signed noise", signed, 65, 65, 1, 400),
             ("signed noise", signed, 4096, 4096, 600, 2), ("signed noise", signed, 2, 2, 1, 1200)]
    lines = ["# Rhythm accuracy (tools/rhythm_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Signals: tests/rhythm_ref.py.  reference: the definition of include/jsg.h section 2j evaluated in",
             "float64 on the float32 products y; errors in units of cap (b), worst over the case's elements; ratio = GPU / restatement (1 where both are 0).", "",
             "| signal | Wn | lags | hop | frames | normalise | path | GPU | restatement | ratio | elements differing in bits |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    worst = 0.0
    for what, o, Wn, Lg, hop, n_frames in cases:
        o = np.array(o)
        w = rr.hann(Wn)
        shared = rr.sums(o, w, Lg, hop, n_frames)
        d_in, d_w = torch.from_numpy(o).cuda(), torch.from_numpy(w).cuda()
        for normalise in (0, 1):
            ref = rr.tempogram(o, w, Lg, hop, n_frames, normalise, shared=shared)
            out = torch.empty((o.shape[0], n_frames, Lg), dtype=torch.float32, device="cuda")
            path = jsg.tempogram_kernel_name(d_in, d_w, out, lags=Lg, hop=hop, n_frames=n_frames, normalise=bool(normalise))
            jsg.tempogram_launch(d_in, d_w, out, lags=Lg, hop=hop, n_frames=n_frames, normalise=bool(normalise))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            e_gpu, e_ref = rr.cap_units(got, ref).max(), rr.cap_units(ref["tg32"], ref).max()
            ratio = 1.0 if e_gpu == e_ref else float("inf") if e_ref == 0 else e_gpu / e_ref
            worst = max(worst, ratio)
            lines.append(f"| {what} | {Wn} | {Lg} | {hop} | {n_frames} | {normalise} | {path} | {e_gpu:.4f} | {e_ref:.4f} | {ratio:.3f} | {int((raw(got) != raw(ref['tg32'])).sum())} of {got.size} |")
            print(lines[-1], flush=True)
    yard = math.ceil(1.25 * worst * 2) / 2
    lines += ["", f"Worst GPU / restatement ratio: {worst:.3f}.  YARDSTICKS = 1.25 x that, rounded up to the next half: {yard:g} (tests/rhythm_ref.py).", ""]
    # onset strength and tempo: bits against their restatements
    S = np.array(rr.planes())
    differ = 0
    for lag, m in ((1, 1), (2, 3), (3, 4)):
        differ += int((raw(jsg.onset_strength(S, lag=lag, max_size=m)) != raw(rr.onset32(S, lag, m))).sum())
    lines.append(f"Onset strength on the planes of tests/rhythm_ref.py (3 x 40 x 200; lag, max_size = 1, 1; 2, 3; 3, 4): {differ} of {3 * S.shape[0] * S.shape[1]} elements differ in bits from the restatement.")
    tg = jsg.tempogram(np.array(rr.envelopes()), win_length=384)
    prior = jsg.tempo_prior(384, rr.FRAME_RATE)
    bpm, lag = jsg.tempo(tg, rr.FRAME_RATE)
    same = sum(int(lag[r] == rr.tempo32(tg[r], prior)[0] and raw(bpm[r:r + 1])[0] == raw(np.float32([rr.tempo32(tg[r], prior)[1]]))[0]) for r in range(tg.shape[0]))
    lines += [f"Tempo on the GPU's tempograms of the shared envelopes (Wn 384): {same} of {tg.shape[0]} rows give the restatement's lag and the bits of its bpm; lags {lag.tolist()}.",
              "Agreement with librosa was not measured (librosa is not installed here; its definitions differ as section 2j of include/jsg.h says).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines[-6:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
