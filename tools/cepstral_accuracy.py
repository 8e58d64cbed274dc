#!/usr/bin/env python3
"""Accuracy of the projection (jsg_mfcc_launch) and of delta (jsg_delta_launch, include/jsg.h section 2k) on the planes of
tests/cepstral_ref.py and on every path of jsg_mfcc_plan: per case the worst error of the GPU and of the float32 restatement against
the float64 evaluation in units of the stated per-element bound, the elements whose bits differ from the restatement's, and the kernel
path.  Writes profiles/cepstral_accuracy.md.

    python tools/cepstral_accuracy.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def units(got, ref64, bound):
    import numpy as np
    err = np.abs(got.astype(np.float64) - ref64)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cepstral_accuracy.md"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import cepstral_ref as cr
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    lines = ["# Cepstral accuracy (tools/cepstral_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Planes: tests/cepstral_ref.py (3 rows x 200 frames of dB-like values).  reference: the sums of include/jsg.h",
             "section 2k in float64 on the exact products of the float32 operands; errors in units of the stated bound, (B + 2) u sum |D| |S| and",
             "(Wd + 2) u sum |w| |X|, worst over the case's elements.", "",
             "## Projection", "",
             "| table | bands | coefficients | path | frames per item | GPU | restatement | elements differing in bits |", "|---|---|---|---|---|---|---|---|"]
    cases = [("DCT ortho", 128, 20, dict()), ("DCT ortho, lifter 22", 128, 20, dict(lifter=22.0)), ("DCT none", 128, 13, dict(norm="none")), ("DCT ortho", 40, 13, dict()),
             ("DCT ortho", 257, 20, dict()), ("DCT ortho", 64, 32, dict()), ("DCT ortho", 64, 40, dict()), ("DCT ortho", 128, 128, dict()),
             ("inverse DCT ortho", 20, 128, dict(inverse=True)), ("inverse DCT none, lifter 22", 13, 40, dict(inverse=True, norm="none", lifter=22.0)),
             ("DCT ortho", 128, 256, None)]
    for what, B, M, kw in cases:
        S = np.array(cr.planes()[:, :, :B])
        if kw is None:
            what, D = "noise, at the table limit", np.array(cr.tables(M, B, seed=3))
        elif kw.get("inverse"):
            D = jsg.mfcc_table(M, B, **kw)
        else:
            D = jsg.mfcc_table(B, M, **kw)
        d_S, d_D = torch.from_numpy(S).cuda(), torch.from_numpy(D).cuda()
        out = torch.empty((S.shape[0], S.shape[1], M), dtype=torch.float32, device="cuda")
        path, F, _ = jsg.mfcc_plan(d_S, d_D, out)
        jsg.mfcc_launch(d_S, d_D, out)
        torch.cuda.synchronize()
        got, want = out.cpu().numpy(), cr.project32(S, D)
        C64, bound = cr.project64(S, D)
        lines.append(f"| {what} | {B} | {M} | {path} | {F} | {units(got, C64, bound):.4f} | {units(want, C64, bound):.4f} | {int((cr.raw(got) != cr.raw(want)).sum())} of {got.size} |")
        print(lines[-1], flush=True)
    lines += ["", "## Delta", "", "| width | order | mode | coefficients | GPU | restatement | elements differing in bits |", "|---|---|---|---|---|---|---|"]
    for width, order, mode, M in ((9, 1, "interp", 20), (9, 2, "interp", 20), (9, 1, "nearest", 20), (3, 1, "interp", 13), (5, 2, "nearest", 65), (255, 1, "nearest", 20),
                                  (199, 2, "interp", 20)):
        X = np.array(cr.planes()[:, :, :M])
        w = jsg.delta_weights(width, order)
        code = cr.INTERP if mode == "interp" else cr.NEAREST
        got, want = jsg.delta(X, width, order, mode), cr.delta32(X, w, code)
        Y64, bound = cr.delta64(X, w, code)
        lines.append(f"| {width} | {order} | {mode} | {M} | {units(got, Y64, bound):.4f} | {units(want, Y64, bound):.4f} | {int((cr.raw(got) != cr.raw(want)).sum())} of {got.size} |")
        print(lines[-1], flush=True)
    lines += ["", "Agreement with librosa was not measured (librosa is not installed here; the definitions differ as section 2k of include/jsg.h says).", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
