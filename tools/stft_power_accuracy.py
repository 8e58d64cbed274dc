#!/usr/bin/env python3
"""Accuracy of the power-STFT plans on impulses, impulse pairs, tones, a comb and noise against float64, next to a float32 CPU FFT on
the same frames (tests/stft_basis.py: the classes, the metric e, the yardstick Y and the bound e <= M * Y are defined there).  Prints
the table that M rests on, one row per plan, class and window (the worst call of the class), as markdown; profiles/stft_power_accuracy.md
keeps it.  Runs on the kernel mirror (oracle/jsg_mirror.c) by default, on the device with --gpu (where the columns must also equal the
mirror's bit for bit: the last column).

    python tools/stft_power_accuracy.py [--gpu] [--thin] [--faults] [--sizes 512,1024,...] [--out FILE]

--thin   the CPU suite's thinned calls instead of the full ones
--faults the fault table of tests/test_stft_basis_ref.py: which injected fault the bound catches, and whether the old gate did
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--thin", action="store_true")
    ap.add_argument("--faults", action="store_true")
    ap.add_argument("--sizes", default="512,1024,2048,4096,8192")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import stft_basis as B
    from oracle import mirror as mirror_mod
    mirror = mirror_mod.load()
    sizes = [int(s) for s in args.sizes.split(",")]
    lines = []

    def say(s=""):
        lines.append(s)
        print(s, flush=True)

    if args.faults:
        import test_stft_basis_ref as T
        say("| fault | n | caught by e <= M * Y on (worst e / Y) | old gate (assert_power_close, 12 frames of synth_audio, Hann, hop n/2) |")
        say("|---|---|---|---|")
        for n in sizes:
            for fault in T.FAULTS:
                new, old = T.fault_verdicts(n, fault)
                hits = ", ".join(f"{k} {v:.3g}" for k, v in new.items() if v > B.M) or "nothing"
                say(f"| {fault} | {n} | {hits} | {old} |")
    else:
        if args.gpu:
            import torch
            import jadespectrogram_amd as jsg
            torch.cuda.set_device(0)
            say(f"Device: {torch.cuda.get_device_name(0)}.  " + ("Thinned calls." if args.thin else "Full calls."))
        else:
            say("Kernel mirror on the CPU.  " + ("Thinned calls." if args.thin else "Full calls."))
        say()
        say("| plan | class | window | calls | frames | e | Y | e / Y | worst at (call; frame, bin) | zero-reference frames |" + (" equals the mirror |" if args.gpu else ""))
        say("|---|---|---|---|---|---|---|---|---|---|" + ("---|" if args.gpu else ""))
        worst = (0.0, "")
        t0 = time.time()
        for n, sel, plan in B.PINS:
            if n not in sizes:
                continue
            pair = B.plan_is_pair(plan)
            for cls in B.CLASSES:
                for wname in B.CLASS_WINDOWS[cls]:
                    cl = B.calls(cls, n, wname, pair=pair, thin=args.thin)
                    best, frames, zeros, same = None, 0, 0, True
                    for call in cl:
                        ref = B.mirror_columns(mirror, plan, call)
                        if args.gpu:
                            P = B.gpu_columns(jsg, torch, call, sel, plan)
                            same = same and bool((P.view(np.uint32) == ref.view(np.uint32)).all())
                        else:
                            P = ref
                        g = B.figures({0: P}, call)[0]
                        frames += call.F
                        zeros = max(zeros, g.zero_frames)
                        if best is None or g.ratio > best[0].ratio:
                            best = (g, call)
                    g, call = best
                    say(f"| {plan} | {cls} | {wname} | {len(cl)} | {frames} | {g.e:.3g} | {g.Y:.3g} | {g.ratio:.2f} | {call.name}; {g.frame}, {g.bin} | "
                        f"{zeros} |" + ((" yes |" if same else " NO |") if args.gpu else ""))
                    if g.ratio > worst[0]:
                        worst = (g.ratio, f"{plan}, {cls}, {wname}")
        rule = math.ceil(worst[0] * 1.25 * 2) / 2
        say()
        say(f"Worst e / Y: {worst[0]:.2f} ({worst[1]}).  Times 1.25, rounded up to the next half: {rule:.1f}; tests/stft_basis.py holds M = {B.M}.  "
            f"({time.time() - t0:.0f} s)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
