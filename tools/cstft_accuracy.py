#!/usr/bin/env python3
"""Accuracy of the complex STFT / inverse STFT kernels against float64, next to a float32 CPU FFT on the same data (tests/cstft_ref.py:
the metric, the yardstick Y and the per-sample inverse bound are defined there).  Writes profiles/cstft_accuracy.md, the table that
the factor M of tests/cstft_ref.py rests on: M = 2 while the worst forward e_gpu / Y is at most 1.6.

    python tools/cstft_accuracy.py [--out FILE] [--sizes 512,1024,...]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cstft_accuracy.md"))
    ap.add_argument("--sizes", default="512,1024,2048,4096,8192")
    args = ap.parse_args()
    import torch
    import cstft_ref as R
    import jadespectrogram_amd as jsg
    torch.cuda.set_device(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [int(s) for s in args.sizes.split(",")]

    def forward(n, w, x, hop, F):
        out = torch.empty((x.shape[0], F, n // 2 + 1), dtype=torch.complex64, device="cuda")
        jsg.cstft(jsg.CStftPlan(n, w), torch.from_numpy(x).cuda(), hop, F, out)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def inverse(n, w, X, hop):
        y = torch.empty((X.shape[0], (X.shape[1] - 1) * hop + n), device="cuda")
        jsg.istft_launch(jsg.CStftPlan(n, w), torch.from_numpy(X).cuda(), hop, X.shape[1], y)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    rows_f, rows_i = [], []
    worst_f, worst_i = {}, {}
    for n in sizes:
        fpb = max(1, 2048 // n)
        cases = []
        for hop in (n // 4, 441):       # walked tiles: 3 rows of 8 CUs + 1 tiles, the last one ragged
            F = 8 * cus * fpb + 1
            cases.append((f"walked tiles, noise, Hann, hop {'n/4' if hop == n // 4 else 441}", R.noise(3, (F - 1) * hop + n, n + hop), hop, F, R.window("hann", n)))
        cases += [(cls,) + R.forward_class(cls, n) for cls in R.FORWARD_CLASSES]
        for name, x, hop, F, w in cases:
            g = R.forward_figures(forward(n, w, x, hop, F), x, n, hop, w)
            rows_f.append(f"| forward | {name} | {n} | {x.shape[0]} x {F} | {g.e:.3g} | {g.Y:.3g} | {g.ratio:.2f} |")
            worst_f[name] = max(worst_f.get(name, 0.0), g.ratio)
            print(rows_f[-1], flush=True)
        inv = [("c2r alone, random bins", "rect", n, R.random_bins(3, 4 * fpb + 3, n, n))]
        inv += [(f"overlap-add, {wk}, hop {hop}", wk, hop, R.random_bins(3, F, n, n + hop)) for wk, hop, F in R.inverse_cases(n)]
        for name, wk, hop, X in inv:
            w = R.window(wk, n)
            ref = R.inverse_f64(X, n, hop, w, (X.shape[1] - 1) * hop + n)
            y = inverse(n, w, X, hop)
            Y_inv = R.inverse_yardstick(X, n)
            g2, g1 = R.inverse_figures(y, ref, Y_inv, 2.0), R.inverse_figures(y, ref, Y_inv, 1.0)
            rows_i.append(f"| inverse | {name} | {n} | {X.shape[0]} x {X.shape[1]} | {g2.err:.3g} | {Y_inv:.3g} | {g2.ratio:.2f} ({g1.ratio:.2f}) |")
            key = name if name.startswith("c2r") else "overlap-add"
            worst_i[key] = max(worst_i.get(key, 0.0), g2.ratio)
            print(rows_i[-1], flush=True)
        # the basis, frame by frame (hop n, rectangular): in slices, 2 (n/2+1) frames of n samples
        X = R.basis_bins(n)
        w = R.window("rect", n)
        y = inverse(n, w, X, n)
        Y_inv = max(R.inverse_yardstick(X[:, f:f + 1024], n) for f in range(0, X.shape[1], 1024))
        b2 = b1 = err = 0.0
        for f in range(0, X.shape[1], 1024):
            Xs = X[:, f:f + 1024]
            ref = R.inverse_f64(Xs, n, n, w, Xs.shape[1] * n)
            ys = y[:, f * n:(f + Xs.shape[1]) * n]
            g2, g1 = R.inverse_figures(ys, ref, Y_inv, 2.0), R.inverse_figures(ys, ref, Y_inv, 1.0)
            if g2.ratio > b2:
                b2, err = g2.ratio, g2.err
            b1 = max(b1, g1.ratio)
        rows_i.append(f"| inverse | c2r alone, basis | {n} | 1 x {X.shape[1]} | {err:.3g} | {Y_inv:.3g} | {b2:.2f} ({b1:.2f}) |")
        worst_i["c2r alone, basis"] = max(worst_i.get("c2r alone, basis", 0.0), b2)
        print(rows_i[-1], flush=True)
    lines = ["# Complex STFT / inverse STFT accuracy (tools/cstft_accuracy.py)", "",
             f"Device: {torch.cuda.get_device_name(0)}, {cus} CUs.  Reference: float64 on the float32 windowed frames / the complex64 bins.",
             "Forward rows: e = the largest over the frames of max_k |X - X_ref| / max_k |X_ref|; Y = the same figure of a float32 CPU FFT",
             "(pocketfft) on the same frames; last column e / Y.  Inverse rows: the error column is |y - y_ref| at the sample with the worst",
             "err / tol, Y is Y_inv, the last column the worst err / tol over every sample with a live envelope at M = 2 (at M = 1).", "",
             "| direction | class | n | rows x frames | e_gpu / error | Y | e / Y, or err / tol at M = 2 (M = 1) |", "|---|---|---|---|---|---|---|"]
    lines += rows_f + rows_i
    lines += ["", "Worst over the sizes, forward e / Y: " + "; ".join(f"{k} {v:.2f}" for k, v in worst_f.items()) + ".",
              "Worst over the sizes, inverse err / tol at M = 2: " + "; ".join(f"{k} {v:.2f}" for k, v in worst_i.items()) + ".", "",
              f"The rule of tests/cstft_ref.py: M = 2 while the worst forward e / Y is at most 1.6; here it is {max(worst_f.values()):.2f}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines[-5:]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
