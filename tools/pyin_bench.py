#!/usr/bin/env python3
"""Time of pYIN on the GPU (include/jsgx.h section 5, libjsgx.so) at librosa's defaults: 8 rows x 4096 frames, P = 601 pitch bins, tau
10..338, N = 100 thresholds.  The observation kernel against the bytes it moves and a measured copy; the factored decoder at W = 50 and
at W = 25, and at W = 25 next to jsgx_viterbi_launch's band form on the same model with the two kinds of state interleaved (half-width
51, the widest that fits) and next to the recurrence written with torch operations; the three ways the forward kernel keeps U in LDS;
and the lanes that share a pitch bin (the first design's rule, as many as 1024 lanes hold, under a cap of 64 ... 1) over P = 16, 64, 256 and W = 10, 50, 128.

    python tools/pyin_bench.py --build-variants            (no GPU) builds tools/variants/libjsgx_pyin_{loop0,loop1,loop2,g64,...,g1}.so
    python tools/pyin_bench.py --run OUT.json [--lib LIB] [--set main|loop|g]      HIP events, best of 7 after a warm-up
    python tools/pyin_bench.py --report profiles/pyin_bench.md --main OUT.json [--variant NAME OUT.json ...]

Every --run is a process of its own: a process loads one build of the library."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, FMIN, FMAX, HOP, FRAME = 22050, 65.40639132514966, 2093.004522404789, 512, 2048
ROWS, FRAMES, P, BPS, N = 8, 4096, 601, 10, 100
TAU_MIN, TAU_MAX = 10, 338
REPS = 7
TORCH_FRAMES = 128
OBSERVE_BURST = 50        # launches of the observation kernel between two events
VARIANTS = {"loop0": ["-DJSGX_PYIN_LOOP=0"], "loop1": ["-DJSGX_PYIN_LOOP=1"], "loop2": ["-DJSGX_PYIN_LOOP=2"]}
VARIANTS.update({f"g{c}": [f"-DJSGX_PYIN_MAX_G={c}"] for c in (64, 32, 16, 8, 4, 2, 1)})
G_SHAPES = ((16, 10), (16, 50), (16, 128), (64, 10), (64, 50), (64, 128), (256, 10), (256, 50), (256, 128))      # (P, W): where P * G <= 1024 leaves a choice


def build_variants():
    from jadespectrogram_amd import _build
    hipcc = _build._hipcc()
    vdir = os.path.join(ROOT, "tools", "variants")
    os.makedirs(vdir, exist_ok=True)
    _build.build_lib()
    for name, flags in VARIANTS.items():
        objs = []
        for src in _build.SOURCES_X:
            o = os.path.join(_build.PKG, "build", os.path.splitext(src)[0] + ".o")
            if "pyin" in src:
                o = os.path.join(vdir, f"{os.path.splitext(src)[0]}_{name}.o")
                cmd = [hipcc, "-std=c++17", "-O3", "-fPIC", "-c", os.path.join(_build.CSRC, src), "-o", o, "-I", os.path.join(ROOT, "include")] + flags + _build.VISIBILITY
                cmd += [f"--offload-arch={_build.ARCH}"] + _build.HIP_FLAGS if src.endswith(".hip") else ["-ffp-contract=off", "-D__HIP_PLATFORM_AMD__"]
                subprocess.check_call(cmd)
            objs.append(o)
        out = os.path.join(vdir, f"libjsgx_pyin_{name}.so")
        subprocess.check_call([hipcc, "-shared", "-fPIC", f"--offload-arch={_build.ARCH}", "-o", out] + objs)
        print(out)


def best_time(torch, fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return min(times)


def triangle(W):
    import numpy as np
    return np.concatenate([np.arange(1, W + 2), np.arange(W, 0, -1)]).astype(np.float64)


def audio(torch):
    """Rows of gliding harmonic tones with noise and silent stretches: frames with many troughs, frames with few and frames with none."""
    import numpy as np
    rng = np.random.default_rng(0)
    L = (FRAMES - 1) * HOP
    t = np.arange(L) / SR
    rows = []
    for r in range(ROWS):
        f0 = 110.0 * 2 ** (r / 4.0) * 2 ** (0.3 * np.sin(2 * np.pi * 0.2 * t + r))
        phase = 2 * np.pi * np.cumsum(f0) / SR
        x = sum(np.sin(h * phase) / h for h in (1, 2, 3, 4)) + 0.05 * rng.standard_normal(L)
        x[(np.sin(2 * np.pi * 0.13 * t + r) > 0.8)] = 0.0
        rows.append(x.astype(np.float32))
    return torch.from_numpy(np.stack(rows)).cuda()


def interleaved_band(np, lw, off, sw, W):
    """The band table of jsgx_viterbi_launch for the same model with the state 2p + u: half-width 2W + 1."""
    Pn, H = off.size, 2 * W + 1
    table = np.full((2 * H + 1, 2 * Pn), -np.inf, np.float32)
    for u in range(2):
        for v in range(2):
            for k in range(2 * W + 1):                    # p' - p + W = k
                p = np.arange(Pn)
                d = p + k - W
                ok = (d >= 0) & (d < Pn)
                i, j = 2 * p[ok] + u, 2 * d[ok] + v
                table[i - j + H, j] = (off[p[ok]] + lw[k]) + sw[2 * u + v]
    return table, H


def torch_loop(torch, emit, p0, lw, off, sw, W, frames):
    """The factored recurrence in torch operations over the first `frames` frames (psi is kept, as a decoder has to)."""
    Q, T, S = emit.shape
    Pn = S // 2
    F = torch.nn.functional
    V = p0[None] + emit[:, 0]
    psi = torch.empty((frames, Q, S), dtype=torch.int64, device="cuda")
    lw_rev, sw2 = lw.flip(0), sw.view(2, 2)
    for t in range(1, frames):
        U = V.view(Q, 2, Pn) + off
        m, at = (F.pad(U, (W, W), value=float("-inf")).unfold(-1, 2 * W + 1, 1) + lw_rev).max(-1)         # [Q][u][p']
        c, u = (m[:, :, None, :] + sw2[None, :, :, None]).max(1)                                           # [Q][u'][p']
        psi[t] = (u * Pn + torch.gather(at, 1, u) + torch.arange(Pn, device="cuda") - W).reshape(Q, S)
        V = c.reshape(Q, S) + emit[:, t]
    return V


def run(args):
    import numpy as np
    import torch
    import jadespectrogram_amd as jsg
    if args.lib:
        jsg.capix.LIB_PATH = os.path.abspath(args.lib)
    torch.cuda.set_device(0)
    rec = {"lib": os.path.basename(args.lib) if args.lib else "libjsgx.so", "set": args.set, "device": f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]})", "reps": REPS}

    def tables(W):
        t = jsg.pyin_tables(SR, FMIN, P, BPS, W, triangle(W), TAU_MIN, TAU_MAX, N)
        return t, {k: torch.from_numpy(v).cuda() for k, v in t.items()}

    def decode_time(emit, d, seqs):
        states = torch.empty((seqs, emit.shape[1]), dtype=torch.int32, device="cuda")
        need = jsg.pyin_decode_scratch_bytes(emit, d["log_init"], d["log_window"], d["src_offset"], d["log_switch"], states)
        scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
        return best_time(torch, lambda: jsg.pyin_decode_launch(emit, d["log_init"], d["log_window"], d["src_offset"], d["log_switch"], states, d_scratch=scratch)), states

    if args.set == "g":         # the cap on G matters only where P * G <= 1024 leaves a choice; 256 sequences, one workgroup per compute unit
        Q, T = 256, 2048
        rng = np.random.default_rng(1)
        rec["g"] = []
        for Pg, Wg in G_SHAPES:
            emit = torch.from_numpy((-4.0 * rng.random((Q, T, 2 * Pg))).astype(np.float32)).cuda()
            t = jsg.pyin_tables(SR, FMIN, Pg, 1, Wg, triangle(Wg), TAU_MIN, TAU_MAX, N)
            d = {k: torch.from_numpy(v).cuda() for k, v in t.items()}
            d["log_init"] = torch.zeros((2 * Pg,), dtype=torch.float32, device="cuda")
            sec, _ = decode_time(emit, d, Q)
            rec["g"].append({"P": Pg, "W": Wg, "seqs": Q, "frames": T, "plan": jsg.pyin_decode_plan(Pg, Wg, T, Q), "seconds": sec, "us_per_frame": sec / T * 1e6})
        json.dump(rec, open(args.run, "w"), indent=1)
        print(json.dumps(rec["g"]))
        return

    x = audio(torch)
    plane = jsg.yin_cmnd(x, SR, FMIN, FMAX, frame_length=FRAME, hop_length=HOP)
    R, T, lags = plane.shape
    assert (R, T, lags) == (ROWS, FRAMES, TAU_MAX + 1), plane.shape
    t50, d50 = tables(50)
    emit = torch.empty((R, T, 2 * P), dtype=torch.float32, device="cuda")
    voiced = torch.empty((R, T), dtype=torch.float32, device="cuda")
    observe = lambda: jsg.pyin_observe_launch(plane, TAU_MIN, TAU_MAX, d50["prior"], d50["decay"], d50["norm"], d50["edges"], emit, d_voiced_prob=voiced)
    if args.set == "main":
        big = torch.empty((64 << 20,), dtype=torch.float32, device="cuda")         # 256 MiB each way
        dst = torch.empty_like(big)
        sec = best_time(torch, lambda: dst.copy_(big))
        rec["copy"] = {"bytes_moved": 2 * big.numel() * 4, "seconds": sec, "gb_per_s": 2 * big.numel() * 4 / sec / 1e9}
        # The kernel takes less than a tenth of a millisecond, and one call through the Python layer (argument checks, ctypes) takes a
        # good part of that on the host: the argument block is built once and OBSERVE_BURST launches go back to back between the two
        # events, so that the queue stays full and the interval is the kernels'.  One call through the Python layer is timed next to it.
        import ctypes
        block = jsg.spectrogram._pyin_observe_args(plane, TAU_MIN, TAU_MAX, d50["prior"], d50["decay"], d50["norm"], d50["edges"], 0.01, emit, None, voiced)
        launch, stream = jsg.capix.lib().jsgx_pyin_observe_launch, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def burst():
            for _ in range(OBSERVE_BURST):
                launch(ctypes.byref(block), stream)

        sec_call = best_time(torch, observe)
        sec = best_time(torch, burst) / OBSERVE_BURST
        moved = 4 * (R * T * lags + R * T * 2 * P + R * T)
        rec["observe"] = {"plan": jsg.pyin_observe_plan(TAU_MIN, TAU_MAX, P, T, R, N), "seconds": sec, "seconds_one_call": sec_call, "burst": OBSERVE_BURST, "bytes_moved": moved, "gb_per_s": moved / sec / 1e9,
                          "of_copy": moved / sec / 1e9 / rec["copy"]["gb_per_s"], "us_per_frame": sec / (R * T) * 1e6,
                          "voiced_frames": float((voiced > 0.5).float().mean())}
    observe()
    torch.cuda.synchronize()
    rec["decode"] = {}
    for W in (50, 25):
        tw, dw = tables(W)
        sec, states = decode_time(emit, dw, R)
        rec["decode"][str(W)] = {"plan": jsg.pyin_decode_plan(P, W, T, R), "seconds": sec, "us_per_frame": sec / T * 1e6,
                                 "voiced_states": float((states < P).float().mean())}
        if W == 25 and args.set == "main":
            table, H = interleaved_band(np, tw["log_window"], tw["src_offset"], tw["log_switch"], W)
            emit_i = emit.view(R, T, 2, P).transpose(2, 3).reshape(R, T, 2 * P).contiguous()
            init_i = dw["log_init"].view(2, P).t().reshape(-1).contiguous()
            d_table = torch.from_numpy(table).cuda()
            st_i = torch.empty((R, T), dtype=torch.int32, device="cuda")
            scratch = torch.empty((jsg.viterbi_scratch_bytes(emit_i, init_i, d_table, st_i, band_half=H),), dtype=torch.uint8, device="cuda")
            sec_b = best_time(torch, lambda: jsg.viterbi_launch(emit_i, init_i, d_table, st_i, band_half=H, d_scratch=scratch))
            same = float(((st_i % 2) * P + st_i // 2 == states).float().mean())
            rec["band51"] = {"plan": jsg.viterbi_plan(2 * P, T, R, band_half=H), "seconds": sec_b, "us_per_frame": sec_b / T * 1e6, "states_equal_share": same}
            sec_t = best_time(torch, lambda: torch_loop(torch, emit, dw["log_init"], dw["log_window"], dw["src_offset"], dw["log_switch"], W, TORCH_FRAMES), reps=3)
            rec["torch25"] = {"frames_timed": TORCH_FRAMES, "seconds": sec_t, "us_per_frame": sec_t / (TORCH_FRAMES - 1) * 1e6}
    json.dump(rec, open(args.run, "w"), indent=1)
    print(json.dumps(rec))


def report(args):
    main = json.load(open(args.main))
    out = ["# pYIN on the GPU: times at librosa's defaults", "",
           f"`tools/pyin_bench.py` on {main['device']}: HIP events, the best of {main['reps']} launches after a warm-up.  {ROWS} rows x {FRAMES} frames, P = {P}, tau {TAU_MIN}..{TAU_MAX}, "
           f"N = {N}; the d' plane is jsg_yin_launch's of gliding four-harmonic tones with noise and silent stretches.", ""]
    c, o = main["copy"], main["observe"]
    out += ["## The observation kernel", "",
            f"- copy of 256 MiB device to device: {c['gb_per_s']:.0f} GB/s moved (read + write)",
            f"- `{o['plan'][0]}` ({o['plan'][1]} lanes, {o['plan'][2]} bytes of LDS, {o['plan'][3]} frame per workgroup), {o['burst']} launches back to back from one prepared argument "
            f"block, per launch: {o['seconds'] * 1e3:.3f} ms for {ROWS * FRAMES} frames (one call through the Python layer between two events: {o['seconds_one_call'] * 1e3:.3f} ms, host time included), "
            f"{o['us_per_frame']:.3f} us per frame; it moves {o['bytes_moved'] / 1e6:.1f} MB (the plane in, the emissions and voiced_prob out): {o['gb_per_s']:.0f} GB/s, "
            f"{100 * o['of_copy']:.1f} % of the copy; the same 202 MB every launch, less than the 256 MiB Infinity Cache, so not an HBM figure", f"- frames with voiced_prob > 0.5: {100 * o['voiced_frames']:.0f} %", ""]
    out += ["## The decoder", "", "| launch | shape | lanes | LDS bytes | ms | us per frame |", "|---|---|---|---|---|---|"]
    for W in ("50", "25"):
        d = main["decode"][W]
        out.append(f"| jsgx_pyin_decode_launch | P = {P}, W = {W}, {ROWS} x {FRAMES} | {d['plan'][2]} | {d['plan'][3]} | {d['seconds'] * 1e3:.2f} | {d['us_per_frame']:.2f} |")
    b, t = main["band51"], main["torch25"]
    out.append(f"| jsgx_viterbi_launch, `{b['plan'][0]}`, states interleaved | S = {2 * P}, half-width 51, {ROWS} x {FRAMES} | {b['plan'][1]} | {b['plan'][2]} | {b['seconds'] * 1e3:.2f} | {b['us_per_frame']:.2f} |")
    out.append(f"| the factored recurrence as a torch loop ({t['frames_timed']} frames timed) | P = {P}, W = 25, {ROWS} rows | | | | {t['us_per_frame']:.1f} |")
    d25 = main["decode"]["25"]
    out += ["", f"At W = 25 the factored kernel takes {d25['us_per_frame'] / b['us_per_frame']:.2f} of the time of the interleaved band form "
            f"({b['us_per_frame'] / d25['us_per_frame']:.2f} x) and {d25['us_per_frame'] / t['us_per_frame']:.4f} of the torch loop's "
            f"({t['us_per_frame'] / d25['us_per_frame']:.0f} x).  The two decoders add the three terms of a transition in different orders, so their states need not be equal: "
            f"{100 * b['states_equal_share']:.2f} % of the frames are.", ""]
    if args.variant:
        loops = [(n, json.load(open(p))) for n, p in args.variant if n.startswith("loop")]
        gs = [(n, json.load(open(p))) for n, p in args.variant if n.startswith("g") or n == "rule"]        # rule: the product build
        if loops:
            out += ["## How U is kept in LDS (JSGX_PYIN_LOOP)", "", "| build | W = 50, us per frame | W = 25, us per frame |", "|---|---|---|"]
            for n, r in loops:
                out.append(f"| {n} | {r['decode']['50']['us_per_frame']:.2f} | {r['decode']['25']['us_per_frame']:.2f} |")
            out.append("")
        if gs:
            g0 = gs[0][1]["g"][0]
            out += [f"## The lanes that share a pitch bin ({g0['seqs']} sequences x {g0['frames']} frames, us per frame; the G of the build in brackets)", "",
                    "| P, W | " + " | ".join(n for n, _ in gs) + " |", "|---|" + "---|" * len(gs)]
            for i, e in enumerate(g0 and gs[0][1]["g"]):
                out.append(f"| {e['P']}, {e['W']} | " + " | ".join(f"{r['g'][i]['us_per_frame']:.2f} [{r['g'][i]['plan'][1]}]" for _, r in gs) + " |")
            out.append("")
    open(args.report, "w").write("\n".join(out))
    print("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--run")
    ap.add_argument("--lib")
    ap.add_argument("--set", default="main", choices=("main", "loop", "g"))
    ap.add_argument("--report")
    ap.add_argument("--main")
    ap.add_argument("--variant", nargs=2, action="append", metavar=("NAME", "JSON"))
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    if args.run:
        return run(args)
    if args.report:
        return report(args)
    ap.error("one of --build-variants, --run, --report")


if __name__ == "__main__":
    main()
