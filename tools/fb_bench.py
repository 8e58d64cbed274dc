#!/usr/bin/env python3
"""Filterbank spectrogram rate (jsg_stft_fb_launch_strided) against the dB-only call (jsg_stft_db_launch_strided) on the same input, one
process, interleaved: C2 geometry (1024 points, hop 512, mono, 4096 frames per batch, 64 batches per call, 128 Slaney mels) and C3 (2048
points, hop 512, 8 channels AbsMean, 4096 frames, 12 batches per call).  Prints one JSON line per geometry: frames/s of both, their ratio,
and the band launch's bytes (power read + bands written) for the rocprofv3 kernel-trace run that times the band kernel alone:

    python tools/fb_bench.py [--steps 20] [--warmup 5]
    rocprofv3 --kernel-trace --stats -d OUT -o fb -- python tools/fb_bench.py --steps 5 --warmup 1 --geometry c2   (one geometry per trace)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMS = {"c2": dict(n=1024, hop=512, C=1, F=4096, K=64, mels=128), "c3": dict(n=2048, hop=512, C=8, F=4096, K=12, mels=128)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--geometry", choices=sorted(GEOMS), action="append", help="only these (default: all)")
    ap.add_argument("--scratch-mib", type=float, default=0.0, help="scratch size (0: the library's recommendation)")
    args = ap.parse_args()
    import torch
    import jadespectrogram_amd as jsg
    from oracle import jsg_oracle as oracle
    torch.cuda.set_device(0)
    for name, g in GEOMS.items():
        if args.geometry and name not in args.geometry:
            continue
        n, hop, C, F, K, M = g["n"], g["hop"], g["C"], g["F"], g["K"], g["mels"]
        H = n // 2 + 1
        plan = jsg.Plan(n, oracle.window(oracle.WIN_HANN, n))
        fb = jsg.Filterbank(n, 48000.0, M, 0.0, 24000.0)
        S = (F - 1) * hop + n
        base = oracle.synth_audio(C, S + K * 64, seed=1234)
        d_in = torch.empty((K, C, S), dtype=torch.float32, device="cuda")
        for b in range(K):
            d_in[b].copy_(torch.from_numpy(np.ascontiguousarray(base[:, b * 64:b * 64 + S])))
        d_db = torch.empty((K, F, (H + 31) // 32 * 32), dtype=torch.float32, device="cuda")
        d_fb = torch.empty((K, F, M), dtype=torch.float32, device="cuda")
        kw = dict(mix_mode=jsg.capi.MIX_ABSMEAN)
        n_sc = (int(args.scratch_mib * 2 ** 18) if args.scratch_mib > 0 else
                jsg.stft_fb_scratch_floats(plan, fb, d_in, hop, F, d_fb, strided=True, **kw))
        d_sc = torch.empty(n_sc, dtype=torch.float32, device="cuda")
        kname = jsg.stft_fb_kernel_name(plan, fb, d_in, hop, F, d_fb, strided=True, **kw)
        st = torch.cuda.Stream()
        s = st.cuda_stream

        def db():
            jsg.stft_db_strided(plan, d_in, hop, F, d_db, stream=s, **kw)

        def fbk():
            jsg.stft_fb_db_strided(plan, fb, d_in, hop, F, d_fb, d_scratch=d_sc, stream=s, **kw)

        times = {"db": [], "fb": []}
        with torch.cuda.stream(st):
            for i in range(args.warmup + args.steps):
                for key, fn in (("db", db), ("fb", fbk)) if i % 2 == 0 else (("fb", fbk), ("db", db)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    fn()
                    e1.record(st)
                    e1.synchronize()
                    if i >= args.warmup:
                        times[key].append(e0.elapsed_time(e1) * 1e-3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        frames = K * F
        band_bytes = K * F * (H * 4 + M * 4)          # power columns read + band columns written (one column per frame: AbsMean)
        print(json.dumps({"geometry": name, "n": n, "hop": hop, "channels": C, "frames_per_batch": F, "batches": K, "mels": M,
                          "stft_kernel": kname, "scratch_MiB": round(n_sc * 4 / 2 ** 20, 1), "nnz": int(fb.weights.size),
                          "db_frames_per_s": frames / med["db"], "fb_frames_per_s": frames / med["fb"], "fb_over_db": med["db"] / med["fb"],
                          "db_ms": med["db"] * 1e3, "fb_ms": med["fb"] * 1e3, "band_kernel_bytes_per_call": band_bytes}), flush=True)


if __name__ == "__main__":
    main()
