#!/usr/bin/env python3
"""Per-kernel resource usage of the built STFT units (VGPRs, SGPRs, spills, scratch, LDS) from the code objects' metadata, plus
instruction-mix counts from the disassembly.  CPU only (llvm-objcopy / clang-offload-bundler / llvm-readelf / llvm-objdump).

    python tools/kernel_regs.py [--isa PATTERN] [obj ...]      (default objects: jadespectrogram_amd/build/jsg_stft_{a,b}.o, jsg_cstft.o, jsg_pvoc.o, jsg_hpss.o, jsg_resample.o, jsg_cqt.o, jsg_yin.o, jsg_rhythm.o, jsg_cepstral.o and jsg_spectral.o; jsg_filterbank.o holds the band kernel,
                                                               jsg_display_axis.o the display-axis colour kernel, jsg_cstft.o the
                                                               complex STFT / inverse STFT kernels, jsg_pvoc.o the phase vocoder,
                                                               jsg_hpss.o the harmonic-percussive separation, jsg_resample.o the
                                                               band-limited resampler, jsg_cqt.o the constant-Q kernel,
                                                               jsg_yin.o the YIN kernel,
                                                               jsg_rhythm.o the onset, tempogram and tempo kernels,
                                                               jsg_cepstral.o the projection (MFCC) and delta kernels,
                                                               jsg_spectral.o the spectral shape kernels;
                                                               jsgx_beat.o, of libjsgx.so, the beat tracker, jsgx_cdist.o the
                                                               pairwise cost, jsgx_dtw.o the time warping, jsgx_viterbi.o
                                                               the Viterbi kernels, jsgx_pyin.o the pYIN kernels, jsgx_knn.o
                                                               the nearest-frame, recurrence and nn_filter kernels and
                                                               jsgx_rqa.o the recurrence quantification alignment, jsgx_path_enhance.o
                                                               the path enhancement and the lag conversion, jsgx_nmf.o the
                                                               non-negative matrix factorisation, jsgx_pcen.o the per-channel
                                                               energy normalisation, jsgx_peak.o the peak picking, jsgx_sync.o the
                                                               segment aggregation and the time-delay embedding, jsgx_agglo.o the
                                                               agglomerative segmentation: name them)
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(obj, tmp):
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.path.join(tmp, "scratch.o")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}"])
    return co


def short(name):
    out = subprocess.check_output(["c++filt", name]).decode().strip()
    m = re.search(r"stft_db_kernel<jsg::Cfg<([^>]*)>, (\d+), (\d+), (\d+), (\d+)>", out)
    if not m:
        return out[:60]
    v = [int(x.replace("(int)", "")) for x in m.group(1).split(", ")]
    tag = f"N{v[0]} {v[1]}x{v[2]}x{v[3]} L{v[4]} WPB{v[9]}" + (" PAIR" if len(v) > 15 and v[15] else "")
    return f"{tag:28s} MIX{m.group(2)} OUT{m.group(3)} STR{m.group(4)} XLOG{m.group(5)}"


def main():
    args = sys.argv[1:]
    isa_pat = None
    if args and args[0] == "--isa":
        isa_pat = args[1]
        args = args[2:]
    objs = args or [os.path.join(ROOT, "jadespectrogram_amd", "build", f) for f in ("jsg_stft_a.o", "jsg_stft_b.o", "jsg_cstft.o", "jsg_pvoc.o", "jsg_hpss.o", "jsg_resample.o", "jsg_cqt.o", "jsg_yin.o", "jsg_rhythm.o", "jsg_cepstral.o", "jsg_spectral.o")]
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            co = code_object(obj, tmp)
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).decode()
            dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co]).decode()
            mix = {}
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = m.group(1)
                    mix[cur] = {}
                    continue
                if cur and line.strip() and not line.startswith("Disassembly"):
                    op = line.split("//")[0].split()
                    if op:
                        mix[cur][op[0]] = mix[cur].get(op[0], 0) + 1
            for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                g = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]
                name = g("name")
                if not any(k in name for k in ("stft_db_kernel", "fb_band_kernel", "colormap_axis_kernel", "cstft_fwd_kernel", "istft_c2r_kernel", "istft_ola_kernel", "pvoc_walk_kernel",
                                               "pvoc_scan_kernel", "hpss_freq_kernel", "hpss_time_kernel", "resample_kernel", "cqt_kernel", "yin_kernel", "onset_kernel", "tempogram_kernel", "tempo_kernel", "mfcc_kernel", "delta_kernel", "spectral_regs_kernel",
                                               "spectral_stream_kernel", "beat_kernel", "cdist_kernel", "dtw_kernel", "dtw_backtrace_kernel", "viterbi_forward_kernel",
                                               "viterbi_jump_kernel", "viterbi_ends_kernel", "viterbi_trace_kernel", "pyin_observe_kernel", "pyin_forward_kernel",
                                               "knn_kernel", "knn_merge_kernel", "recurrence_kernel", "nn_filter_kernel", "rqa_kernel", "rqa_backtrace_kernel",
                                               "path_enhance_kernel", "lag_columns_kernel", "lag_rows_kernel", "nmf_gram_kernel", "nmf_chunk_sum_kernel",
                                               "nmf_update_a_kernel", "nmf_partial_c_kernel", "nmf_update_c_kernel", "pcen_scan_kernel", "pcen_carry_kernel", "pcen_apply_kernel",
                                               "peak_single_kernel", "peak_stats_kernel", "peak_row_kernel", "peak_cand_kernel", "peak_carry_kernel", "peak_emit_kernel",
                                               "sync_segments_kernel", "sync_aggregate_kernel", "stack_memory_kernel",
                                               "agglo_segments_kernel", "agglo_copy_kernel", "agglo_offsets_kernel", "agglo_wave_kernel", "agglo_group_kernel")):
                    continue
                mx = mix.get(name, {})
                valu = sum(c for o, c in mx.items() if o.startswith("v_"))
                pk = sum(c for o, c in mx.items() if o.startswith("v_pk_"))
                lds = sum(c for o, c in mx.items() if o.startswith("ds_"))
                vmem = sum(c for o, c in mx.items() if o.startswith(("global_", "buffer_", "scratch_")))
                print(f"{short(name)}  vgpr {g('vgpr_count'):>3} spill {g('vgpr_spill_count'):>2} sgpr {g('sgpr_count'):>3} sspill {g('sgpr_spill_count'):>2} "
                      f"scratch {g('private_segment_fixed_size'):>3} lds {g('group_segment_fixed_size'):>6} | static: valu {valu} (pk {pk}) ds {lds} vmem {vmem} "
                      f"nop {mx.get('s_nop', 0)} mov {mx.get('v_mov_b32_e32', 0) + mx.get('v_mov_b32_e64', 0)} swap {mx.get('v_permlane32_swap_b32_e32', 0)}")
                if isa_pat and re.search(isa_pat, short(name)):
                    print(dis.split(f"<{name}>:")[1].split("\n\n")[0][:2000000])


if __name__ == "__main__":
    main()
