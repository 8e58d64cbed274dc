"""jadespectrogram_amd -- MI355X-native (gfx950) STFT spectrogram engine behind the reference's Spectrogram API.

The compute path is hand-written HIP in libjsg.so (csrc/), reached through the C-ABI of include/jsg.h.
Importing this package does not load the library; the first call does, and fails loudly if it is missing.
"""
from . import capi, capix  # noqa: F401
from .capi import JsgError  # noqa: F401
from .spectrogram import (CColorPalette, Filterbank, FreqAxis, Plan, Spectrogram, SpectrogramDisplay, StftLaunch, colormap, colormap_lut,  # noqa: F401
                          colormap_axis, colormap_range, columns_from_tail_layout, feed_samples, memsize_blocks, next_power_of_2, stft_db, stft_db_batches, stft_db_strided, stft_db_strided_kernel_name, stft_image, stft_image_needs_scratch, stft_image_strided, stft_image_strided_needs_scratch, stft_kernel_name, window,
                          mel_spectrogram_db, stft_fb_db, stft_fb_db_strided, stft_fb_kernel_name, stft_fb_scratch_floats, fb_band_plan,
                          CStftPlan, cstft, istft, istft_launch, istft_nola, istft_scratch_floats, stft,
                          phase_vocoder, phase_vocoder_launch, pvoc_frames, time_stretch,
                          hpss, hpss_audio, hpss_launch, hpss_scratch_bytes,
                          Resampler, pitch_shift, resample, resample_kernel_name, resample_launch, resample_length, resample_plan, sinc_table,
                          CqtBasis, cqt, cqt_db, cqt_frames, cqt_frequencies, cqt_kernel_name, cqt_launch, cqt_plan, vqt,
                          yin, yin_cmnd, yin_frames, yin_kernel_name, yin_launch, yin_plan,
                          estimate_tempo, onset_strength, onset_strength_launch, tempo, tempo_launch, tempo_prior, tempogram, tempogram_frames,
                          tempogram_kernel_name, tempogram_launch, tempogram_plan,
                          beat_launch, beat_log_table, beat_plan, beat_scratch_bytes, beat_track, beat_track_audio,
                          cdist, cdist_launch, cdist_plan, dtw, dtw_launch, dtw_plan, dtw_scratch_bytes,
                          viterbi, viterbi_band_transition, viterbi_launch, viterbi_plan, viterbi_scratch_bytes,
                          pyin, pyin_geometry, pyin_decode_launch, pyin_decode_plan, pyin_decode_scratch_bytes, pyin_observe_launch, pyin_observe_plan, pyin_prior, pyin_tables,
                          cross_similarity, knn, knn_default_k, knn_launch, knn_plan, knn_scratch_bytes, nn_filter, nn_filter_launch, recurrence_launch, recurrence_matrix,
                          rqa, rqa_launch, rqa_plan, rqa_scratch_bytes,
                          diagonal_filter, lag_launch, lag_to_recurrence, path_enhance, path_enhance_filters, path_enhance_launch, path_enhance_plan, recurrence_to_lag,
                          decompose, nmf_launch, nmf_plan, nmf_scratch_bytes,
                          pcen, pcen_audio, pcen_coefficient, pcen_decay, pcen_launch, pcen_plan, pcen_scratch_bytes,
                          onset_backtrack, onset_detect, onset_detect_audio, peak_launch, peak_pick, peak_plan, peak_scratch_bytes,
                          beat_sync_audio, stack_memory, stack_memory_launch, sync, sync_launch, sync_plan,
                          delta, delta_launch, delta_weights, mfcc, mfcc_audio, mfcc_kernel_name, mfcc_launch, mfcc_plan, mfcc_table, mfcc_to_mel_db,
                          fft_frequencies, spectral_bandwidth, spectral_centroid, spectral_crest, spectral_flatness, spectral_rolloff, spectral_shape,
                          spectral_shape_audio, spectral_shape_kernel_name, spectral_shape_launch, spectral_shape_plan)

__all__ = ["Spectrogram", "SpectrogramDisplay", "CColorPalette", "Plan", "stft_db", "colormap", "window", "colormap_lut",
           "colormap_range", "feed_samples", "memsize_blocks", "next_power_of_2", "JsgError", "capi",
           "Filterbank", "stft_fb_db", "stft_fb_db_strided", "stft_fb_kernel_name", "fb_band_plan", "mel_spectrogram_db", "FreqAxis", "colormap_axis",
           "CStftPlan", "cstft", "istft_launch", "istft_nola", "istft_scratch_floats", "stft", "istft",
           "pvoc_frames", "phase_vocoder_launch", "phase_vocoder", "time_stretch",
           "hpss_scratch_bytes", "hpss_launch", "hpss", "hpss_audio",
           "sinc_table", "Resampler", "resample_length", "resample_launch", "resample_kernel_name", "resample_plan", "resample", "pitch_shift",
           "CqtBasis", "cqt_frames", "cqt_launch", "cqt_plan", "cqt_kernel_name", "cqt", "vqt", "cqt_frequencies", "cqt_db",
           "yin_frames", "yin_launch", "yin_plan", "yin_kernel_name", "yin", "yin_cmnd",
           "onset_strength", "onset_strength_launch", "tempogram", "tempogram_launch", "tempogram_frames", "tempogram_plan", "tempogram_kernel_name",
           "tempo_prior", "tempo_launch", "tempo", "estimate_tempo",
           "capix", "beat_log_table", "beat_scratch_bytes", "beat_launch", "beat_plan", "beat_track", "beat_track_audio",
           "cdist", "cdist_launch", "cdist_plan", "dtw", "dtw_launch", "dtw_scratch_bytes", "dtw_plan",
           "viterbi_scratch_bytes", "viterbi_launch", "viterbi_plan", "viterbi_band_transition", "viterbi",
           "pyin_prior", "pyin_tables", "pyin_observe_launch", "pyin_observe_plan", "pyin_decode_launch", "pyin_decode_scratch_bytes", "pyin_decode_plan", "pyin_geometry", "pyin",
           "knn", "knn_launch", "knn_scratch_bytes", "knn_plan", "knn_default_k", "recurrence_matrix", "cross_similarity", "recurrence_launch", "nn_filter", "nn_filter_launch",
           "rqa", "rqa_launch", "rqa_scratch_bytes", "rqa_plan",
           "diagonal_filter", "path_enhance_filters", "path_enhance", "path_enhance_launch", "path_enhance_plan", "recurrence_to_lag", "lag_to_recurrence", "lag_launch",
           "decompose", "nmf_launch", "nmf_scratch_bytes", "nmf_plan",
           "pcen", "pcen_audio", "pcen_coefficient", "pcen_decay", "pcen_launch", "pcen_scratch_bytes", "pcen_plan",
           "peak_launch", "peak_scratch_bytes", "peak_plan", "peak_pick", "onset_backtrack", "onset_detect", "onset_detect_audio",
           "sync", "sync_launch", "sync_plan", "stack_memory", "stack_memory_launch", "beat_sync_audio",
           "mfcc_table", "mfcc_launch", "mfcc_plan", "mfcc_kernel_name", "delta_weights", "delta_launch", "mfcc", "mfcc_to_mel_db", "delta", "mfcc_audio",
           "spectral_shape_launch", "spectral_shape_plan", "spectral_shape_kernel_name", "fft_frequencies", "spectral_shape", "spectral_centroid",
           "spectral_bandwidth", "spectral_rolloff", "spectral_flatness", "spectral_crest", "spectral_shape_audio"]
