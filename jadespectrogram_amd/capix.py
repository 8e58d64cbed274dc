"""ctypes binding of the companion C-ABI declared in include/jsgx.h (libjsgx.so: hand-written HIP for gfx950).

Plumbing only, as capi is for libjsg.so, and with NO CPU fallback: a missing library fails loudly, and without a usable MI355X the
launch returns JSGX_ERR_NO_DEVICE.  The two libraries share nothing but device memory.
"""
from __future__ import annotations

import ctypes as C
import os

from .capi import JsgError

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libjsgx.so")

JSGX_ABI_VERSION = 1
JSGX_OK = 0
JSGX_ERR_INVALID = -2
JSGX_ERR_HIP = -4
JSGX_ERR_NO_DEVICE = -5

BEAT_MAX_PERIOD, BEAT_MAX_FRAMES, BEAT_THREADS, BEAT_LDS_BYTES = 1024, 1 << 24, 256, 31008
BEAT_LOG_TABLE = 2 * BEAT_MAX_PERIOD + 1
EXP_REL_BOUND = 1.0e-7


class BeatArgs(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_pitch", C.c_int64), ("rows", C.c_int32), ("n_frames", C.c_int32), ("period", C.c_void_p),
                ("period_all", C.c_int32), ("smooth", C.c_int32), ("log_table", C.c_void_p), ("tightness", C.c_float), ("normalise", C.c_int32),
                ("beats", C.c_void_p), ("beats_pitch", C.c_int64), ("max_beats", C.c_int32), ("reserved0", C.c_int32), ("n_beats", C.c_void_p),
                ("local_score", C.c_void_p), ("local_pitch", C.c_int64), ("cum_score", C.c_void_p), ("cum_pitch", C.c_int64)]


METRIC_SQEUCLIDEAN, METRIC_EUCLIDEAN, METRIC_COSINE = 0, 1, 2
CDIST_MAX_FEATURES, DTW_MAX_LEN = 1024, 65536
CDIST_TILE, CDIST_THREADS, CDIST_LDS_BYTES = 64, 256, 17408
DTW_TILE_ROWS, DTW_TILE_COLS, DTW_THREADS, DTW_LDS_BYTES = 64, 64, 64, 16656


class CdistArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_frame_pitch", C.c_int64), ("x_pair_pitch", C.c_int64), ("y", C.c_void_p), ("y_frame_pitch", C.c_int64),
                ("y_pair_pitch", C.c_int64), ("pairs", C.c_int32), ("n_features", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("metric", C.c_int32),
                ("reserved0", C.c_int32), ("cost", C.c_void_p), ("cost_pitch", C.c_int64), ("cost_pair_pitch", C.c_int64)]


class DtwArgs(C.Structure):
    _fields_ = [("cost", C.c_void_p), ("cost_pitch", C.c_int64), ("cost_pair_pitch", C.c_int64), ("pairs", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("subseq", C.c_int32), ("band", C.c_int32), ("reserved0", C.c_int32), ("weights_mul", C.c_float * 3), ("weights_add", C.c_float * 3),
                ("acc", C.c_void_p), ("acc_pitch", C.c_int64), ("acc_pair_pitch", C.c_int64), ("path_i", C.c_void_p), ("path_j", C.c_void_p),
                ("path_pitch", C.c_int64), ("max_path", C.c_int32), ("path_len", C.c_void_p), ("total", C.c_void_p)]


TRANS_DENSE, TRANS_BAND = 0, 1
VITERBI_MAX_STATES, VITERBI_MAX_FRAMES, VITERBI_MAX_BAND_HALF = 2048, 1 << 20, 64
VITERBI_LDS_STATES, VITERBI_THREADS, VITERBI_LDS_LIMIT, VITERBI_BLOCK = 192, 1024, 163840, 256


class ViterbiArgs(C.Structure):
    _fields_ = [("log_emit", C.c_void_p), ("emit_frame_pitch", C.c_int64), ("emit_seq_pitch", C.c_int64), ("log_init", C.c_void_p), ("trans", C.c_void_p),
                ("trans_pitch", C.c_int64), ("trans_form", C.c_int32), ("band_half", C.c_int32), ("seqs", C.c_int32), ("n_states", C.c_int32),
                ("n_frames", C.c_int32), ("reserved0", C.c_int32), ("states", C.c_void_p), ("states_pitch", C.c_int64), ("logp", C.c_void_p),
                ("value", C.c_void_p), ("value_frame_pitch", C.c_int64), ("value_seq_pitch", C.c_int64)]


PYIN_MAX_BINS, PYIN_MAX_BAND_HALF, PYIN_MAX_THRESHOLDS, PYIN_MAX_LAG = 1024, 128, 256, 4096
PYIN_OBSERVE_THREADS, PYIN_THREADS = 64, 1024
LOG_ABS_BOUND = 1.0e-7


class PyinObserveArgs(C.Structure):
    _fields_ = [("cmnd", C.c_void_p), ("cmnd_frame_pitch", C.c_int64), ("cmnd_row_pitch", C.c_int64), ("rows", C.c_int32), ("n_frames", C.c_int32),
                ("tau_min", C.c_int32), ("tau_max", C.c_int32), ("prior", C.c_void_p), ("decay", C.c_void_p), ("norm", C.c_void_p), ("edges", C.c_void_p),
                ("n_thresholds", C.c_int32), ("boltz_len", C.c_int32), ("n_bins", C.c_int32), ("no_trough_prob", C.c_float), ("log_emit", C.c_void_p),
                ("emit_frame_pitch", C.c_int64), ("emit_row_pitch", C.c_int64), ("obs", C.c_void_p), ("obs_frame_pitch", C.c_int64), ("obs_row_pitch", C.c_int64),
                ("voiced_prob", C.c_void_p), ("voiced_pitch", C.c_int64)]


class PyinDecodeArgs(C.Structure):
    _fields_ = [("log_emit", C.c_void_p), ("emit_frame_pitch", C.c_int64), ("emit_seq_pitch", C.c_int64), ("log_init", C.c_void_p), ("log_window", C.c_void_p),
                ("src_offset", C.c_void_p), ("log_switch", C.c_void_p), ("n_bins", C.c_int32), ("band_half", C.c_int32), ("seqs", C.c_int32), ("n_frames", C.c_int32),
                ("states", C.c_void_p), ("states_pitch", C.c_int64), ("logp", C.c_void_p), ("value", C.c_void_p), ("value_frame_pitch", C.c_int64),
                ("value_seq_pitch", C.c_int64)]


KNN_MAX_K, KNN_MAX_SPLIT, KNN_STRIP, KNN_TILE, KNN_THREADS, KNN_LDS_STATIC, KNN_LDS_LIMIT, KNN_MERGE_THREADS = 256, 16, 64, 64, 256, 43776, 163840, 256
REC_CONNECTIVITY, REC_DISTANCE, REC_AFFINITY = 0, 1, 2
REC_THREADS, REC_CHUNK, REC_LDS_BYTES = 256, 4096, 18432
NNF_MAX_FEATURES, NNF_THREADS = 65536, 64


class KnnArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_frame_pitch", C.c_int64), ("x_pair_pitch", C.c_int64), ("y", C.c_void_p), ("y_frame_pitch", C.c_int64),
                ("y_pair_pitch", C.c_int64), ("pairs", C.c_int32), ("n_features", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("metric", C.c_int32),
                ("k", C.c_int32), ("width", C.c_int32), ("split", C.c_int32), ("nn_index", C.c_void_p), ("index_pitch", C.c_int64),
                ("index_pair_pitch", C.c_int64), ("nn_dist", C.c_void_p), ("dist_pitch", C.c_int64), ("dist_pair_pitch", C.c_int64)]


class RecurrenceArgs(C.Structure):
    _fields_ = [("nn_index", C.c_void_p), ("index_pitch", C.c_int64), ("index_pair_pitch", C.c_int64), ("nn_dist", C.c_void_p), ("dist_pitch", C.c_int64),
                ("dist_pair_pitch", C.c_int64), ("bandwidth", C.c_void_p), ("pairs", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("k", C.c_int32),
                ("mode", C.c_int32), ("sym", C.c_int32), ("diag", C.c_int32), ("reserved0", C.c_int32), ("out", C.c_void_p), ("out_pitch", C.c_int64),
                ("out_pair_pitch", C.c_int64)]


class NnFilterArgs(C.Structure):
    _fields_ = [("s", C.c_void_p), ("s_frame_pitch", C.c_int64), ("s_pair_pitch", C.c_int64), ("nn_index", C.c_void_p), ("index_pitch", C.c_int64),
                ("index_pair_pitch", C.c_int64), ("weights", C.c_void_p), ("weights_pitch", C.c_int64), ("weights_pair_pitch", C.c_int64), ("pairs", C.c_int32),
                ("n", C.c_int32), ("n_features", C.c_int32), ("k", C.c_int32), ("out", C.c_void_p), ("out_frame_pitch", C.c_int64), ("out_pair_pitch", C.c_int64)]


RQA_THREADS, RQA_LDS_BYTES, RQA_WINDOW = 64, 17408, 32


class RqaArgs(C.Structure):
    _fields_ = [("sim", C.c_void_p), ("sim_pitch", C.c_int64), ("sim_pair_pitch", C.c_int64), ("pairs", C.c_int32), ("n", C.c_int32), ("m", C.c_int32),
                ("knight", C.c_int32), ("gap_onset", C.c_float), ("gap_extend", C.c_float), ("reserved0", C.c_int32), ("max_path", C.c_int32),
                ("score", C.c_void_p), ("score_pitch", C.c_int64), ("score_pair_pitch", C.c_int64), ("step", C.c_void_p), ("step_pitch", C.c_int64),
                ("step_pair_pitch", C.c_int64), ("path_i", C.c_void_p), ("path_j", C.c_void_p), ("path_pitch", C.c_int64), ("path_len", C.c_void_p),
                ("end", C.c_void_p), ("total", C.c_void_p)]


PE_MAX_REACH, PE_MAX_FILTERS, PE_MAX_TAPS, PE_TILE, PE_THREADS, PE_LDS_LIMIT, PE_MIN_WINDOW, PE_MAX_WINDOW = 64, 32, 1 << 20, 64, 256, 163840, 3, 101
LAG_THREADS, LAG_TILE, LAG_LDS_BYTES = 256, 64, 32512


class PathEnhanceArgs(C.Structure):
    _fields_ = [("r", C.c_void_p), ("r_pitch", C.c_int64), ("r_pair_pitch", C.c_int64), ("tap_w", C.c_void_p), ("tap_at", C.c_void_p), ("filter_first", C.c_void_p),
                ("pairs", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("n_filters", C.c_int32), ("n_taps", C.c_int32), ("reach_i", C.c_int32),
                ("reach_j", C.c_int32), ("clip", C.c_int32), ("out", C.c_void_p), ("out_pitch", C.c_int64), ("out_pair_pitch", C.c_int64)]


class LagArgs(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_pitch", C.c_int64), ("in_pair_pitch", C.c_int64), ("pairs", C.c_int32), ("n", C.c_int32), ("pad", C.c_int32),
                ("axis", C.c_int32), ("inverse", C.c_int32), ("reserved0", C.c_int32), ("out", C.c_void_p), ("out_pitch", C.c_int64), ("out_pair_pitch", C.c_int64)]


NMF_MAX_COMPONENTS, NMF_MAX_BINS, NMF_MAX_FRAMES, NMF_MAX_ITER, NMF_CHUNK_K, NMF_CHUNK_T = 64, 16384, 1 << 24, 65536, 256, 256
NMF_FROBENIUS, NMF_EPSILON, NMF_THREADS, NMF_LDS_BYTES = 0, 2.0 ** -23, 256, 40960


class NmfArgs(C.Structure):
    _fields_ = [("v", C.c_void_p), ("v_pitch", C.c_int64), ("v_problem_pitch", C.c_int64), ("a", C.c_void_p), ("a_pitch", C.c_int64), ("a_problem_pitch", C.c_int64),
                ("c", C.c_void_p), ("c_pitch", C.c_int64), ("c_problem_pitch", C.c_int64), ("problems", C.c_int32), ("n_frames", C.c_int32), ("n_bins", C.c_int32),
                ("n_components", C.c_int32), ("n_iter", C.c_int32), ("update_components", C.c_int32), ("loss", C.c_int32), ("reserved0", C.c_int32)]


PCEN_CHUNK, PCEN_MAX_BANDS, PCEN_MAX_CHAINS, PCEN_THREADS = 256, 65536, 1 << 36, 256


class PcenArgs(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("frame_pitch", C.c_int64), ("row_pitch", C.c_int64), ("decay", C.c_void_p), ("state_in", C.c_void_p),
                ("state_in_pitch", C.c_int64), ("state_out", C.c_void_p), ("state_out_pitch", C.c_int64), ("smooth_out", C.c_void_p),
                ("smooth_frame_pitch", C.c_int64), ("smooth_row_pitch", C.c_int64), ("out", C.c_void_p), ("out_frame_pitch", C.c_int64),
                ("out_row_pitch", C.c_int64), ("rows", C.c_int32), ("n_bands", C.c_int32), ("n_frames", C.c_int32), ("b", C.c_float), ("gain", C.c_float),
                ("bias", C.c_float), ("power", C.c_float), ("eps", C.c_float)]


PEAK_BLOCK, PEAK_MAX_REACH, PEAK_MAX_FRAMES, PEAK_THREADS, PEAK_SHORT, PEAK_LDS_LIMIT = 1024, 256, 1 << 24, 256, 64, 163840
PEAK_LOG2_BLOCK = PEAK_BLOCK.bit_length() - 1
PEAK_LDS_BYTES = 2 * PEAK_BLOCK * PEAK_LOG2_BLOCK + 2 * (PEAK_BLOCK + 4) + 2 * PEAK_BLOCK


class PeakArgs(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("in_pitch", C.c_int64), ("energy", C.c_void_p), ("energy_pitch", C.c_int64), ("candidate", C.c_void_p),
                ("candidate_pitch", C.c_int64), ("peaks", C.c_void_p), ("backtracked", C.c_void_p), ("peaks_pitch", C.c_int64), ("n_peaks", C.c_void_p),
                ("rows", C.c_int32), ("n_frames", C.c_int32), ("pre_max", C.c_int32), ("post_max", C.c_int32), ("pre_avg", C.c_int32), ("post_avg", C.c_int32),
                ("delta", C.c_float), ("wait", C.c_int32), ("normalise", C.c_int32), ("max_peaks", C.c_int32)]


SYNC_MEAN, SYNC_MIN, SYNC_MAX, SYNC_MEDIAN = 0, 1, 2, 3
SYNC_CHUNK, SYNC_WAVE_MAX, SYNC_STAGE, SYNC_THREADS = 256, 64, 256, 256
SYNC_MAX_FRAMES, SYNC_MAX_FEATURES, SYNC_MAX_BOUNDS, SYNC_MAX_SEGMENTS = 1 << 24, 65536, 1 << 20, (1 << 20) + 1
SYNC_NAN_BITS, SYNC_LDS_BYTES, SYNC_LDS_TILE = 0x7FC00000, 4096, 65536
STACK_CONSTANT, STACK_EDGE, STACK_MAX_STEPS, STACK_MAX_DELAY, STACK_MAX_WIDTH, STACK_THREADS = 0, 1, 256, 1 << 24, 1 << 20, 256


class SyncArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_frame_pitch", C.c_int64), ("x_pair_pitch", C.c_int64), ("bounds", C.c_void_p), ("bounds_pitch", C.c_int64),
                ("n_bounds", C.c_void_p), ("segments", C.c_void_p), ("segments_pitch", C.c_int64), ("n_segments", C.c_void_p), ("out", C.c_void_p),
                ("out_frame_pitch", C.c_int64), ("out_pair_pitch", C.c_int64), ("pairs", C.c_int32), ("n_frames", C.c_int32), ("n_features", C.c_int32),
                ("max_bounds", C.c_int32), ("bounds_all", C.c_int32), ("max_segments", C.c_int32), ("aggregate", C.c_int32), ("pad", C.c_int32),
                ("reserved0", C.c_int32), ("reserved1", C.c_int32)]


class StackMemoryArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_frame_pitch", C.c_int64), ("x_pair_pitch", C.c_int64), ("out", C.c_void_p), ("out_frame_pitch", C.c_int64),
                ("out_pair_pitch", C.c_int64), ("pairs", C.c_int32), ("n_frames", C.c_int32), ("n_features", C.c_int32), ("n_steps", C.c_int32),
                ("delay", C.c_int32), ("mode", C.c_int32), ("fill", C.c_float), ("reserved0", C.c_int32)]


AGGLO_MAX_STRETCH, AGGLO_SHORT, AGGLO_THREADS, AGGLO_GROUP_THREADS, AGGLO_COPY_FRAMES, AGGLO_MAX_OUT = 16384, 64, 256, 64, 64, 1 << 24
AGGLO_LDS_BYTES, AGGLO_LDS_LIMIT = 2048, 133120


class AgglomerativeArgs(C.Structure):
    _fields_ = [("x", C.c_void_p), ("x_frame_pitch", C.c_int64), ("x_pair_pitch", C.c_int64), ("bounds", C.c_void_p), ("bounds_pitch", C.c_int64),
                ("n_bounds", C.c_void_p), ("segments", C.c_void_p), ("segments_pitch", C.c_int64), ("n_segments", C.c_void_p), ("out_bounds", C.c_void_p),
                ("out_pitch", C.c_int64), ("n_out", C.c_void_p), ("order", C.c_void_p), ("height", C.c_void_p), ("tree_pitch", C.c_int64), ("pairs", C.c_int32),
                ("n_frames", C.c_int32), ("n_features", C.c_int32), ("max_bounds", C.c_int32), ("bounds_all", C.c_int32), ("max_segments", C.c_int32),
                ("max_out", C.c_int32), ("n_clusters", C.c_int32), ("pad", C.c_int32), ("reserved0", C.c_int32)]


# every symbol include/jsgx.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SIGNATURES = {
    "jsgx_abi_version": (C.c_int, []),
    "jsgx_last_error": (C.c_char_p, []),
    "jsgx_log_table_build": (C.c_int, [C.c_int32, _P]),
    "jsgx_beat_scratch_bytes": (C.c_int64, [C.POINTER(BeatArgs)]),
    "jsgx_beat_launch": (C.c_int, [C.POINTER(BeatArgs), _P, C.c_int64, _P]),
    "jsgx_beat_plan": (C.c_int, [C.POINTER(BeatArgs), C.c_int32, C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "jsgx_cdist_launch": (C.c_int, [C.POINTER(CdistArgs), _P]),
    "jsgx_cdist_plan": (C.c_int, [C.POINTER(CdistArgs), C.c_char_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "jsgx_dtw_scratch_bytes": (C.c_int64, [C.POINTER(DtwArgs)]),
    "jsgx_dtw_launch": (C.c_int, [C.POINTER(DtwArgs), _P, C.c_int64, _P]),
    "jsgx_dtw_plan": (C.c_int, [C.POINTER(DtwArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 5),
    "jsgx_viterbi_scratch_bytes": (C.c_int64, [C.POINTER(ViterbiArgs)]),
    "jsgx_viterbi_launch": (C.c_int, [C.POINTER(ViterbiArgs), _P, C.c_int64, _P]),
    "jsgx_viterbi_plan": (C.c_int, [C.POINTER(ViterbiArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 3),
    "jsgx_viterbi_band_build": (C.c_int, [C.c_int32, C.c_int32, _P, _P, C.c_int64]),
    "jsgx_pyin_prior_build": (C.c_int, [C.c_int32, C.c_double, C.c_double, _P]),
    "jsgx_pyin_boltzmann_build": (C.c_int, [C.c_double, C.c_int32, _P, _P]),
    "jsgx_pyin_bins_build": (C.c_int, [C.c_double, C.c_double, C.c_int32, C.c_int32, _P, _P]),
    "jsgx_pyin_transition_build": (C.c_int, [C.c_int32, C.c_int32, _P, C.c_double, _P, _P, _P]),
    "jsgx_pyin_observe_launch": (C.c_int, [C.POINTER(PyinObserveArgs), _P]),
    "jsgx_pyin_observe_plan": (C.c_int, [C.POINTER(PyinObserveArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 3),
    "jsgx_pyin_decode_scratch_bytes": (C.c_int64, [C.POINTER(PyinDecodeArgs)]),
    "jsgx_pyin_decode_launch": (C.c_int, [C.POINTER(PyinDecodeArgs), _P, C.c_int64, _P]),
    "jsgx_pyin_decode_plan": (C.c_int, [C.POINTER(PyinDecodeArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 4),
    "jsgx_knn_scratch_bytes": (C.c_int64, [C.POINTER(KnnArgs)]),
    "jsgx_knn_launch": (C.c_int, [C.POINTER(KnnArgs), _P, C.c_int64, _P]),
    "jsgx_knn_plan": (C.c_int, [C.POINTER(KnnArgs), C.c_int32, C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 4),
    "jsgx_recurrence_launch": (C.c_int, [C.POINTER(RecurrenceArgs), _P]),
    "jsgx_nn_filter_launch": (C.c_int, [C.POINTER(NnFilterArgs), _P]),
    "jsgx_rqa_scratch_bytes": (C.c_int64, [C.POINTER(RqaArgs)]),
    "jsgx_rqa_launch": (C.c_int, [C.POINTER(RqaArgs), _P, C.c_int64, _P]),
    "jsgx_rqa_plan": (C.c_int, [C.POINTER(RqaArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 5),
    "jsgx_path_enhance_launch": (C.c_int, [C.POINTER(PathEnhanceArgs), _P]),
    "jsgx_path_enhance_plan": (C.c_int, [C.POINTER(PathEnhanceArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 4),
    "jsgx_diagonal_filter_table": (C.c_int, [_P, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _P, C.c_int64]),
    "jsgx_diagonal_filter_build": (C.c_int, [_P, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_double] + [C.POINTER(C.c_int32)] * 3 + [_P, _P, _P, C.c_int64]),
    "jsgx_lag_launch": (C.c_int, [C.POINTER(LagArgs), _P]),
    "jsgx_nmf_scratch_bytes": (C.c_int64, [C.POINTER(NmfArgs)]),
    "jsgx_nmf_launch": (C.c_int, [C.POINTER(NmfArgs), _P, C.c_int64, _P]),
    "jsgx_nmf_plan": (C.c_int, [C.POINTER(NmfArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 4),
    "jsgx_pcen_decay_build": (C.c_int, [C.c_float, _P]),
    "jsgx_pcen_scratch_bytes": (C.c_int64, [C.POINTER(PcenArgs)]),
    "jsgx_pcen_launch": (C.c_int, [C.POINTER(PcenArgs), _P, C.c_int64, _P]),
    "jsgx_pcen_plan": (C.c_int, [C.POINTER(PcenArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 4),
    "jsgx_peak_scratch_bytes": (C.c_int64, [C.POINTER(PeakArgs)]),
    "jsgx_peak_launch": (C.c_int, [C.POINTER(PeakArgs), _P, C.c_int64, _P]),
    "jsgx_peak_plan": (C.c_int, [C.POINTER(PeakArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 4),
    "jsgx_sync_launch": (C.c_int, [C.POINTER(SyncArgs), _P]),
    "jsgx_sync_plan": (C.c_int, [C.POINTER(SyncArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 3),
    "jsgx_stack_memory_launch": (C.c_int, [C.POINTER(StackMemoryArgs), _P]),
    "jsgx_agglomerative_scratch_bytes": (C.c_int64, [C.POINTER(AgglomerativeArgs)]),
    "jsgx_agglomerative_launch": (C.c_int, [C.POINTER(AgglomerativeArgs), _P, C.c_int64, _P]),
    "jsgx_agglomerative_plan": (C.c_int, [C.POINTER(AgglomerativeArgs), C.c_char_p, C.c_int] + [C.POINTER(C.c_int32)] * 3),
}

_lib = None


def lib() -> C.CDLL:
    """Load libjsgx.so (once).  Raises if the HIP extension has not been built -- no silent fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  jadespectrogram_amd has no CPU fallback.")
        # one HIP runtime per process: torch first, for the reason capi.lib() gives
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)   # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int) -> int:
    if rc < 0:
        msg = lib().jsgx_last_error()
        raise JsgError(rc, msg.decode() if msg else "")
    return rc
