// libjsgx.so, what its units share (include/jsgx.h): the error text, the argument checks, the refusals that every unit words alike, the
// launchers' two ends and the float32 routines whose every operation the header states.  Of libjsg.so it takes two headers without
// state, jsg_spans.h (spans, overlap, alignment) and jsg_launch.h (OncePerDevice, launch_large_lds): the two libraries share that
// text, no object code and no state.  The first part needs no HIP header: plain g++ builds the host units for the sanitizer drivers.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "jsg_spans.h"
#include "jsgx.h"

#if defined(__HIPCC__)      // hipcc compiles the host unit as HIP too
#include <hip/hip_runtime.h>

#include "jsg_launch.h"
#define JSGX_HD __host__ __device__ __forceinline__
#else
#define JSGX_HD static inline
#include <cmath>
#endif

namespace jsgx {

// sets the calling thread's error text to "<who>: <what>" and returns code
int fail(int code, const char* who, const char* what);
// every refusal of jsgx_beat_launch that does not look at the scratch, in the header's order
int beat_check(const jsgx_beat_args* g, const char* who);
int64_t beat_scratch_bytes(const jsgx_beat_args* g);
// sections 2 and 3 (jsgx_dtw_host.cpp): every refusal that does not look at the scratch, in the header's order
int cdist_check(const jsgx_cdist_args* g, const char* who);
int dtw_check(const jsgx_dtw_args* g, const char* who);
int64_t dtw_scratch_bytes(const jsgx_dtw_args* g);
// section 4 (jsgx_viterbi_host.cpp): every refusal that does not look at the scratch, in the header's order
int viterbi_check(const jsgx_viterbi_args* g, const char* who);

// How the forward kernel of section 4 serves a shape (include/jsgx.h, "The kernels"), and where the parts of the scratch lie.
struct ViterbiPlan {
    const char* name;
    bool band, table_in_lds;
    int G, threads, lds_bytes;
    int n_blocks, n_launches;
    long long off_end, off_psi, off_jump;          // byte offsets in the scratch; V[T-1] is at 0
    long long scratch_bytes;
};
ViterbiPlan viterbi_plan(const jsgx_viterbi_args* g);
// The parts of the scratch behind V[T-1] for Q sequences of T frames and S states, and the blocks of the backtrace: what sections 4 and 5 share.
inline void viterbi_layout(long long Q, long long S, long long T, ViterbiPlan* p) {
    p->n_blocks = (int)((T + JSGX_VITERBI_BLOCK - 1) / JSGX_VITERBI_BLOCK);
    p->off_end = 4 * Q * S;
    p->off_psi = p->off_end + 4 * Q * p->n_blocks;
    p->off_jump = p->off_psi + 2 * Q * T * S;
    p->scratch_bytes = (p->off_jump + 2 * Q * p->n_blocks * S + 3) / 4 * 4;
}

// section 5 (jsgx_pyin_host.cpp): every refusal that does not look at the scratch, in the header's order
int pyin_observe_check(const jsgx_pyin_observe_args* g, const char* who);
int pyin_decode_check(const jsgx_pyin_decode_args* g, const char* who);
// The most troughs a frame can hold: no two lags next to each other are troughs and tau_max never is one.
inline int pyin_max_troughs(int tau_min, int tau_max) { return (tau_max - tau_min + 1) / 2; }
// The words of LDS of the observation kernel: d' of the frame, then lag, probability and bin of every trough, then obs.
inline int pyin_observe_lds_bytes(int tau_min, int tau_max, int P) { return 4 * (tau_max + 1 + 3 * (pyin_max_troughs(tau_min, tau_max) + 1) + P); }
// How the forward kernel of section 5 serves a shape: G lanes per pitch bin, and the scratch of section 4 with S = 2P (psi, jump, end, V[T-1]).
struct PyinDecodePlan {
    int G, threads, lds_bytes;
    ViterbiPlan back;
};
PyinDecodePlan pyin_decode_plan(const jsgx_pyin_decode_args* g);

// sections 6 to 8 (jsgx_knn_host.cpp): every refusal that does not look at the scratch, in the header's order
int knn_check(const jsgx_knn_args* g, const char* who);
int recurrence_check(const jsgx_recurrence_args* g, const char* who);
int nn_filter_check(const jsgx_nn_filter_args* g, const char* who);
// How section 6 serves a shape on a device of n_cu compute units: the column tiles, the workgroups S that share a strip (split = 0: the
// automatic rule; n_cu = 0: its largest answer, which is what the scratch is sized for), the dynamic LDS and the bytes of the partial lists.
struct KnnPlan {
    int tiles, S, lds_dynamic;
    long long scratch_bytes;
};
KnnPlan knn_plan(const jsgx_knn_args* g, int n_cu);

// section 9 (jsgx_rqa_host.cpp): every refusal that does not look at the scratch, in the header's order
int rqa_check(const jsgx_rqa_args* g, const char* who);
// Where the parts of the scratch of section 9 lie: the tiles' best cells at 0 (8 bytes a tile), the reversed paths behind them.
struct RqaScratch {
    long long tiles;               // of one pair
    long long off_paths, bytes;
};
RqaScratch rqa_scratch(const jsgx_rqa_args* g);

// sections 10 and 11 (jsgx_path_enhance_host.cpp): every refusal, in the header's order
int path_enhance_check(const jsgx_path_enhance_args* g, const char* who);
int lag_check(const jsgx_lag_args* g, const char* who);
// The staged window of section 10: its rows, and the words of a row (64 + 2 reach_j rounded up to 1 mod 4: eight rows, eight banks apart).
JSGX_HD int pe_window_rows(int reach_i) { return JSGX_PE_TILE + 2 * reach_i; }
JSGX_HD int pe_window_pitch(int reach_j) { return ((JSGX_PE_TILE + 2 * reach_j + 3) & ~3) + 1; }
JSGX_HD int pe_lds_bytes(int reach_i, int reach_j) { return 4 * pe_window_rows(reach_i) * pe_window_pitch(reach_j); }
// The planes of section 11: rows and columns of the input and of the output.
struct LagShape {
    int L, in_rows, in_cols, out_rows, out_cols;
};
JSGX_HD LagShape lag_shape(int n, int pad, int axis, int inverse) {
    LagShape s;
    s.L = pad ? 2 * n : n;
    const int lag_rows = axis == 1 ? s.L : n, lag_cols = axis == 1 ? n : s.L;
    s.in_rows = inverse ? lag_rows : n, s.in_cols = inverse ? lag_cols : n;
    s.out_rows = inverse ? n : lag_rows, s.out_cols = inverse ? n : lag_cols;
    return s;
}

// section 12 (jsgx_nmf_host.cpp): every refusal that does not look at the scratch, in the header's order, and the bytes of the planes;
// then the refusals of the scratch
struct NmfSpans {
    jsg::i128 v, a, c;
};
int nmf_check(const jsgx_nmf_args* g, const char* who, NmfSpans* spans);
int nmf_check_scratch(const jsgx_nmf_args* g, const char* who, const NmfSpans& spans, const void* scratch, int64_t scratch_bytes);
// Where the parts of the scratch of section 12 lie, in floats: G and G2 ([P][r][r] each), the chunks' partials of either Gram matrix
// ([P][chunks][r][r], the larger chunk count), the chunks' partials of N2 ([P][cT][r][K]).
struct NmfScratch {
    long long chunks_k, chunks_t, chunks_g;
    long long off_g2, off_gpart, off_n2part, bytes;
};
inline NmfScratch nmf_scratch(const jsgx_nmf_args* g) {
    NmfScratch s;
    const long long P = g->problems, r = g->n_components, K = g->n_bins;
    s.chunks_k = (K + JSGX_NMF_CHUNK_K - 1) / JSGX_NMF_CHUNK_K;
    s.chunks_t = ((long long)g->n_frames + JSGX_NMF_CHUNK_T - 1) / JSGX_NMF_CHUNK_T;
    s.chunks_g = g->update_components && s.chunks_t > s.chunks_k ? s.chunks_t : s.chunks_k;
    s.off_g2 = P * r * r;
    s.off_gpart = 2 * s.off_g2;
    s.off_n2part = s.off_gpart + P * s.chunks_g * r * r;
    s.bytes = 4 * (s.off_n2part + (g->update_components ? P * s.chunks_t * r * K : 0));
    return s;
}

// section 13 (jsgx_pcen_host.cpp): every refusal that does not look at the scratch, in the header's order, and the bytes of the buffers;
// then the refusals of the scratch
struct PcenSpans {
    jsg::i128 in, decay, state_in, out, smooth, state_out;
};
int pcen_check(const jsgx_pcen_args* g, const char* who, PcenSpans* spans);
int pcen_check_scratch(const jsgx_pcen_args* g, const char* who, const PcenSpans& spans, const void* scratch, int64_t scratch_bytes);
// How section 13 serves a shape: the chunks of a row, the chains (one lane each: a band of a chunk of a row), the launches and the bytes
// of the scratch ([rows][chunks][bands] floats: a chunk's last p, then the state that enters it; none where a row is one chunk).
struct PcenPlan {
    const char* name;
    long long chunks, chains;
    int launches;
    long long scratch_bytes;
};
inline PcenPlan pcen_plan(const jsgx_pcen_args* g) {
    PcenPlan p;
    p.chunks = ((long long)g->n_frames + JSGX_PCEN_CHUNK - 1) / JSGX_PCEN_CHUNK;
    p.chains = (long long)g->rows * p.chunks * g->n_bands;
    p.name = p.chunks == 1 ? "pcen_single" : "pcen_chunked";
    p.launches = p.chunks == 1 ? 1 : 3;
    p.scratch_bytes = p.chunks == 1 ? 0 : 4 * p.chains;
    return p;
}

// section 14 (jsgx_peak_host.cpp): every refusal that does not look at the scratch, in the header's order, and the bytes of the buffers;
// then the refusals of the scratch
struct PeakSpans {
    jsg::i128 in, energy, peaks, backtracked, n_peaks, candidate;
};
int peak_check(const jsgx_peak_args* g, const char* who, PeakSpans* spans);
int peak_check_scratch(const jsgx_peak_args* g, const char* who, const PeakSpans& spans, const void* scratch, int64_t scratch_bytes);
// What "peak_stats", "peak_row", "peak_cand" and "peak_carry" leave for a block of a row, 32 bytes: the row's minimum, maximum and
// non-finite vote (the block's own until "peak_row"), the block's last energy minimum (a frame, -1: none); the frame the chain enters
// the block at (the block's end: it does not), the peaks in front of the block and inside it, the last minimum in front of the block
struct PeakRecord {
    float mn, mx;
    int bad, block_min;
    int enter, run, count, carried_min;
};
static_assert(sizeof(PeakRecord) == 32, "include/jsgx.h states the bytes of a block's record");
// How section 14 serves a shape: the blocks of a row, the entering offsets of a block, and where the parts of the scratch lie (bytes):
// the records [rows][blocks] at 0, the words [rows][blocks][offsets] (count << 16 | last pick, as offsets in the block), the
// candidates [rows][blocks][B] as bytes
struct PeakPlan {
    const char* name;
    long long blocks, offsets;
    int launches;
    long long off_words, off_flags, scratch_bytes;
};
inline PeakPlan peak_plan(const jsgx_peak_args* g) {
    PeakPlan p;
    const long long B = JSGX_PEAK_BLOCK, R = g->rows;
    p.blocks = (g->n_frames + B - 1) / B;
    p.offsets = (long long)g->wait + 1 < B ? (long long)g->wait + 1 : B;
    const bool single = p.blocks == 1;
    p.name = single ? "peak_single" : "peak_blocked";
    p.launches = single ? 1 : 5;
    p.off_words = R * p.blocks * 32;
    p.off_flags = p.off_words + R * p.blocks * p.offsets * 4;
    p.scratch_bytes = single ? 0 : p.off_flags + R * p.blocks * B;
    return p;
}

// sections 15 and 16 (jsgx_sync_host.cpp): every refusal, in the header's order
int sync_check(const jsgx_sync_args* g, const char* who);
int stack_memory_check(const jsgx_stack_memory_args* g, const char* who);
// How section 15 serves a call: the aggregate's kernel, the most segments a pair can have (what the grid of "sync_aggregate" covers:
// strictly rising frames in 0..N, one fewer than the entries of s, and no more than the caller takes), the dynamic LDS and the launches
struct SyncPlan {
    const char* name;
    long long segments;
    int lds_dynamic, launches;
};
inline SyncPlan sync_plan(const jsgx_sync_args* g) {
    static const char* const names[4] = {"sync_mean", "sync_min", "sync_max", "sync_median"};
    SyncPlan p;
    p.name = names[g->aggregate];
    const long long entries = (long long)(g->n_bounds ? g->max_bounds : g->bounds_all) + 2 * g->pad;
    p.segments = entries - 1 < g->n_frames ? entries - 1 : g->n_frames;
    if (p.segments > g->max_segments) p.segments = g->max_segments;
    if (p.segments < 0) p.segments = 0;
    p.lds_dynamic = g->aggregate == JSGX_SYNC_MEDIAN ? JSGX_SYNC_LDS_TILE : 0;
    p.launches = p.segments > 0 ? 2 : 1;
    return p;
}
// The frames of the output a workgroup of section 16 takes: about 4096 elements, and few enough workgroups for one grid axis
inline int stack_frames_per_group(long long n_frames, long long width) {
    long long G = (4096 + width - 1) / width;
    const long long least = (n_frames + (1 << 23) - 1) >> 23;
    return (int)(G < least ? least : G);
}

// section 17 (jsgx_agglo_host.cpp): every refusal that does not look at the scratch, in the header's order, and the bytes of the
// buffers; then the refusals of the scratch
struct AggloSpans {
    jsg::i128 x, bounds, n_bounds, out_bounds, n_out, segments, n_segments, order, height;
};
int agglo_check(const jsgx_agglomerative_args* g, const char* who, AggloSpans* spans);
int agglo_check_scratch(const jsgx_agglomerative_args* g, const char* who, const AggloSpans& spans, const void* scratch, int64_t scratch_bytes);
// How section 17 serves a call: the stretches a pair can have (what the grids of the merge kernels cover, and what max_segments must
// cover), the longest of them, the form that takes it, and where the parts of the scratch lie (in 4-byte words): the plane of sums
// [pairs][N][F] at 0, the first costs as keys [pairs][N], the votes [pairs][votes], the offsets [pairs][stretches], the verdicts [pairs]
struct AggloPlan {
    const char* name;
    long long stretches, longest, votes;
    int threads, lds_bytes, launches;
    long long off_cost, off_votes, off_offsets, off_verdict, scratch_bytes;
};
JSGX_HD int agglo_group_lds(long long longest) { return (int)(8 * longest + 8 * ((longest + 63) / 64)); }
inline AggloPlan agglo_plan(const jsgx_agglomerative_args* g) {
    AggloPlan p;
    const long long P = g->pairs, N = g->n_frames, F = g->n_features;
    const long long entries = (long long)(g->n_bounds ? g->max_bounds : g->bounds_all) + 2 * g->pad;
    p.stretches = entries - 1 < N ? entries - 1 : N;
    if (p.stretches < 0) p.stretches = 0;
    p.longest = N < JSGX_AGGLO_MAX_STRETCH ? N : JSGX_AGGLO_MAX_STRETCH;
    const bool group = N > JSGX_AGGLO_SHORT;
    p.name = group ? "agglo_group" : "agglo_wave";
    p.threads = group ? JSGX_AGGLO_GROUP_THREADS : JSGX_AGGLO_THREADS;
    p.lds_bytes = group ? agglo_group_lds(p.longest) : JSGX_AGGLO_LDS_BYTES;
    p.launches = p.stretches == 0 ? 2 : group ? 5 : 4;
    p.votes = (N + JSGX_AGGLO_COPY_FRAMES - 1) / JSGX_AGGLO_COPY_FRAMES;
    p.off_cost = P * N * F;
    p.off_votes = p.off_cost + P * N;
    p.off_offsets = p.off_votes + P * p.votes;
    p.off_verdict = p.off_offsets + P * p.stretches;
    p.scratch_bytes = 4 * (p.off_verdict + P);
    return p;
}

// The three refusals of a launch's scratch buffer, in this order; `sizer` names the call that states `need`.
inline int check_scratch(const char* who, const void* scratch, int64_t scratch_bytes, int64_t need, const char* sizer) {
    if (!scratch) return fail(JSGX_ERR_INVALID, who, "null scratch");
    if (!jsg::aligned4(scratch)) return fail(JSGX_ERR_INVALID, who, "scratch must be 4-byte aligned");
    if (scratch_bytes >= need) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "scratch smaller than %s", sizer);
    return fail(JSGX_ERR_INVALID, who, what);
}

// One plane per pair, `rows` rows of `cols` elements of 4 bytes: its two refusals in the words every unit uses, "<name><row>_pitch smaller
// than <cols_name>" (row: "" or "_frame") and then "<name>_pair_pitch does not cover a plane", and its bytes for the overlap refusals.
inline int check_plane(const char* who, const char* name, const char* row, const char* cols_name, long long rows, long long cols, long long pitch,
                       long long pair_pitch, long long pairs, jsg::i128* bytes) {
    char what[96];
    const jsg::i128 one = jsg::plane(rows, pitch, cols);
    *bytes = jsg::span_bytes(pairs, pair_pitch, one, 4);
    if (pitch < cols)
        std::snprintf(what, sizeof what, "%s%s_pitch smaller than %s", name, row, cols_name);
    else if (pairs > 1 && pair_pitch < one)
        std::snprintf(what, sizeof what, "%s_pair_pitch does not cover a plane", name);
    else
        return JSGX_OK;
    return fail(JSGX_ERR_INVALID, who, what);
}
// Its sibling for a sequence of `frames` frames that the pairs may share (a pair pitch of 0), behind the refusal of its frame pitch.
inline int check_sequence(const char* who, const char* name, long long frames, long long K, long long frame_pitch, long long pair_pitch, long long pairs,
                          jsg::i128* bytes) {
    const jsg::i128 one = jsg::plane(frames, frame_pitch, K);
    *bytes = jsg::span_bytes(pairs, pair_pitch, one, 4);
    if (pair_pitch == 0 || pair_pitch >= one) return JSGX_OK;
    char what[96];
    std::snprintf(what, sizeof what, "%s_pair_pitch does not cover a sequence", name);
    return fail(JSGX_ERR_INVALID, who, what);
}
// x and y of sections 2 and 6, whose argument blocks name them alike: both frame pitches, then both pair pitches.
template <class Args>
int check_xy(const Args* g, const char* who, jsg::i128* x_bytes, jsg::i128* y_bytes) {
    if (g->x_frame_pitch < g->n_features) return fail(JSGX_ERR_INVALID, who, "x_frame_pitch smaller than n_features");
    if (g->y_frame_pitch < g->n_features) return fail(JSGX_ERR_INVALID, who, "y_frame_pitch smaller than n_features");
    const int rc = check_sequence(who, "x", g->n, g->n_features, g->x_frame_pitch, g->x_pair_pitch, g->pairs, x_bytes);
    return rc != JSGX_OK ? rc : check_sequence(who, "y", g->m, g->n_features, g->y_frame_pitch, g->y_pair_pitch, g->pairs, y_bytes);
}

// The two ends of a ..._plan call's name buffer: the refusal of one below min_len bytes, before any other (a call may pass none), and
// the kernel's name into it once the call has passed.
inline int check_name_buffer(const char* who, const char* buf, int len, int min_len) {
    return buf && len < min_len ? fail(JSGX_ERR_INVALID, who, "bad argument") : JSGX_OK;
}
inline void put_name(char* buf, int len, const char* name) {
    if (buf) std::strncpy(buf, name, len);
}

// The tiles of an n x m plane of section 3, down and across.  A launch takes one anti-diagonal of them.
struct DtwTiles {
    int i, j;
    int diagonals() const { return i + j - 1; }
};
inline DtwTiles dtw_tiles(int n, int m) { return {(n + JSGX_DTW_TILE_ROWS - 1) / JSGX_DTW_TILE_ROWS, (m + JSGX_DTW_TILE_COLS - 1) / JSGX_DTW_TILE_COLS}; }
// The tiles (ti, d - ti) of anti-diagonal d: ti in first..last.
struct TileRange {
    int first, last;
};
inline TileRange tiles_on_diagonal(const DtwTiles& t, int d) { return {d - (t.j - 1) > 0 ? d - (t.j - 1) : 0, d < t.i - 1 ? d : t.i - 1}; }
// The kernels a launch of section 3 or 9 enqueues: one per tile anti-diagonal, and the backtrace.
inline int tile_launches(int n, int m, bool backtrace) { return dtw_tiles(n, m).diagonals() + (backtrace ? 1 : 0); }
// What a ..._plan call of those sections writes, each where asked for.
inline void put_tiles_plan(int32_t* tile_rows, int32_t* tile_cols, int32_t* n_launches, int32_t* threads, int32_t* lds_bytes, int launches, int lanes, int lds) {
    if (tile_rows) *tile_rows = JSGX_DTW_TILE_ROWS;
    if (tile_cols) *tile_cols = JSGX_DTW_TILE_COLS;
    if (n_launches) *n_launches = launches;
    if (threads) *threads = lanes;
    if (lds_bytes) *lds_bytes = lds;
}

// The path outputs of sections 3 and 9, whose argument blocks name them alike: their refusals, each called at its place in the header's
// order (`what`: "max_path smaller than" the section's longest path), and the bytes of path_i and of path_j for the overlap refusals.
template <class Args>
int check_path_pointers(const Args* g, const char* who) {
    if (!g->path_i != !g->path_j) return fail(JSGX_ERR_INVALID, who, "path_i and path_j go together");
    return g->path_i && !g->path_len ? fail(JSGX_ERR_INVALID, who, "null path_len with paths") : JSGX_OK;
}
template <class Args>
int check_max_path(const Args* g, const char* who, long long longest, const char* what) {
    return g->path_i && g->max_path < longest ? fail(JSGX_ERR_INVALID, who, what) : JSGX_OK;
}
template <class Args>
int check_path_pitch(const Args* g, const char* who, jsg::i128* path_bytes) {
    *path_bytes = g->path_i ? jsg::span_bytes(g->pairs, g->path_pitch, g->max_path, 4) : 0;
    return g->pairs > 1 && g->path_i && g->path_pitch < g->max_path ? fail(JSGX_ERR_INVALID, who, "path_pitch smaller than max_path") : JSGX_OK;
}

#if defined(__HIPCC__)
// the device a launch goes to
inline int current_device(int* dev, const char* who) {
    return hipGetDevice(dev) == hipSuccess ? JSGX_OK : fail(JSGX_ERR_NO_DEVICE, who, "no HIP device");
}
// after the last launch of a call: what the launches left (hipGetLastError(), or what launch_large_lds returned), as the call's return code
inline int finish_launch(const char* who, hipError_t err) {
    if (err == hipSuccess) return JSGX_OK;
    char what[160];
    std::snprintf(what, sizeof what, "HIP error %d (%s)", (int)err, hipGetErrorString(err));
    return fail(JSGX_ERR_HIP, who, what);
}
// A pitched plane per pair as a kernel takes it: the pointer, the elements between its rows and between the pairs' planes.
template <class T>
struct Plane {
    T* p;
    long long pitch, pair_pitch;
    __device__ __forceinline__ T* row(long long pair, long long i) const { return p + pair * pair_pitch + i * pitch; }
};
// of a call's arguments: one pair has no pair pitch, whatever the field holds ...
template <class T>
Plane<T> plane_of(T* p, long long pitch, long long pair_pitch, int pairs) {
    return {p, pitch, pairs > 1 ? pair_pitch : 0};
}
// ... and a sequence's pair pitch is the caller's, 0 for one that every pair shares
template <class T>
Plane<T> sequence_of(T* p, long long frame_pitch, long long pair_pitch) {
    return {p, frame_pitch, pair_pitch};
}
// The blocked backtrace of section 4 (jsgx_viterbi.hip: jump where n_blocks > 1, ends, trace) onto the stream, from psi and V[T-1] in the
// scratch `base` laid out by viterbi_layout: what jsgx_viterbi_launch and jsgx_pyin_decode_launch enqueue behind their forward kernels.
// states_pitch is 0 for one sequence.  Returns hipGetLastError().
hipError_t viterbi_backtrace_enqueue(char* base, const ViterbiPlan& p, int seqs, int S, int T, int* states, long long states_pitch, float* logp, hipStream_t s);
#endif

constexpr int kBeatRing = 4096;                                 // >= 2 * JSGX_BEAT_MAX_PERIOD + JSGX_BEAT_THREADS, a power of two
constexpr int kBeatPen = 2 * JSGX_BEAT_MAX_PERIOD + 4;           // pen[tau], tau <= 2P
constexpr int kBeatG = JSGX_BEAT_MAX_PERIOD + 4;                 // g[k], k <= P

// a = (P + 1) / 2; G lanes per frame, F frames per step (include/jsgx.h, "The kernel")
struct BeatForm {
    int a, G, F;
};
JSGX_HD BeatForm beat_form(int P) {
    BeatForm f;
    f.a = (P + 1) / 2;
    f.G = 1;
    while (f.G < 64 && JSGX_BEAT_THREADS / f.G > f.a) f.G *= 2;
    f.F = JSGX_BEAT_THREADS / f.G < f.a ? JSGX_BEAT_THREADS / f.G : f.a;
    return f;
}

JSGX_HD float float_of_bits(unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(b);
#else
    float v;
    memcpy(&v, &b, 4);
    return v;
#endif
}

// E(x), the exponential as include/jsgx.h states it, operation by operation: jsgx_exp of section 1 carried to the whole line (section
// 13).  The scale 2^n, -126 <= n <= 128, goes on as two exact factors; for -87 <= x <= 0 the bits are those of the one product
JSGX_HD float exp_any(float x) {
    // straight-line: the arithmetic runs on an argument inside the range (itself wherever it lies inside), the three special answers
    // are selected behind it
    const float v = __builtin_fminf(__builtin_fmaxf(x, -87.0f), 88.72f);
    const float n = __builtin_floorf(__builtin_fmaf(v, 1.44269502162933349609375f, 0.5f));
    float r = __builtin_fmaf(n, -0.693145751953125f, v);
    r = __builtin_fmaf(n, -1.42860676533018704503775e-06f, r);
    float p = 1.984127011382952332496643e-04f;
    p = __builtin_fmaf(p, r, 1.388888922519981861114502e-03f);
    p = __builtin_fmaf(p, r, 8.333333767950534820556641e-03f);
    p = __builtin_fmaf(p, r, 4.166666790843009948730469e-02f);
    p = __builtin_fmaf(p, r, 1.666666716337203979492188e-01f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    const int ni = (int)n, half = ni >> 1;            // floor(n / 2)
    const float e = (p * float_of_bits((unsigned)(half + 127) << 23)) * float_of_bits((unsigned)(ni - half + 127) << 23);
    float out = x > 88.72f ? __builtin_inff() : e;          // one select each: no arm is an expression
    out = x < -87.0f ? 0.f : out;
    return x != x ? x : out;
}
// the name sections 1 and 7 call it by: their arguments are <= 0
JSGX_HD float exp_neg(float x) { return exp_any(x); }

JSGX_HD unsigned bits_of_float(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    unsigned b;
    memcpy(&b, &v, 4);
    return b;
#endif
}

// L(x), the natural logarithm as include/jsgx.h section 5 states it, operation by operation: plain float32 adds, multiplies and one
// correctly rounded divide, no fmaf and no hardware logarithm
JSGX_HD float log_pos(float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    // straight-line: the arithmetic runs on a positive finite argument (x itself wherever it is one), the special answers are selected
    // behind it
    const float x0 = x;
    const bool plain = x > 0.f && x < __builtin_inff();
    x = plain ? x : 1.0f;
    const bool tiny = x < 1.1754943508222875e-38f;           // below 2^-126: scaled by 2^24, exactly
    const float scaled = x * 16777216.0f;
    x = tiny ? scaled : x;
    int k = tiny ? -24 : 0;
    unsigned ix = bits_of_float(x) + (0x3f800000u - 0x3f3504f3u);
    k += (int)(ix >> 23) - 127;
    const float m = float_of_bits((ix & 0x007fffffu) + 0x3f3504f3u);        // x = m 2^k, sqrt(1/2) <= m < sqrt(2)
    const float f = m - 1.0f;
    const float s = f / (2.0f + f);
    const float z = s * s;
    const float w = z * z;
    const float t1 = w * (0xccce13.0p-25f + w * 0xf89e26.0p-26f);
    const float t2 = z * (0xaaaaaa.0p-24f + w * 0x91e9ee.0p-25f);
    const float r = t2 + t1;
    const float hfsq = (0.5f * f) * f;
    const float dk = (float)k;
    const float l = (((s * (hfsq + r) + dk * 9.0580006145e-06f) - hfsq) + f) + dk * 6.9313812256e-01f;
    float special = x0 == 0.f ? -__builtin_inff() : __builtin_nanf("");          // one select each: no arm is an expression
    special = x0 == __builtin_inff() ? x0 : special;
    return plain ? l : special;
}

}  // namespace jsgx
