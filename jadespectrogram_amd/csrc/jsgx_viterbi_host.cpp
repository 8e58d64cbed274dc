// libjsgx.so, Viterbi decoding (include/jsgx.h section 4): the refusals, the plan of a shape with the layout of the scratch, and the
// band transition builder, on the host and without a device.  The kernels and their launcher are in jsgx_viterbi.hip; the error text
// (jsgx::fail) is in jsgx_beat_host.cpp.  The span and overlap arithmetic is jsg_spans.h, a header without state that both libraries take.
#include <cmath>
#include <cstdint>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::i128;
}  // namespace

int viterbi_check(const jsgx_viterbi_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->log_emit) return fail(JSGX_ERR_INVALID, who, "null log_emit");
    if (!g->log_init) return fail(JSGX_ERR_INVALID, who, "null log_init");
    if (!g->trans) return fail(JSGX_ERR_INVALID, who, "null trans");
    if (!g->states) return fail(JSGX_ERR_INVALID, who, "null states");
    if (!jsg::aligned4(g->log_emit, g->log_init, g->trans, g->states, g->logp, g->value))
        return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->seqs < 1 || g->seqs > 65535) return fail(JSGX_ERR_INVALID, who, "seqs must be in 1..65535");
    if (g->n_states < 1 || g->n_states > JSGX_VITERBI_MAX_STATES) return fail(JSGX_ERR_INVALID, who, "n_states must be in 1..2048");
    if (g->n_frames < 1 || g->n_frames > JSGX_VITERBI_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..2^20");
    if (g->trans_form != JSGX_TRANS_DENSE && g->trans_form != JSGX_TRANS_BAND) return fail(JSGX_ERR_INVALID, who, "trans_form must be 0 (dense) or 1 (band)");
    if (g->trans_form == JSGX_TRANS_DENSE && g->band_half != 0) return fail(JSGX_ERR_INVALID, who, "band_half must be 0 with the dense form");
    if (g->band_half < 0 || g->band_half > JSGX_VITERBI_MAX_BAND_HALF) return fail(JSGX_ERR_INVALID, who, "band_half must be in 0..64");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    const long long S = g->n_states, T = g->n_frames, Q = g->seqs;
    const bool multi = Q > 1;
    if (g->emit_frame_pitch < S) return fail(JSGX_ERR_INVALID, who, "emit_frame_pitch smaller than n_states");
    if (multi && g->emit_seq_pitch < jsg::plane(T, g->emit_frame_pitch, S)) return fail(JSGX_ERR_INVALID, who, "emit_seq_pitch does not cover a sequence");
    if (g->trans_pitch < S) return fail(JSGX_ERR_INVALID, who, "trans_pitch smaller than n_states");
    if (multi && g->states_pitch < T) return fail(JSGX_ERR_INVALID, who, "states_pitch smaller than n_frames");
    if (g->value && g->value_frame_pitch < S) return fail(JSGX_ERR_INVALID, who, "value_frame_pitch smaller than n_states");
    if (g->value && multi && g->value_seq_pitch < jsg::plane(T, g->value_frame_pitch, S)) return fail(JSGX_ERR_INVALID, who, "value_seq_pitch does not cover a sequence");
    const long long trans_rows = g->trans_form == JSGX_TRANS_BAND ? 2 * g->band_half + 1 : S;
    const i128 in[3] = {jsg::addr(g->log_emit), jsg::addr(g->log_init), jsg::addr(g->trans)};
    const i128 in_bytes[3] = {jsg::span_bytes(Q, g->emit_seq_pitch, jsg::plane(T, g->emit_frame_pitch, S), 4), 4 * (i128)S,
                              4 * jsg::plane(trans_rows, g->trans_pitch, S)};
    const i128 out[3] = {jsg::addr(g->states), jsg::addr(g->logp), jsg::addr(g->value)};
    const i128 out_bytes[3] = {jsg::span_bytes(Q, g->states_pitch, T, 4), 4 * (i128)Q,
                               g->value ? jsg::span_bytes(Q, g->value_seq_pitch, jsg::plane(T, g->value_frame_pitch, S), 4) : 0};
    static const char* const what[3] = {"an output overlaps log_emit", "an output overlaps log_init", "an output overlaps trans"};
    for (int j = 0; j < 3; ++j)         // input by input, in the header's order
        for (int i = 0; i < 3; ++i)
            if (jsg::overlap(out[i], out_bytes[i], in[j], in_bytes[j])) return fail(JSGX_ERR_INVALID, who, what[j]);
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (jsg::overlap(out[i], out_bytes[i], out[j], out_bytes[j])) return fail(JSGX_ERR_INVALID, who, "an output overlaps another output");
    return JSGX_OK;
}

ViterbiPlan viterbi_plan(const jsgx_viterbi_args* g) {
    ViterbiPlan p{};
    const long long S = g->n_states, T = g->n_frames, Q = g->seqs, W = g->band_half;
    p.band = g->trans_form == JSGX_TRANS_BAND;
    const long long table_bytes = 4 * ((p.band ? 2 * W + 1 : S) * S + 2 * S);
    p.table_in_lds = p.band ? table_bytes <= JSGX_VITERBI_LDS_LIMIT : S <= JSGX_VITERBI_LDS_STATES;
    p.name = p.band ? (p.table_in_lds ? "viterbi_band_lds" : "viterbi_band_mem") : (p.table_in_lds ? "viterbi_dense_lds" : "viterbi_dense_mem");
    p.lds_bytes = (int)(p.table_in_lds ? table_bytes : 8 * S);
    p.G = 1;
    while (p.G < 64 && S * p.G * 2 <= JSGX_VITERBI_THREADS) p.G *= 2;
    const long long lanes = (S * p.G + 63) / 64 * 64;
    p.threads = (int)(lanes < JSGX_VITERBI_THREADS ? lanes : JSGX_VITERBI_THREADS);
    viterbi_layout(Q, S, T, &p);
    p.n_launches = p.n_blocks > 1 ? 4 : 3;
    return p;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int64_t jsgx_viterbi_scratch_bytes(const jsgx_viterbi_args* g) {
    const int rc = viterbi_check(g, "jsgx_viterbi_scratch_bytes");
    return rc != JSGX_OK ? rc : viterbi_plan(g).scratch_bytes;
}

int jsgx_viterbi_plan(const jsgx_viterbi_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches) {
    static const char* who = "jsgx_viterbi_plan";
    int rc = check_name_buffer(who, name, name_len, 24);
    if (rc == JSGX_OK) rc = viterbi_check(g, who);
    if (rc != JSGX_OK) return rc;
    const ViterbiPlan p = viterbi_plan(g);
    put_name(name, name_len, p.name);
    if (threads) *threads = p.threads;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (n_launches) *n_launches = p.n_launches;
    return JSGX_OK;
}

int jsgx_viterbi_band_build(int32_t n_states, int32_t band_half, const double* window, float* out, int64_t out_pitch) {
    static const char* who = "jsgx_viterbi_band_build";
    if (!window) return fail(JSGX_ERR_INVALID, who, "null window");
    if (!out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (n_states < 1 || n_states > JSGX_VITERBI_MAX_STATES) return fail(JSGX_ERR_INVALID, who, "n_states must be in 1..2048");
    if (band_half < 0 || band_half > JSGX_VITERBI_MAX_BAND_HALF) return fail(JSGX_ERR_INVALID, who, "band_half must be in 0..64");
    const int S = n_states, W = band_half;
    for (int k = 0; k <= 2 * W; ++k)
        if (!std::isfinite(window[k]) || window[k] < 0.0) return fail(JSGX_ERR_INVALID, who, "window entries must be finite and >= 0");
    if (!(window[W] > 0.0)) return fail(JSGX_ERR_INVALID, who, "window[band_half] must be > 0");
    if (out_pitch < S) return fail(JSGX_ERR_INVALID, who, "out_pitch smaller than n_states");
    const float minus_inf = -INFINITY;
    for (int r = 0; r <= 2 * W; ++r)
        for (int j = 0; j < S; ++j) out[r * out_pitch + j] = minus_inf;
    for (int i = 0; i < S; ++i) {
        const int lo = i - W > 0 ? i - W : 0, hi = i + W < S - 1 ? i + W : S - 1;
        double sum = 0.0;
        for (int j = lo; j <= hi; ++j) sum += window[j - i + W];
        for (int j = lo; j <= hi; ++j) {
            const double weight = window[j - i + W];
            out[(int64_t)(i - j + W) * out_pitch + j] = weight > 0.0 ? (float)std::log(weight / sum) : minus_inf;
        }
    }
    return JSGX_OK;
}

}  // extern "C"
