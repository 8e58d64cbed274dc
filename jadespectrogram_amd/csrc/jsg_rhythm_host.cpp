// libjsg.so, onset strength, autocorrelation tempogram and tempo (include/jsg.h section 2j): the refusals, the frame count, the plan of
// a tempogram call and the standard tempo prior, on the host and without a device.  The kernels and their launchers are in
// jsg_rhythm.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

int onset_check(const jsg_onset_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null out");
    int rc = check_aligned4(who, g->in, g->out);
    if (rc == JSG_OK) rc = check_rows(g->rows, who);
    if (rc != JSG_OK) return rc;
    if (g->n_bands < 1 || g->n_bands > JSG_ONSET_MAX_BANDS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bands must be in 1..65536");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (g->lag < 1 || g->lag > JSG_ONSET_MAX_LAG) return jsg_fail_who(JSG_ERR_INVALID, who, "lag must be in 1..4096");
    if (g->max_size < 1 || g->max_size > JSG_ONSET_MAX_SIZE) return jsg_fail_who(JSG_ERR_INVALID, who, "max_size must be in 1..255");
    if (g->frame_pitch < g->n_bands) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_pitch smaller than n_bands");
    const bool multi = g->rows > 1;
    const i128 in_plane = plane(g->n_frames, g->frame_pitch, g->n_bands);
    if (multi && (i128)g->row_pitch < in_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "row_pitch smaller than (n_frames-1)*frame_pitch + n_bands");
    if (multi && g->out_pitch < g->n_frames) return jsg_fail_who(JSG_ERR_INVALID, who, "out_pitch smaller than n_frames");
    if (overlap(addr(g->in), span_bytes(g->rows, g->row_pitch, in_plane, 4), addr(g->out), span_bytes(g->rows, g->out_pitch, g->n_frames, 4)))
        return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps in");
    return JSG_OK;
}

int tempogram_check(const jsg_tempogram_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->window) return jsg_fail_who(JSG_ERR_INVALID, who, "null window");
    if (!g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null out");
    int rc = check_aligned4(who, g->in, g->window, g->out);
    if (rc == JSG_OK) rc = check_rows(g->rows, who);
    if (rc != JSG_OK) return rc;
    if (g->n_in < 1 || g->n_in >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_in must be in 1..2^31-1");
    if (g->win_length < 2 || g->win_length > JSG_TEMPOGRAM_MAX_WINDOW) return jsg_fail_who(JSG_ERR_INVALID, who, "win_length must be in 2..4096");
    if (g->lags < 1 || g->lags > g->win_length) return jsg_fail_who(JSG_ERR_INVALID, who, "lags must be in 1..win_length");
    if (g->hop < 1 || g->hop > (1ll << 20)) return jsg_fail_who(JSG_ERR_INVALID, who, "hop must be in 1..2^20");
    if (g->n_frames < 1 || g->n_frames > 1 + (g->n_in - 1) / g->hop) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..jsg_tempogram_frames");
    if (g->normalise != 0 && g->normalise != 1) return jsg_fail_who(JSG_ERR_INVALID, who, "normalise must be 0 or 1");
    if (g->chunk_frames < 0 || g->chunk_frames > 65536) return jsg_fail_who(JSG_ERR_INVALID, who, "chunk_frames must be 0 or in 1..65536");
    const bool multi = g->rows > 1;
    if (multi && g->in_pitch < g->n_in) return jsg_fail_who(JSG_ERR_INVALID, who, "in_pitch smaller than n_in");
    if (g->frame_pitch < g->lags) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_pitch smaller than lags");
    const i128 out_plane = plane(g->n_frames, g->frame_pitch, g->lags);
    if (multi && (i128)g->row_pitch < out_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "row_pitch smaller than (n_frames-1)*frame_pitch + lags");
    const i128 out_bytes = span_bytes(g->rows, g->row_pitch, out_plane, 4);
    if (overlap(addr(g->in), span_bytes(g->rows, g->in_pitch, g->n_in, 4), addr(g->out), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps in");
    if (overlap(addr(g->window), 4 * (i128)g->win_length, addr(g->out), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps window");
    return JSG_OK;
}

// NL by lags alone: the smallest of 1, 2, 4, 8 whose 64 NL lags of a wave cover them, else 8.  S = min(hop, Wn).  F is chunk_frames or
// kTgFrames, bounded by n_frames and by the LDS: 40 KiB where one frame fits in it (four workgroups per compute unit), else 80 KiB,
// else 160 KiB.  Where the library chooses, F is cut to a whole number of rounds of the four waves over the item's tiles (frames x
// blocks of 64 NL lags).  One frame needs at most 3 * 4096 + 4096 + 64 floats, so 1 <= F and lds_floats <= kTgLdsOne always.
void tempogram_resolve(const jsg_tempogram_args* g, TgPlan* p) {
    const long long Wn = g->win_length, Lg = g->lags;
    p->NL = 1;
    while (p->NL < 8 && 64 * p->NL < Lg) p->NL *= 2;
    p->S = (int)std::min<long long>(g->hop, Wn);
    const long long Wp = (Wn + 3) / 4 * 4;          // a row of y
    const long long one = Wp + 2 * Wn + Lg + kTgPad, more = Wp + Lg + p->S;
    const long long budget = one <= kTgLdsFour ? kTgLdsFour : one <= kTgLdsTwo ? kTgLdsTwo : kTgLdsOne;
    long long F = g->chunk_frames ? g->chunk_frames : kTgFrames;
    F = std::min<long long>(F, g->n_frames);
    F = std::max<long long>(1, std::min<long long>(F, 1 + (budget - one) / more));
    const int blocks = (int)((Lg + 64 * p->NL - 1) / (64 * p->NL));
    const int round = blocks % 4 == 0 ? 1 : blocks % 2 == 0 ? 2 : 4;      // frames whose tiles fill the four waves evenly
    if (!g->chunk_frames && F > round) F = F / round * round;
    p->F = (int)F;
    p->chunks = (g->n_frames + F - 1) / F;
    p->lds_floats = (int)((F - 1) * more + one);
}

const char* tempogram_path_name(const TgPlan& p) {
    return p.NL == 1 ? "tempogram_lags1" : p.NL == 2 ? "tempogram_lags2" : p.NL == 4 ? "tempogram_lags4" : "tempogram_lags8";
}

int tempo_check(const jsg_tempo_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->prior) return jsg_fail_who(JSG_ERR_INVALID, who, "null prior");
    if (!g->bpm && !g->lag && !g->profile) return jsg_fail_who(JSG_ERR_INVALID, who, "bpm, lag and profile are all null");
    int rc = check_aligned4(who, g->in, g->prior, g->bpm, g->lag, g->profile);
    if (rc == JSG_OK) rc = check_rows(g->rows, who);
    if (rc != JSG_OK) return rc;
    if (g->lags < 2 || g->lags > JSG_TEMPOGRAM_MAX_WINDOW) return jsg_fail_who(JSG_ERR_INVALID, who, "lags must be in 2..4096");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (!std::isfinite(g->frame_rate) || !(g->frame_rate > 0.f)) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_rate must be finite and > 0");
    if (g->frame_pitch < g->lags) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_pitch smaller than lags");
    const bool multi = g->rows > 1;
    const i128 in_plane = plane(g->n_frames, g->frame_pitch, g->lags);
    if (multi && (i128)g->row_pitch < in_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "row_pitch smaller than (n_frames-1)*frame_pitch + lags");
    if (multi && g->profile && g->profile_pitch < g->lags) return jsg_fail_who(JSG_ERR_INVALID, who, "profile_pitch smaller than lags");
    const i128 src[2] = {addr(g->in), addr(g->prior)};
    const i128 src_bytes[2] = {span_bytes(g->rows, g->row_pitch, in_plane, 4), 4 * (i128)g->lags};
    const i128 dst[3] = {addr(g->bpm), addr(g->lag), addr(g->profile)};
    const i128 dst_bytes[3] = {4 * (i128)g->rows, 4 * (i128)g->rows, span_bytes(g->rows, g->profile_pitch, g->lags, 4)};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 2; ++j)
            if (overlap(src[j], src_bytes[j], dst[i], dst_bytes[i])) return jsg_fail_who(JSG_ERR_INVALID, who, j == 0 ? "an output overlaps in" : "an output overlaps prior");
    return JSG_OK;
}

}  // namespace jsg

using namespace jsg;

namespace {
// jsg_tempogram_plan (the name is optional) and jsg_tempogram_kernel_name (the name is all it gives)
int tempogram_plan_call(const char* who, const jsg_tempogram_args* g, char* name, int name_len, bool need_name, int32_t* frames_per_item, int32_t* lds_bytes) {
    int rc = check_name_buffer(who, name, name_len, need_name);
    if (rc == JSG_OK) rc = tempogram_check(g, who);
    if (rc != JSG_OK) return rc;
    TgPlan p{};
    tempogram_resolve(g, &p);
    put_path_name(name, name_len, tempogram_path_name(p));
    if (frames_per_item) *frames_per_item = p.F;
    if (lds_bytes) *lds_bytes = 4 * p.lds_floats;
    return JSG_OK;
}
}  // namespace

extern "C" {

int64_t jsg_tempogram_frames(int64_t n_in, int64_t hop) {
    static const char* who = "jsg_tempogram_frames";
    if (n_in < 1 || n_in >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_in must be in 1..2^31-1");
    if (hop < 1 || hop > (1ll << 20)) return jsg_fail_who(JSG_ERR_INVALID, who, "hop must be in 1..2^20");
    return 1 + (n_in - 1) / hop;
}

int jsg_tempogram_plan(const jsg_tempogram_args* g, char* name, int name_len, int32_t* frames_per_item, int32_t* lds_bytes) {
    return tempogram_plan_call("jsg_tempogram_plan", g, name, name_len, false, frames_per_item, lds_bytes);
}

int jsg_tempogram_kernel_name(const jsg_tempogram_args* g, char* out, int out_len) {
    return tempogram_plan_call("jsg_tempogram_kernel_name", g, out, out_len, true, nullptr, nullptr);
}

int jsg_tempo_prior_build(int32_t lags, double frame_rate, double start_bpm, double std_bpm, double max_bpm, float* out) {
    static const char* who = "jsg_tempo_prior_build";
    if (!out) return jsg_fail_who(JSG_ERR_INVALID, who, "null out");
    if (lags < 1 || lags > JSG_TEMPOGRAM_MAX_WINDOW) return jsg_fail_who(JSG_ERR_INVALID, who, "lags must be in 1..4096");
    if (!std::isfinite(frame_rate) || !(frame_rate > 0)) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_rate must be finite and > 0");
    if (!std::isfinite(start_bpm) || !(start_bpm > 0)) return jsg_fail_who(JSG_ERR_INVALID, who, "start_bpm must be finite and > 0");
    if (!std::isfinite(std_bpm) || !(std_bpm > 0)) return jsg_fail_who(JSG_ERR_INVALID, who, "std_bpm must be finite and > 0");
    if (!std::isfinite(max_bpm)) return jsg_fail_who(JSG_ERR_INVALID, who, "max_bpm must be finite");
    out[0] = 0.f;
    const double centre = std::log2(start_bpm);
    for (int tau = 1; tau < lags; ++tau) {
        const double bpm = 60.0 * frame_rate / tau;
        const double z = (std::log2(bpm) - centre) / std_bpm;
        out[tau] = max_bpm > 0 && bpm > max_bpm ? 0.f : (float)std::exp(-0.5 * (z * z));
    }
    return JSG_OK;
}

}  // extern "C"
