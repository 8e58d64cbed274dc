// libjsg.so, YIN fundamental-frequency tracking (include/jsg.h section 2i): the refusals, the frame count and the plan of a call, on
// the host and without a device.  The kernel and its launcher are in jsg_yin.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

namespace {
long long yin_frame_count(long long L, int w, int tau_max, long long hop) {
    const long long span = (long long)w + tau_max;
    return L >= span ? 1 + (L - span) / hop : 0;
}
}  // namespace

int yin_check(const jsg_yin_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->f0 && !g->aper && !g->cmnd) return jsg_fail_who(JSG_ERR_INVALID, who, "f0, aper and cmnd are all null");
    int rc = check_aligned4(who, g->in, g->f0, g->aper, g->cmnd);
    if (rc == JSG_OK) rc = check_rows(g->rows, who);
    if (rc != JSG_OK) return rc;
    if (g->in_samples < 1 || g->in_samples >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "in_samples must be in 1..2^31-1");
    if (g->window < 1 || g->window > JSG_YIN_MAX_WINDOW) return jsg_fail_who(JSG_ERR_INVALID, who, "window must be in 1..8192");
    if (g->tau_max < 1 || g->tau_max > JSG_YIN_MAX_LAG) return jsg_fail_who(JSG_ERR_INVALID, who, "tau_max must be in 1..8192");
    if (g->tau_min < 1 || g->tau_min > g->tau_max) return jsg_fail_who(JSG_ERR_INVALID, who, "tau_min must be in 1..tau_max");
    if (g->hop < 1 || g->hop > (1ll << 20)) return jsg_fail_who(JSG_ERR_INVALID, who, "hop must be in 1..2^20");
    const long long T = yin_frame_count(g->in_samples, g->window, g->tau_max, g->hop);
    if (g->n_frames < 1 || g->n_frames > T) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..jsg_yin_frames");
    if (g->chunk_frames < 0 || g->chunk_frames > 65536) return jsg_fail_who(JSG_ERR_INVALID, who, "chunk_frames must be 0 or in 1..65536");
    if (!std::isfinite(g->threshold) || !(g->threshold > 0.f)) return jsg_fail_who(JSG_ERR_INVALID, who, "threshold must be finite and > 0");
    if (!std::isfinite(g->sample_rate) || !(g->sample_rate > 0.f)) return jsg_fail_who(JSG_ERR_INVALID, who, "sample_rate must be finite and > 0");
    const bool multi = g->rows > 1;
    if (multi && g->in_pitch < g->in_samples) return jsg_fail_who(JSG_ERR_INVALID, who, "in_pitch smaller than in_samples");
    if (multi && (g->f0 || g->aper) && g->out_pitch < g->n_frames) return jsg_fail_who(JSG_ERR_INVALID, who, "out_pitch smaller than n_frames");
    const long long lags = (long long)g->tau_max + 1;
    if (g->cmnd && g->cmnd_frame_pitch < lags) return jsg_fail_who(JSG_ERR_INVALID, who, "cmnd_frame_pitch smaller than tau_max + 1");
    const i128 cmnd_plane = g->cmnd ? plane(g->n_frames, g->cmnd_frame_pitch, lags) : 0;
    if (multi && g->cmnd && (i128)g->cmnd_row_pitch < cmnd_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "cmnd_row_pitch smaller than (n_frames-1)*cmnd_frame_pitch + tau_max + 1");
    // an output that overlaps the input
    const i128 in_bytes = span_bytes(g->rows, g->in_pitch, g->in_samples, 4), line = span_bytes(g->rows, g->out_pitch, g->n_frames, 4);
    const void* out[3] = {g->f0, g->aper, g->cmnd};
    const i128 len[3] = {line, line, span_bytes(g->rows, g->cmnd_row_pitch, cmnd_plane, 4)};
    for (int i = 0; i < 3; ++i)
        if (overlap(addr(g->in), in_bytes, addr(out[i]), len[i])) return jsg_fail_who(JSG_ERR_INVALID, who, "an output overlaps in");
    return JSG_OK;
}

// NL by tau_max alone: the smallest of 1, 2, 4, 8 whose 64 NL lags of a wave cover tau_max, else 8.  S = min(hop, w + tau_max).  F is
// chunk_frames or kYinFrames, bounded by T and by the LDS: 40 KiB where one frame fits in it (four workgroups per compute unit, four
// waves per SIMD), else 80 KiB, else 160 KiB.  Where the library chooses, F is cut to a whole number of rounds of the four waves over
// the item's tiles (frames x blocks of 64 NL lags).  One frame needs at most 16384 + 1024 + 8193 floats, so 1 <= F and
// lds_floats <= kYinLdsOne always.
void yin_resolve(const jsg_yin_args* g, YinPlan* p) {
    const long long span = (long long)g->window + g->tau_max, row = (long long)g->tau_max + 1;
    p->NL = 1;
    while (p->NL < 8 && 64 * p->NL < g->tau_max) p->NL *= 2;
    p->S = (int)std::min<long long>(g->hop, span);
    const long long one = span + kYinPad + row;
    const long long budget = one <= kYinLdsFour ? kYinLdsFour : one <= kYinLdsTwo ? kYinLdsTwo : kYinLdsOne;
    long long F = g->chunk_frames ? g->chunk_frames : kYinFrames;
    F = std::min<long long>(F, g->n_frames);
    F = std::max<long long>(1, std::min<long long>(F, 1 + (budget - one) / (p->S + row)));
    const int blocks = (g->tau_max + 64 * p->NL - 1) / (64 * p->NL);
    const int round = blocks % 4 == 0 ? 1 : blocks % 2 == 0 ? 2 : 4;      // frames whose tiles fill the four waves evenly
    if (!g->chunk_frames && F > round) F = F / round * round;
    p->F = (int)F;
    p->chunks = (g->n_frames + F - 1) / F;
    p->lds_floats = (int)((F - 1) * (p->S + row) + one);
}

const char* yin_path_name(const YinPlan& p) { return p.NL == 1 ? "yin_lags1" : p.NL == 2 ? "yin_lags2" : p.NL == 4 ? "yin_lags4" : "yin_lags8"; }

}  // namespace jsg

using namespace jsg;

namespace {
// jsg_yin_plan (the name is optional) and jsg_yin_kernel_name (the name is all it gives)
int yin_plan_call(const char* who, const jsg_yin_args* g, char* name, int name_len, bool need_name, int32_t* frames_per_item, int32_t* lds_bytes) {
    int rc = check_name_buffer(who, name, name_len, need_name);
    if (rc == JSG_OK) rc = yin_check(g, who);
    if (rc != JSG_OK) return rc;
    YinPlan p{};
    yin_resolve(g, &p);
    put_path_name(name, name_len, yin_path_name(p));
    if (frames_per_item) *frames_per_item = p.F;
    if (lds_bytes) *lds_bytes = 4 * p.lds_floats;
    return JSG_OK;
}
}  // namespace

extern "C" {

int64_t jsg_yin_frames(int64_t in_samples, int32_t window, int32_t tau_max, int64_t hop) {
    static const char* who = "jsg_yin_frames";
    if (in_samples < 1 || in_samples >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "in_samples must be in 1..2^31-1");
    if (window < 1 || window > JSG_YIN_MAX_WINDOW) return jsg_fail_who(JSG_ERR_INVALID, who, "window must be in 1..8192");
    if (tau_max < 1 || tau_max > JSG_YIN_MAX_LAG) return jsg_fail_who(JSG_ERR_INVALID, who, "tau_max must be in 1..8192");
    if (hop < 1 || hop > (1ll << 20)) return jsg_fail_who(JSG_ERR_INVALID, who, "hop must be in 1..2^20");
    return yin_frame_count(in_samples, window, tau_max, hop);
}

int jsg_yin_plan(const jsg_yin_args* g, char* name, int name_len, int32_t* frames_per_item, int32_t* lds_bytes) {
    return yin_plan_call("jsg_yin_plan", g, name, name_len, false, frames_per_item, lds_bytes);
}

int jsg_yin_kernel_name(const jsg_yin_args* g, char* out, int out_len) { return yin_plan_call("jsg_yin_kernel_name", g, out, out_len, true, nullptr, nullptr); }

}  // extern "C"
