// libjsgx.so, beat tracking (include/jsgx.h section 1): the error text, the refusals, the scratch size, the plan of a period and the
// logarithm table, on the host and without a device.  The kernel and its launcher are in jsgx_beat.hip.  jsgx::fail lives here for
// all units; the span and overlap arithmetic is jsg_spans.h, a header without state that both libraries take.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
thread_local char g_error[192] = "";
}  // namespace

int fail(int code, const char* who, const char* what) {
    std::snprintf(g_error, sizeof g_error, "%s: %s", who, what);
    return code;
}

int beat_check(const jsgx_beat_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->in) return fail(JSGX_ERR_INVALID, who, "null in");
    if (!g->log_table) return fail(JSGX_ERR_INVALID, who, "null log_table");
    if (!g->beats) return fail(JSGX_ERR_INVALID, who, "null beats");
    if (!g->n_beats) return fail(JSGX_ERR_INVALID, who, "null n_beats");
    if (!jsg::aligned4(g->in, g->period, g->log_table, g->beats, g->n_beats, g->local_score, g->cum_score)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->rows < 1 || g->rows > 65535) return fail(JSGX_ERR_INVALID, who, "rows must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames > JSGX_BEAT_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..2^24");
    if (!g->period && (g->period_all < 1 || g->period_all > JSGX_BEAT_MAX_PERIOD)) return fail(JSGX_ERR_INVALID, who, "period_all must be in 1..1024 (period is null)");
    if (!std::isfinite(g->tightness) || !(g->tightness > 0.f)) return fail(JSGX_ERR_INVALID, who, "tightness must be finite and > 0");
    if (g->smooth != 0 && g->smooth != 1) return fail(JSGX_ERR_INVALID, who, "smooth must be 0 or 1");
    if (g->normalise != 0 && g->normalise != 1) return fail(JSGX_ERR_INVALID, who, "normalise must be 0 or 1");
    if (g->max_beats < 1 || g->max_beats > JSGX_BEAT_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "max_beats must be in 1..2^24");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    const bool multi = g->rows > 1;
    if (multi && g->in_pitch < g->n_frames) return fail(JSGX_ERR_INVALID, who, "in_pitch smaller than n_frames");
    if (multi && g->beats_pitch < g->max_beats) return fail(JSGX_ERR_INVALID, who, "beats_pitch smaller than max_beats");
    if (multi && g->local_score && g->local_pitch < g->n_frames) return fail(JSGX_ERR_INVALID, who, "local_pitch smaller than n_frames");
    if (multi && g->cum_score && g->cum_pitch < g->n_frames) return fail(JSGX_ERR_INVALID, who, "cum_pitch smaller than n_frames");
    const long long R = g->rows, T = g->n_frames;
    const i128 src[3] = {addr(g->in), addr(g->period), addr(g->log_table)};
    const i128 src_bytes[3] = {jsg::span_bytes(R, g->in_pitch, T, 4), 4 * (i128)R, 4 * (i128)(2 * JSGX_BEAT_MAX_PERIOD + 1)};
    const i128 dst[4] = {addr(g->beats), addr(g->n_beats), addr(g->local_score), addr(g->cum_score)};
    const i128 dst_bytes[4] = {jsg::span_bytes(R, g->beats_pitch, g->max_beats, 4), 4 * (i128)R, jsg::span_bytes(R, g->local_pitch, T, 4),
                               jsg::span_bytes(R, g->cum_pitch, T, 4)};
    static const char* const what[3] = {"an output overlaps in", "an output overlaps period", "an output overlaps log_table"};
    for (int j = 0; j < 3; ++j)         // input by input, in the header's order
        for (int i = 0; i < 4; ++i)
            if (jsg::overlap(src[j], src_bytes[j], dst[i], dst_bytes[i])) return fail(JSGX_ERR_INVALID, who, what[j]);
    return JSGX_OK;
}

int64_t beat_scratch_bytes(const jsgx_beat_args* g) { return 4ll * g->rows * g->n_frames * (g->smooth ? 2 : 1); }

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int jsgx_abi_version(void) { return JSGX_ABI_VERSION; }

const char* jsgx_last_error(void) { return g_error; }

int jsgx_log_table_build(int32_t n, float* out) {
    static const char* who = "jsgx_log_table_build";
    if (!out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (n < 1 || n > 2 * JSGX_BEAT_MAX_PERIOD + 1) return fail(JSGX_ERR_INVALID, who, "n must be in 1..2049");
    out[0] = 0.f;
    for (int k = 1; k < n; ++k) out[k] = (float)std::log((double)k);
    return JSGX_OK;
}

int64_t jsgx_beat_scratch_bytes(const jsgx_beat_args* g) {
    const int rc = beat_check(g, "jsgx_beat_scratch_bytes");
    return rc != JSGX_OK ? rc : beat_scratch_bytes(g);
}

int jsgx_beat_plan(const jsgx_beat_args* g, int32_t period, char* name, int name_len, int32_t* threads, int32_t* lds_bytes) {
    static const char* who = "jsgx_beat_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = beat_check(g, who);
    if (rc != JSGX_OK) return rc;
    if (period < 1 || period > JSGX_BEAT_MAX_PERIOD) return fail(JSGX_ERR_INVALID, who, "period must be in 1..1024");
    put_name(name, name_len, beat_form(period).G == 1 ? "beat_frames" : "beat_split");
    if (threads) *threads = JSGX_BEAT_THREADS;
    if (lds_bytes) *lds_bytes = JSGX_BEAT_LDS_BYTES;
    return JSGX_OK;
}

}  // extern "C"
