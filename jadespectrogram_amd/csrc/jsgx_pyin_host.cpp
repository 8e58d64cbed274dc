// libjsgx.so, pYIN (include/jsgx.h section 5): the four table builders, the refusals of the two launches and their plans, on the host and
// without a device.  The kernels and their launchers are in jsgx_pyin.hip; the error text (jsgx::fail) is in jsgx_beat_host.cpp.
#include <cmath>
#include <cstdint>

#include "jsgx_internal.h"

// JSGX_PYIN_MAX_G is not defined in the product.  tools/pyin_bench.py builds the library with it at 64 ... 1: the rule of the first
// design (as many lanes per pitch bin as 1024 lanes hold) under that cap, for the comparison in profiles/pyin_bench.md that the
// product's rule comes from.

namespace jsgx {

namespace {
using jsg::i128;
constexpr int kSplitLanes = 512;        // bins are split among lanes only while the workgroup stays within this many lanes

// The continued fraction of the incomplete beta function (Lentz's method, the form of Numerical Recipes' betacf), in double.
double beta_fraction(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 10000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return h;
}

// I(x; a, b), the regularised incomplete beta function: the fraction on the side where it converges fast, the other by symmetry
double beta_cdf(double a, double b, double x) {
    if (x <= 0.0) return 0.0;
    if (x >= 1.0) return 1.0;
    const double front = std::exp(std::lgamma(a + b) - std::lgamma(a) - std::lgamma(b) + a * std::log(x) + b * std::log1p(-x));
    if (x < (a + 1.0) / (a + b + 2.0)) return front * beta_fraction(a, b, x) / a;
    return 1.0 - front * beta_fraction(b, a, 1.0 - x) / b;
}

// whether any of the outputs overlaps the input, input by input in the header's order; then output against output
template <int NI, int NO>
int check_overlaps(const char* who, const i128 (&in)[NI], const i128 (&in_bytes)[NI], const char* const (&what)[NI], const i128 (&out)[NO], const i128 (&out_bytes)[NO]) {
    for (int j = 0; j < NI; ++j)
        for (int i = 0; i < NO; ++i)
            if (jsg::overlap(out[i], out_bytes[i], in[j], in_bytes[j])) return fail(JSGX_ERR_INVALID, who, what[j]);
    for (int i = 0; i < NO; ++i)
        for (int j = i + 1; j < NO; ++j)
            if (jsg::overlap(out[i], out_bytes[i], out[j], out_bytes[j])) return fail(JSGX_ERR_INVALID, who, "an output overlaps another output");
    return JSGX_OK;
}
}  // namespace

int pyin_observe_check(const jsgx_pyin_observe_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->cmnd) return fail(JSGX_ERR_INVALID, who, "null cmnd");
    if (!g->prior) return fail(JSGX_ERR_INVALID, who, "null prior");
    if (!g->decay) return fail(JSGX_ERR_INVALID, who, "null decay");
    if (!g->norm) return fail(JSGX_ERR_INVALID, who, "null norm");
    if (!g->edges) return fail(JSGX_ERR_INVALID, who, "null edges");
    if (!g->log_emit) return fail(JSGX_ERR_INVALID, who, "null log_emit");
    if (!jsg::aligned4(g->cmnd, g->prior, g->decay, g->norm, g->edges, g->log_emit, g->obs, g->voiced_prob))
        return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->rows < 1 || g->rows > 65535) return fail(JSGX_ERR_INVALID, who, "rows must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames > JSGX_VITERBI_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..2^20");
    if (g->tau_max < 1 || g->tau_max > JSGX_PYIN_MAX_LAG) return fail(JSGX_ERR_INVALID, who, "tau_max must be in 1..4096");
    if (g->tau_min < 1 || g->tau_min > g->tau_max) return fail(JSGX_ERR_INVALID, who, "tau_min must be in 1..tau_max");
    if (g->n_thresholds < 1 || g->n_thresholds > JSGX_PYIN_MAX_THRESHOLDS) return fail(JSGX_ERR_INVALID, who, "n_thresholds must be in 1..256");
    if (g->n_bins < 1 || g->n_bins > JSGX_PYIN_MAX_BINS) return fail(JSGX_ERR_INVALID, who, "n_bins must be in 1..1024");
    const int most = pyin_max_troughs(g->tau_min, g->tau_max);
    if (g->boltz_len < (most > 1 ? most : 1) || g->boltz_len > JSGX_PYIN_MAX_LAG) return fail(JSGX_ERR_INVALID, who, "boltz_len must be in max(1, (tau_max - tau_min + 1) / 2)..4096");
    if (!(g->no_trough_prob >= 0.f && g->no_trough_prob <= 1.f)) return fail(JSGX_ERR_INVALID, who, "no_trough_prob must be in [0, 1]");
    const long long R = g->rows, T = g->n_frames, P = g->n_bins, lags = g->tau_max + 1;
    const bool multi = R > 1;
    if (g->cmnd_frame_pitch < lags) return fail(JSGX_ERR_INVALID, who, "cmnd_frame_pitch smaller than tau_max + 1");
    if (multi && g->cmnd_row_pitch < jsg::plane(T, g->cmnd_frame_pitch, lags)) return fail(JSGX_ERR_INVALID, who, "cmnd_row_pitch does not cover a row");
    if (g->emit_frame_pitch < 2 * P) return fail(JSGX_ERR_INVALID, who, "emit_frame_pitch smaller than 2 * n_bins");
    if (multi && g->emit_row_pitch < jsg::plane(T, g->emit_frame_pitch, 2 * P)) return fail(JSGX_ERR_INVALID, who, "emit_row_pitch does not cover a row");
    if (g->obs && g->obs_frame_pitch < P) return fail(JSGX_ERR_INVALID, who, "obs_frame_pitch smaller than n_bins");
    if (g->obs && multi && g->obs_row_pitch < jsg::plane(T, g->obs_frame_pitch, P)) return fail(JSGX_ERR_INVALID, who, "obs_row_pitch does not cover a row");
    if (g->voiced_prob && multi && g->voiced_pitch < T) return fail(JSGX_ERR_INVALID, who, "voiced_pitch smaller than n_frames");
    const i128 in[5] = {jsg::addr(g->cmnd), jsg::addr(g->prior), jsg::addr(g->decay), jsg::addr(g->norm), jsg::addr(g->edges)};
    const i128 in_bytes[5] = {jsg::span_bytes(R, g->cmnd_row_pitch, jsg::plane(T, g->cmnd_frame_pitch, lags), 4), 4 * (i128)g->n_thresholds, 4 * (i128)g->boltz_len,
                              4 * ((i128)g->boltz_len + 1), 4 * ((i128)P + 1)};
    static const char* const what[5] = {"an output overlaps cmnd", "an output overlaps prior", "an output overlaps decay", "an output overlaps norm", "an output overlaps edges"};
    const i128 out[3] = {jsg::addr(g->log_emit), jsg::addr(g->obs), jsg::addr(g->voiced_prob)};
    const i128 out_bytes[3] = {jsg::span_bytes(R, g->emit_row_pitch, jsg::plane(T, g->emit_frame_pitch, 2 * P), 4),
                               g->obs ? jsg::span_bytes(R, g->obs_row_pitch, jsg::plane(T, g->obs_frame_pitch, P), 4) : 0,
                               g->voiced_prob ? jsg::span_bytes(R, g->voiced_pitch, T, 4) : 0};
    return check_overlaps(who, in, in_bytes, what, out, out_bytes);
}

int pyin_decode_check(const jsgx_pyin_decode_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->log_emit) return fail(JSGX_ERR_INVALID, who, "null log_emit");
    if (!g->log_init) return fail(JSGX_ERR_INVALID, who, "null log_init");
    if (!g->log_window) return fail(JSGX_ERR_INVALID, who, "null log_window");
    if (!g->src_offset) return fail(JSGX_ERR_INVALID, who, "null src_offset");
    if (!g->log_switch) return fail(JSGX_ERR_INVALID, who, "null log_switch");
    if (!g->states) return fail(JSGX_ERR_INVALID, who, "null states");
    if (!jsg::aligned4(g->log_emit, g->log_init, g->log_window, g->src_offset, g->log_switch, g->states, g->logp, g->value))
        return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->seqs < 1 || g->seqs > 65535) return fail(JSGX_ERR_INVALID, who, "seqs must be in 1..65535");
    if (g->n_bins < 1 || g->n_bins > JSGX_PYIN_MAX_BINS) return fail(JSGX_ERR_INVALID, who, "n_bins must be in 1..1024");
    if (g->band_half < 0 || g->band_half > JSGX_PYIN_MAX_BAND_HALF) return fail(JSGX_ERR_INVALID, who, "band_half must be in 0..128");
    if (g->n_frames < 1 || g->n_frames > JSGX_VITERBI_MAX_FRAMES) return fail(JSGX_ERR_INVALID, who, "n_frames must be in 1..2^20");
    const long long Q = g->seqs, T = g->n_frames, P = g->n_bins, S = 2 * P;
    const bool multi = Q > 1;
    if (g->emit_frame_pitch < S) return fail(JSGX_ERR_INVALID, who, "emit_frame_pitch smaller than 2 * n_bins");
    if (multi && g->emit_seq_pitch < jsg::plane(T, g->emit_frame_pitch, S)) return fail(JSGX_ERR_INVALID, who, "emit_seq_pitch does not cover a sequence");
    if (multi && g->states_pitch < T) return fail(JSGX_ERR_INVALID, who, "states_pitch smaller than n_frames");
    if (g->value && g->value_frame_pitch < S) return fail(JSGX_ERR_INVALID, who, "value_frame_pitch smaller than 2 * n_bins");
    if (g->value && multi && g->value_seq_pitch < jsg::plane(T, g->value_frame_pitch, S)) return fail(JSGX_ERR_INVALID, who, "value_seq_pitch does not cover a sequence");
    const i128 in[5] = {jsg::addr(g->log_emit), jsg::addr(g->log_init), jsg::addr(g->log_window), jsg::addr(g->src_offset), jsg::addr(g->log_switch)};
    const i128 in_bytes[5] = {jsg::span_bytes(Q, g->emit_seq_pitch, jsg::plane(T, g->emit_frame_pitch, S), 4), 4 * (i128)S, 4 * (2 * (i128)g->band_half + 1), 4 * (i128)P, 16};
    static const char* const what[5] = {"an output overlaps log_emit", "an output overlaps log_init", "an output overlaps log_window", "an output overlaps src_offset",
                                        "an output overlaps log_switch"};
    const i128 out[3] = {jsg::addr(g->states), jsg::addr(g->logp), jsg::addr(g->value)};
    const i128 out_bytes[3] = {jsg::span_bytes(Q, g->states_pitch, T, 4), 4 * (i128)Q,
                               g->value ? jsg::span_bytes(Q, g->value_seq_pitch, jsg::plane(T, g->value_frame_pitch, S), 4) : 0};
    return check_overlaps(who, in, in_bytes, what, out, out_bytes);
}

PyinDecodePlan pyin_decode_plan(const jsgx_pyin_decode_args* g) {
    PyinDecodePlan p{};
    const long long P = g->n_bins, W = g->band_half;
    p.G = 1;
#ifdef JSGX_PYIN_MAX_G      // the first design's rule under a cap: tools/pyin_bench.py
    while (p.G < JSGX_PYIN_MAX_G && P * p.G * 2 <= JSGX_PYIN_THREADS) p.G *= 2;
#else                       // the rule of include/jsgx.h 5c, chosen by measurement (profiles/pyin_bench.md)
    while (p.G < 64 && 8 * (p.G * 2) <= 2 * W + 1 && P * p.G * 2 <= kSplitLanes) p.G *= 2;
#endif
    const long long lanes = (P * p.G + 63) / 64 * 64;
    p.threads = (int)(lanes < JSGX_PYIN_THREADS ? lanes : JSGX_PYIN_THREADS);
    p.lds_bytes = (int)(4 * (4 * (P + 2 * W) + 2 * W + 1));
    viterbi_layout(g->seqs, 2 * P, g->n_frames, &p.back);
    p.back.n_launches = p.back.n_blocks > 1 ? 4 : 3;
    p.back.name = "pyin_decode";
    return p;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int jsgx_pyin_prior_build(int32_t n_thresholds, double a, double b, float* out) {
    static const char* who = "jsgx_pyin_prior_build";
    if (!out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (n_thresholds < 1 || n_thresholds > JSGX_PYIN_MAX_THRESHOLDS) return fail(JSGX_ERR_INVALID, who, "n_thresholds must be in 1..256");
    if (!(std::isfinite(a) && a > 0.0 && std::isfinite(b) && b > 0.0)) return fail(JSGX_ERR_INVALID, who, "a and b must be finite and > 0");
    double below = 0.0;
    for (int k = 0; k < n_thresholds; ++k) {
        const double above = beta_cdf(a, b, (k + 1) / (double)n_thresholds);
        out[k] = (float)(above - below);
        below = above;
    }
    return JSGX_OK;
}

int jsgx_pyin_boltzmann_build(double lambda, int32_t n, float* decay, float* norm) {
    static const char* who = "jsgx_pyin_boltzmann_build";
    if (!decay) return fail(JSGX_ERR_INVALID, who, "null decay");
    if (!norm) return fail(JSGX_ERR_INVALID, who, "null norm");
    if (!(std::isfinite(lambda) && lambda > 0.0)) return fail(JSGX_ERR_INVALID, who, "lambda must be finite and > 0");
    if (n < 1 || n > JSGX_PYIN_MAX_LAG) return fail(JSGX_ERR_INVALID, who, "n must be in 1..4096");
    for (int i = 0; i < n; ++i) decay[i] = (float)std::exp(-lambda * i);
    norm[0] = 0.f;
    for (int m = 1; m <= n; ++m) norm[m] = (float)((1.0 - std::exp(-lambda)) / (1.0 - std::exp(-lambda * m)));
    return JSGX_OK;
}

int jsgx_pyin_bins_build(double sample_rate, double fmin, int32_t bins_per_semitone, int32_t n_bins, float* edges, float* freqs) {
    static const char* who = "jsgx_pyin_bins_build";
    if (!edges) return fail(JSGX_ERR_INVALID, who, "null edges");
    if (!freqs) return fail(JSGX_ERR_INVALID, who, "null freqs");
    if (!(std::isfinite(sample_rate) && sample_rate > 0.0)) return fail(JSGX_ERR_INVALID, who, "sample_rate must be finite and > 0");
    if (!(std::isfinite(fmin) && fmin > 0.0)) return fail(JSGX_ERR_INVALID, who, "fmin must be finite and > 0");
    if (bins_per_semitone < 1 || bins_per_semitone > 1024) return fail(JSGX_ERR_INVALID, who, "bins_per_semitone must be in 1..1024");
    if (n_bins < 1 || n_bins > JSGX_PYIN_MAX_BINS) return fail(JSGX_ERR_INVALID, who, "n_bins must be in 1..1024");
    const double per_octave = 12.0 * bins_per_semitone;
    for (int b = 0; b < n_bins; ++b) freqs[b] = (float)(fmin * std::exp2(b / per_octave));
    for (int b = 0; b <= n_bins; ++b) edges[b] = (float)(sample_rate / (fmin * std::exp2((b - 0.5) / per_octave)));
    return JSGX_OK;
}

int jsgx_pyin_transition_build(int32_t n_bins, int32_t band_half, const double* window, double switch_prob, float* log_window, float* src_offset, float* log_switch) {
    static const char* who = "jsgx_pyin_transition_build";
    if (!window) return fail(JSGX_ERR_INVALID, who, "null window");
    if (!log_window) return fail(JSGX_ERR_INVALID, who, "null log_window");
    if (!src_offset) return fail(JSGX_ERR_INVALID, who, "null src_offset");
    if (!log_switch) return fail(JSGX_ERR_INVALID, who, "null log_switch");
    if (n_bins < 1 || n_bins > JSGX_PYIN_MAX_BINS) return fail(JSGX_ERR_INVALID, who, "n_bins must be in 1..1024");
    if (band_half < 0 || band_half > JSGX_PYIN_MAX_BAND_HALF) return fail(JSGX_ERR_INVALID, who, "band_half must be in 0..128");
    const int P = n_bins, W = band_half;
    for (int k = 0; k <= 2 * W; ++k)
        if (!std::isfinite(window[k]) || window[k] < 0.0) return fail(JSGX_ERR_INVALID, who, "window entries must be finite and >= 0");
    if (!(window[W] > 0.0)) return fail(JSGX_ERR_INVALID, who, "window[band_half] must be > 0");
    if (!(switch_prob >= 0.0 && switch_prob <= 1.0)) return fail(JSGX_ERR_INVALID, who, "switch_prob must be in [0, 1]");
    const float minus_inf = -INFINITY;
    for (int k = 0; k <= 2 * W; ++k) log_window[k] = window[k] > 0.0 ? (float)std::log(window[k]) : minus_inf;
    for (int p = 0; p < P; ++p) {
        const int lo = p - W > 0 ? p - W : 0, hi = p + W < P - 1 ? p + W : P - 1;
        double sum = 0.0;
        for (int d = lo; d <= hi; ++d) sum += window[d - p + W];
        src_offset[p] = (float)-std::log(sum);
    }
    for (int u = 0; u < 2; ++u)
        for (int v = 0; v < 2; ++v) {
            const double pr = u == v ? 1.0 - switch_prob : switch_prob;
            log_switch[2 * u + v] = pr > 0.0 ? (float)std::log(pr) : minus_inf;
        }
    return JSGX_OK;
}

int jsgx_pyin_observe_plan(const jsgx_pyin_observe_args* g, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* frames_per_workgroup) {
    static const char* who = "jsgx_pyin_observe_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = pyin_observe_check(g, who);
    if (rc != JSGX_OK) return rc;
    put_name(name, name_len, "pyin_observe");
    if (threads) *threads = JSGX_PYIN_OBSERVE_THREADS;
    if (lds_bytes) *lds_bytes = pyin_observe_lds_bytes(g->tau_min, g->tau_max, g->n_bins);
    if (frames_per_workgroup) *frames_per_workgroup = 1;
    return JSGX_OK;
}

int64_t jsgx_pyin_decode_scratch_bytes(const jsgx_pyin_decode_args* g) {
    const int rc = pyin_decode_check(g, "jsgx_pyin_decode_scratch_bytes");
    return rc != JSGX_OK ? rc : pyin_decode_plan(g).back.scratch_bytes;
}

int jsgx_pyin_decode_plan(const jsgx_pyin_decode_args* g, char* name, int name_len, int32_t* lanes_per_bin, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches) {
    static const char* who = "jsgx_pyin_decode_plan";
    int rc = check_name_buffer(who, name, name_len, 16);
    if (rc == JSGX_OK) rc = pyin_decode_check(g, who);
    if (rc != JSGX_OK) return rc;
    const PyinDecodePlan p = pyin_decode_plan(g);
    put_name(name, name_len, p.back.name);
    if (lanes_per_bin) *lanes_per_bin = p.G;
    if (threads) *threads = p.threads;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    if (n_launches) *n_launches = p.back.n_launches;
    return JSGX_OK;
}

}  // extern "C"
