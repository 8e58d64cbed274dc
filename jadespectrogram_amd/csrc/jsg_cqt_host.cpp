// libjsg.so, the standard constant-Q / variable-Q basis of include/jsg.h section 2h, built on the host.  All arithmetic is double (this
// unit is compiled with contraction off); each tap component is rounded to float32 once.
#include <cmath>
#include <cstdint>
#include <vector>

#include "jsg_internal.h"

using namespace jsg;

extern "C" int jsg_cqt_basis_build(const jsg_cqt_spec* s, int32_t* half_len, int64_t* offset, float* centre_hz, float* taps, int64_t taps_cap,
                                   int64_t* n_taps) {
    static const char* who = "jsg_cqt_basis_build";
    if (!s || !n_taps) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    *n_taps = 0;
    if (!std::isfinite(s->fs) || !(s->fs > 0.0)) return jsg_fail_who(JSG_ERR_INVALID, who, "fs must be finite and > 0");
    if (!std::isfinite(s->fmin) || !(s->fmin > 0.0)) return jsg_fail_who(JSG_ERR_INVALID, who, "fmin must be finite and > 0");
    if (s->n_bins < 1 || s->n_bins > JSG_CQT_MAX_BINS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bins must be in 1..4096");
    if (s->bins_per_octave < 1 || s->bins_per_octave > 1200) return jsg_fail_who(JSG_ERR_INVALID, who, "bins_per_octave must be in 1..1200");
    if (!std::isfinite(s->filter_scale) || !(s->filter_scale > 0.0)) return jsg_fail_who(JSG_ERR_INVALID, who, "filter_scale must be finite and > 0");
    if (!std::isfinite(s->gamma) || s->gamma < 0.0) return jsg_fail_who(JSG_ERR_INVALID, who, "gamma must be finite and >= 0");
    const int K = s->n_bins;
    const double B = (double)s->bins_per_octave;
    const double r = std::exp2(1.0 / B);
    const double alpha = (r * r - 1.0) / (r * r + 1.0);
    const double Q = s->filter_scale / alpha;
    const double f_top = s->fmin * std::exp2((double)(K - 1) / B);
    if (!(f_top * (1.0 + alpha / 2.0) <= s->fs / 2.0)) return jsg_fail_who(JSG_ERR_INVALID, who, "the highest bin reaches past fs / 2");
    std::vector<double> len(K), freq(K);
    std::vector<int32_t> h(K);
    int64_t total = 0;
    for (int k = 0; k < K; ++k) {
        freq[k] = s->fmin * std::exp2((double)k / B);
        len[k] = Q * s->fs / (freq[k] + s->gamma / alpha);
        const double hk = std::floor(len[k] / 2.0);
        if (!(hk <= (double)JSG_CQT_MAX_HALF_LEN)) return jsg_fail_who(JSG_ERR_INVALID, who, "a bin is longer than 2 * 131072 + 1 taps");
        h[k] = (int32_t)hk;
        total += 2 * (int64_t)h[k] + 1;
    }
    if (total > JSG_CQT_MAX_TAPS) return jsg_fail_who(JSG_ERR_INVALID, who, "the basis has more than 2^24 taps");
    if (taps && taps_cap < total) return jsg_fail_who(JSG_ERR_INVALID, who, "taps_cap is smaller than the number of taps");
    *n_taps = total;
    const double pi = 3.14159265358979323846;
    int64_t at = 0;
    std::vector<double> g;
    for (int k = 0; k < K; ++k) {
        if (half_len) half_len[k] = h[k];
        if (offset) offset[k] = at;
        if (centre_hz) centre_hz[k] = (float)freq[k];
        const int hk = h[k], N = 2 * hk + 1;
        if (taps) {
            g.resize(N);
            double sum = 0.0;
            for (int i = 0; i < N; ++i) {
                g[i] = 0.5 + 0.5 * std::cos(pi * (double)(i - hk) / (double)(hk + 1));
                sum += g[i];
            }
            const double norm = (s->scale ? std::sqrt(len[k]) : 1.0) / sum;
            for (int i = 0; i < N; ++i) {
                const double u = freq[k] * (double)(i - hk) / s->fs;
                const double phi = 2.0 * pi * (u - std::floor(u));
                const double w = g[i] * norm;
                taps[2 * (at + i)] = (float)(w * std::cos(phi));
                taps[2 * (at + i) + 1] = (float)(-(w * std::sin(phi)));
            }
        }
        at += N;
    }
    return JSG_OK;
}
