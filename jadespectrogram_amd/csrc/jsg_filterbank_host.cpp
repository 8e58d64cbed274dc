// Filterbanks of the mel and log-frequency spectrograms: construction on the host (jsg_filterbank_build: double arithmetic, every
// weight rounded to float32 once) and the device object (jsg_filterbank_create / _create_matrix: the CSR uploaded once).  The band
// kernel and the launcher that applies a bank live in jsg_filterbank.hip; include/jsg.h (section 2b) states the semantics.
//
// The mel scales are those of librosa.filters.mel (htk = False: Slaney's Auditory Toolbox, htk = True: the HTK formula).  Positions
// are fractional bins, x = f * n / fs, so that a LINEAR bank of n/2+1 rows over [0, fs/2] is exactly the identity.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/jsg.h"
#include "jsg_internal.h"

using namespace jsg;

namespace {

struct Csr {
    std::vector<int> first, count, offset;
    std::vector<float> centre, w;
};

inline double hz_to_mel(double f, bool htk) {
    if (htk) return 2595.0 * std::log10(1.0 + f / 700.0);
    return slaney_hz_to_mel(f);
}
inline double mel_to_hz(double m, bool htk) {
    if (htk) return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    return slaney_mel_to_hz(m);
}

int check_spec(const jsg_fb_spec* s) {
    if (!s) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: null spec");
    if (!fft_size_supported(s->n)) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: n must be a power of two in 512..8192");
    if (!(s->fs > 0.f) || !std::isfinite(s->fs)) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: fs must be > 0");
    if (s->n_bands < 1 || s->n_bands > JSG_FB_MAX_BANDS) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: n_bands must be in 1..8192");
    if (!(s->fmin >= 0.f)) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: fmin must be >= 0");
    if (!(double(s->fmax) <= 0.5 * double(s->fs))) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: fmax must be <= fs/2");
    if (!(s->fmin < s->fmax)) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: fmin must be < fmax");
    if (s->scale < JSG_FB_MEL_SLANEY || s->scale > JSG_FB_LINEAR) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: unknown scale");
    if (s->norm < JSG_FB_NORM_NONE || s->norm > JSG_FB_NORM_UNIT_SUM) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: unknown norm");
    if ((s->scale == JSG_FB_LOG || s->scale == JSG_FB_LINEAR) && s->n_bands < 2)
        return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: LOG / LINEAR banks need at least two bands");
    if (s->scale == JSG_FB_LOG && !(s->fmin > 0.f)) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank: a LOG bank needs fmin > 0");
    return JSG_OK;
}

// band b = the triangle (lo, c, hi) in bins; NORM_SLANEY scales it by slaney (2 / (hi - lo) in Hz, computed by the caller)
void add_band(Csr& m, int H, double lo, double c, double hi, double centre_hz, int norm, double slaney) {
    std::vector<double> v;
    const int k0 = std::max(0, int(std::ceil(lo))), k1 = std::min(H - 1, int(std::floor(hi)));
    for (int k = k0; k <= k1; ++k) {
        const double up = (double(k) - lo) / (c - lo), down = (hi - double(k)) / (hi - c);
        v.push_back(std::max(0.0, std::min(up, down)));
    }
    double scale = 1.0;
    if (norm == JSG_FB_NORM_SLANEY) scale = slaney;
    if (norm == JSG_FB_NORM_UNIT_SUM) {
        double sum = 0.0;
        for (double x : v) sum += x;
        if (sum > 0.0) scale = 1.0 / sum;
    }
    std::vector<float> f(v.size());
    for (size_t i = 0; i < v.size(); ++i) f[i] = float(v[i] * scale);   // the one rounding of every weight
    size_t a = 0, e = f.size();
    while (a < e && f[a] == 0.0f) ++a;
    while (e > a && f[e - 1] == 0.0f) --e;
    m.first.push_back(a < e ? k0 + int(a) : 0);
    m.count.push_back(int(e - a));
    m.offset.push_back(int(m.w.size()));
    m.centre.push_back(float(centre_hz));
    m.w.insert(m.w.end(), f.begin() + a, f.begin() + e);
}

void build_csr(const jsg_fb_spec* s, Csr& m) {
    const int B = s->n_bands, H = s->n / 2 + 1;
    const double fs = s->fs, n = s->n, fmin = s->fmin, fmax = s->fmax;
    auto bins = [&](double hz) { return hz * n / fs; };
    if (s->scale == JSG_FB_MEL_SLANEY || s->scale == JSG_FB_MEL_HTK) {
        const bool htk = s->scale == JSG_FB_MEL_HTK;
        const double m0 = hz_to_mel(fmin, htk), m1 = hz_to_mel(fmax, htk);
        std::vector<double> hz(B + 2);
        const double step = (m1 - m0) / double(B + 1);   // numpy.linspace(m0, m1, B + 2)
        for (int i = 0; i < B + 2; ++i) hz[i] = mel_to_hz(i == B + 1 ? m1 : m0 + double(i) * step, htk);
        for (int b = 0; b < B; ++b)
            add_band(m, H, bins(hz[b]), bins(hz[b + 1]), bins(hz[b + 2]), hz[b + 1], s->norm, 2.0 / (hz[b + 2] - hz[b]));
        return;
    }
    // LOG / LINEAR: centres c_b, b = -1 .. B (the outer two extend the progression)
    const bool geo = s->scale == JSG_FB_LOG;
    const double r = geo ? std::pow(fmax / fmin, 1.0 / double(B - 1)) : 0.0, d = geo ? 0.0 : (fmax - fmin) / double(B - 1);
    auto centre = [&](int b) { return geo ? fmin * std::pow(r, double(b)) : fmin + double(b) * d; };
    for (int b = 0; b < B; ++b) {
        const double c = bins(centre(b));
        const double lo = std::min(bins(centre(b - 1)), c - 1.0), hi = std::max(bins(centre(b + 1)), c + 1.0);
        add_band(m, H, lo, c, hi, centre(b), s->norm, 2.0 / ((hi - lo) * fs / n));
    }
}

int upload(jsg_filterbank** out, int n, Csr& m) {
    static const char* who = "jsg_filterbank_create";
    *out = nullptr;
    std::unique_ptr<jsg_filterbank> fb(new (std::nothrow) jsg_filterbank());
    if (!fb) return jsg_fail_who(JSG_ERR_NOMEM, who, "out of host memory");
    fb->n = n;
    fb->n_bands = int(m.first.size());
    fb->nnz = (long long)m.w.size();
    const size_t B = size_t(fb->n_bands);
    std::vector<int> blob(3 * B + m.w.size());
    std::memcpy(blob.data(), m.first.data(), B * 4);
    std::memcpy(blob.data() + B, m.count.data(), B * 4);
    std::memcpy(blob.data() + 2 * B, m.offset.data(), B * 4);
    if (!m.w.empty()) std::memcpy(blob.data() + 3 * B, m.w.data(), m.w.size() * 4);
    const int rc = fb->blob.upload(blob.data(), blob.size() * 4, who);
    if (rc != JSG_OK) return rc;
    fb->d_desc = static_cast<const int*>(fb->blob.data());
    fb->d_w = reinterpret_cast<const float*>(fb->d_desc + 3 * B);
    fb->first = std::move(m.first);
    fb->count = std::move(m.count);
    fb->offset = std::move(m.offset);
    fb->w = std::move(m.w);
    *out = fb.release();
    return JSG_OK;
}

}  // namespace

extern "C" {

int jsg_filterbank_build(const jsg_fb_spec* s, int32_t* first_bin, int32_t* n_bins, int32_t* offset, float* centre_hz, float* weights,
                         int64_t weights_cap, int64_t* nnz) {
    int rc = check_spec(s);
    if (rc != JSG_OK) return rc;
    if (!nnz) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_build: null nnz");
    Csr m;
    build_csr(s, m);
    *nnz = (int64_t)m.w.size();
    if (!weights) return JSG_OK;
    if (!first_bin || !n_bins || !offset || !centre_hz) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_build: null output array");
    if (weights_cap < *nnz) return jsg_fail(JSG_ERR_SIZE_MISMATCH, "jsg_filterbank_build: weights_cap < nnz");
    const size_t B = m.first.size();
    std::memcpy(first_bin, m.first.data(), B * 4);
    std::memcpy(n_bins, m.count.data(), B * 4);
    std::memcpy(offset, m.offset.data(), B * 4);
    std::memcpy(centre_hz, m.centre.data(), B * 4);
    if (!m.w.empty()) std::memcpy(weights, m.w.data(), m.w.size() * 4);
    return JSG_OK;
}

int jsg_filterbank_create(jsg_filterbank** out, const jsg_fb_spec* s) {
    if (!out) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_create: null argument");
    *out = nullptr;
    int rc = check_spec(s);
    if (rc != JSG_OK) return rc;
    Csr m;
    build_csr(s, m);
    return upload(out, s->n, m);
}

int jsg_filterbank_create_matrix(jsg_filterbank** out, int n, int n_bands, const float* w) {
    if (!out || !w) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_create_matrix: null argument");
    *out = nullptr;
    if (!fft_size_supported(n) || n_bands < 1 || n_bands > JSG_FB_MAX_BANDS)
        return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_create_matrix: n must be a power of two in 512..8192, n_bands in 1..8192");
    const int H = n / 2 + 1;
    Csr m;
    for (int b = 0; b < n_bands; ++b) {
        const float* row = w + (size_t)b * H;
        int a = 0, e = H;
        for (int k = 0; k < H; ++k)
            if (!std::isfinite(row[k])) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_create_matrix: weights must be finite");
        while (a < e && row[a] == 0.0f) ++a;
        while (e > a && row[e - 1] == 0.0f) --e;
        m.first.push_back(a < e ? a : 0);
        m.count.push_back(e - a);
        m.offset.push_back(int(m.w.size()));
        m.w.insert(m.w.end(), row + a, row + e);
    }
    if (m.w.size() > size_t(INT32_MAX)) return jsg_fail(JSG_ERR_UNSUPPORTED, "jsg_filterbank_create_matrix: more than 2^31 weights");
    return upload(out, n, m);
}

int jsg_filterbank_destroy(jsg_filterbank* fb) {
    delete fb;
    return JSG_OK;
}

int jsg_filterbank_bands(const jsg_filterbank* fb) { return fb ? fb->n_bands : jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_bands: null"); }
int jsg_filterbank_fft_size(const jsg_filterbank* fb) { return fb ? fb->n : jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_fft_size: null"); }

int jsg_filterbank_weights(const jsg_filterbank* fb, float* dense) {
    if (!fb || !dense) return jsg_fail(JSG_ERR_INVALID, "jsg_filterbank_weights: null argument");
    const int H = fb->n / 2 + 1;
    std::fill(dense, dense + (size_t)fb->n_bands * H, 0.0f);
    for (int b = 0; b < fb->n_bands; ++b)
        for (int k = 0; k < fb->count[b]; ++k) dense[(size_t)b * H + fb->first[b] + k] = fb->w[(size_t)fb->offset[b] + k];
    return JSG_OK;
}

}  // extern "C"
