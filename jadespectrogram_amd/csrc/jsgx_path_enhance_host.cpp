// libjsgx.so, path enhancement and time-lag conversion (include/jsgx.h sections 10 and 11): the refusals, the plan and the filter-bank
// builder, on the host and without a device.  The kernels and their launchers are in jsgx_path_enhance.hip; the error text (jsgx::fail) is
// in jsgx_beat_host.cpp.
#include <cmath>
#include <cstdint>
#include <vector>

#include "jsgx_internal.h"

namespace jsgx {

namespace {
using jsg::addr;
using jsg::i128;
using jsg::overlap;

// the centred quintic B-spline
double b5(double x) {
    x = std::fabs(x);
    if (x < 1.0) {
        const double t = x * x;
        return t * (t * (0.25 - x / 12.0) - 0.5) + 0.55;
    }
    if (x < 2.0) return x * (x * (x * (x * (x / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
    if (x < 3.0) {
        const double y = 3.0 - x;
        return y * y * y * y * y / 120.0;
    }
    return 0.0;
}

// the reflection about the end samples of 0..n-1, period 2 (n - 1)
int mirror(int k, int n) {
    const int period = 2 * (n - 1);
    k %= period;
    if (k < 0) k += period;
    return k < n ? k : period - k;
}

struct Table {
    int h = 0, w = 0;
    std::vector<double> v;
};

// One filter of the bank, as the header states it: diag(window), rotated unless the slope is 1, clipped, normalised, zero_mean.
// False where the clipped table has no positive sum.
bool diagonal_table(const double* win, int n, double slope, bool zero_mean, Table* out) {
    Table t;
    if (std::fabs(slope - 1.0) <= 1e-8 + 1e-5) {
        t.h = t.w = n;
        t.v.assign((size_t)n * n, 0.0);
        for (int k = 0; k < n; ++k) t.v[(size_t)k * n + k] = win[k];
    } else {
        const double pi = 3.14159265358979323846;
        const double degrees = -(std::atan(slope) * 180.0 / pi - 45.0);
        const double angle = degrees * (pi / 180.0);
        const double c = std::cos(angle), s = std::sin(angle), dn = (double)n;
        // the rotated corners (0, 0), (0, n), (n, 0), (n, n): the extent of each coordinate
        const double y4[4] = {0.0, s * dn, c * dn, c * dn + s * dn}, x4[4] = {0.0, c * dn, -s * dn, -s * dn + c * dn};
        double ylo = y4[0], yhi = y4[0], xlo = x4[0], xhi = x4[0];
        for (int k = 1; k < 4; ++k) {
            ylo = std::fmin(ylo, y4[k]), yhi = std::fmax(yhi, y4[k]);
            xlo = std::fmin(xlo, x4[k]), xhi = std::fmax(xhi, x4[k]);
        }
        t.h = (int)(yhi - ylo + 0.5), t.w = (int)(xhi - xlo + 0.5);
        if (t.h < 1 || t.w < 1) return false;
        const double cy = (t.h - 1) / 2.0, cx = (t.w - 1) / 2.0, centre = (dn - 1.0) / 2.0;
        const double off_y = centre - (c * cy + s * cx), off_x = centre - (-s * cy + c * cx);
        t.v.assign((size_t)t.h * t.w, 0.0);
        for (int y = 0; y < t.h; ++y)
            for (int x = 0; x < t.w; ++x) {
                const double py = c * y + s * x + off_y, px = -s * y + c * x + off_x;
                if (py < 0.0 || py > dn - 1.0 || px < 0.0 || px > dn - 1.0) continue;
                const int y0 = (int)std::floor(py) - 2, x0 = (int)std::floor(px) - 2;
                double wy[6], wx[6];
                for (int k = 0; k < 6; ++k) wy[k] = b5(py - (y0 + k)), wx[k] = b5(px - (x0 + k));
                // win is diag(window): of the 6 x 6 samples only those with mirror(yy) == mirror(xx) are not zero
                double sum = 0.0;
                for (int a = 0; a < 6; ++a) {
                    const int ya = mirror(y0 + a, n);
                    double row = 0.0;
                    for (int b = 0; b < 6; ++b)
                        if (mirror(x0 + b, n) == ya) row += wx[b] * win[ya];
                    sum += wy[a] * row;
                }
                t.v[(size_t)y * t.w + x] = sum;
            }
    }
    double total = 0.0;
    for (double& e : t.v) {
        if (e < 0.0) e = 0.0;
        total += e;
    }
    if (!(total > 0.0) || !std::isfinite(total)) return false;
    for (double& e : t.v) e /= total;
    if (zero_mean) {
        double mean = 0.0;
        for (double e : t.v) mean += e;
        mean /= (double)t.v.size();
        for (double& e : t.v) e -= mean;
    }
    *out = std::move(t);
    return true;
}

bool finite_window(const double* w, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(w[k])) return false;
    return true;
}
}  // namespace

int path_enhance_check(const jsgx_path_enhance_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->r) return fail(JSGX_ERR_INVALID, who, "null r");
    if (!g->tap_w) return fail(JSGX_ERR_INVALID, who, "null tap_w");
    if (!g->tap_at) return fail(JSGX_ERR_INVALID, who, "null tap_at");
    if (!g->filter_first) return fail(JSGX_ERR_INVALID, who, "null filter_first");
    if (!g->out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!jsg::aligned4(g->r, g->tap_w, g->out) || !jsg::aligned4(g->tap_at, g->filter_first)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->m < 1 || g->m > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "m must be in 1..65536");
    if (g->n_filters < 1 || g->n_filters > JSGX_PE_MAX_FILTERS) return fail(JSGX_ERR_INVALID, who, "n_filters must be in 1..32");
    if (g->n_taps < 1 || g->n_taps > JSGX_PE_MAX_TAPS) return fail(JSGX_ERR_INVALID, who, "n_taps must be in 1..1048576");
    if (g->reach_i < 0 || g->reach_i > JSGX_PE_MAX_REACH) return fail(JSGX_ERR_INVALID, who, "reach_i must be in 0..64");
    if (g->reach_j < 0 || g->reach_j > JSGX_PE_MAX_REACH) return fail(JSGX_ERR_INVALID, who, "reach_j must be in 0..64");
    if (g->clip != 0 && g->clip != 1) return fail(JSGX_ERR_INVALID, who, "clip must be 0 or 1");
    i128 r_bytes, out_bytes;
    int rc = check_plane(who, "r", "", "m", g->n, g->m, g->r_pitch, g->r_pair_pitch, g->pairs, &r_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "out", "", "m", g->n, g->m, g->out_pitch, g->out_pair_pitch, g->pairs, &out_bytes);
    if (rc != JSGX_OK) return rc;
    const i128 out0 = addr(g->out);
    if (overlap(out0, out_bytes, addr(g->r), r_bytes)) return fail(JSGX_ERR_INVALID, who, "out overlaps r");
    if (overlap(out0, out_bytes, addr(g->tap_w), 4 * (i128)g->n_taps)) return fail(JSGX_ERR_INVALID, who, "out overlaps tap_w");
    if (overlap(out0, out_bytes, addr(g->tap_at), 4 * (i128)g->n_taps)) return fail(JSGX_ERR_INVALID, who, "out overlaps tap_at");
    if (overlap(out0, out_bytes, addr(g->filter_first), 4 * ((i128)g->n_filters + 1))) return fail(JSGX_ERR_INVALID, who, "out overlaps filter_first");
    return JSGX_OK;
}

int lag_check(const jsgx_lag_args* g, const char* who) {
    if (!g) return fail(JSGX_ERR_INVALID, who, "null argument");
    if (!g->in) return fail(JSGX_ERR_INVALID, who, "null in");
    if (!g->out) return fail(JSGX_ERR_INVALID, who, "null out");
    if (!jsg::aligned4(g->in, g->out)) return fail(JSGX_ERR_INVALID, who, "pointers must be 4-byte aligned");
    if (g->pairs < 1 || g->pairs > 65535) return fail(JSGX_ERR_INVALID, who, "pairs must be in 1..65535");
    if (g->n < 1 || g->n > JSGX_DTW_MAX_LEN) return fail(JSGX_ERR_INVALID, who, "n must be in 1..65536");
    if (g->pad != 0 && g->pad != 1) return fail(JSGX_ERR_INVALID, who, "pad must be 0 or 1");
    if (g->axis != 0 && g->axis != 1) return fail(JSGX_ERR_INVALID, who, "axis must be 0 or 1");
    if (g->inverse != 0 && g->inverse != 1) return fail(JSGX_ERR_INVALID, who, "inverse must be 0 or 1");
    if (g->reserved0 != 0) return fail(JSGX_ERR_INVALID, who, "reserved0 must be 0");
    const LagShape s = lag_shape(g->n, g->pad, g->axis, g->inverse);
    i128 in_bytes, out_bytes;
    int rc = check_plane(who, "in", "", "the input's columns", s.in_rows, s.in_cols, g->in_pitch, g->in_pair_pitch, g->pairs, &in_bytes);
    if (rc == JSGX_OK) rc = check_plane(who, "out", "", "the output's columns", s.out_rows, s.out_cols, g->out_pitch, g->out_pair_pitch, g->pairs, &out_bytes);
    if (rc != JSGX_OK) return rc;
    if (overlap(addr(g->out), out_bytes, addr(g->in), in_bytes)) return fail(JSGX_ERR_INVALID, who, "out overlaps in");
    return JSGX_OK;
}

}  // namespace jsgx

using namespace jsgx;

extern "C" {

int jsgx_path_enhance_plan(const jsgx_path_enhance_args* g, char* name, int name_len, int32_t* tile_rows, int32_t* tile_cols, int32_t* threads, int32_t* lds_bytes) {
    static const char* who = "jsgx_path_enhance_plan";
    int rc = check_name_buffer(who, name, name_len, 32);
    if (rc == JSGX_OK) rc = path_enhance_check(g, who);
    if (rc != JSGX_OK) return rc;
    put_name(name, name_len, "path_enhance_tiles");
    if (tile_rows) *tile_rows = JSGX_PE_TILE;
    if (tile_cols) *tile_cols = JSGX_PE_TILE;
    if (threads) *threads = JSGX_PE_THREADS;
    if (lds_bytes) *lds_bytes = pe_lds_bytes(g->reach_i, g->reach_j);
    return JSGX_OK;
}

int jsgx_diagonal_filter_table(const double* window, int32_t n, double slope, int32_t zero_mean, int32_t* rows, int32_t* cols, double* table, int64_t capacity) {
    static const char* who = "jsgx_diagonal_filter_table";
    if (!window) return fail(JSGX_ERR_INVALID, who, "null window");
    if (!rows) return fail(JSGX_ERR_INVALID, who, "null rows");
    if (!cols) return fail(JSGX_ERR_INVALID, who, "null cols");
    if (n < JSGX_PE_MIN_WINDOW || n > JSGX_PE_MAX_WINDOW) return fail(JSGX_ERR_INVALID, who, "n must be in 3..101");
    if (!std::isfinite(slope) || !(slope > 0.0)) return fail(JSGX_ERR_INVALID, who, "slope must be finite and > 0");
    if (zero_mean != 0 && zero_mean != 1) return fail(JSGX_ERR_INVALID, who, "zero_mean must be 0 or 1");
    if (!finite_window(window, n)) return fail(JSGX_ERR_INVALID, who, "window must be finite");
    Table t;
    if (!diagonal_table(window, n, slope, zero_mean != 0, &t)) return fail(JSGX_ERR_INVALID, who, "the filter has no positive sum");
    *rows = t.h, *cols = t.w;
    if (!table) return JSGX_OK;
    if (capacity < (int64_t)t.v.size()) return fail(JSGX_ERR_INVALID, who, "capacity smaller than rows * cols");
    for (size_t k = 0; k < t.v.size(); ++k) table[k] = t.v[k];
    return JSGX_OK;
}

int jsgx_diagonal_filter_build(const double* window, int32_t n, double min_ratio, double max_ratio, int32_t n_filters, int32_t zero_mean, double drop_below,
                               int32_t* n_taps, int32_t* reach_i, int32_t* reach_j, float* tap_w, int32_t* tap_at, int32_t* filter_first, int64_t capacity) {
    static const char* who = "jsgx_diagonal_filter_build";
    if (!window) return fail(JSGX_ERR_INVALID, who, "null window");
    if (!n_taps) return fail(JSGX_ERR_INVALID, who, "null n_taps");
    if (!reach_i) return fail(JSGX_ERR_INVALID, who, "null reach_i");
    if (!reach_j) return fail(JSGX_ERR_INVALID, who, "null reach_j");
    const int given = (tap_w != nullptr) + (tap_at != nullptr) + (filter_first != nullptr);
    if (given != 0 && given != 3) return fail(JSGX_ERR_INVALID, who, "tap_w, tap_at and filter_first go together");
    if (n < JSGX_PE_MIN_WINDOW || n > JSGX_PE_MAX_WINDOW) return fail(JSGX_ERR_INVALID, who, "n must be in 3..101");
    if (!std::isfinite(min_ratio) || !(min_ratio > 0.0)) return fail(JSGX_ERR_INVALID, who, "min_ratio must be finite and > 0");
    if (!std::isfinite(max_ratio) || !(max_ratio > 0.0)) return fail(JSGX_ERR_INVALID, who, "max_ratio must be finite and > 0");
    if (min_ratio > max_ratio) return fail(JSGX_ERR_INVALID, who, "min_ratio above max_ratio");
    if (n_filters < 1 || n_filters > JSGX_PE_MAX_FILTERS) return fail(JSGX_ERR_INVALID, who, "n_filters must be in 1..32");
    if (zero_mean != 0 && zero_mean != 1) return fail(JSGX_ERR_INVALID, who, "zero_mean must be 0 or 1");
    if (!(drop_below >= 0.0) || !(drop_below < 1.0)) return fail(JSGX_ERR_INVALID, who, "drop_below must be in [0, 1)");
    if (!finite_window(window, n)) return fail(JSGX_ERR_INVALID, who, "window must be finite");
    // numpy's linspace: start + i * step, the last one the stop itself
    const double lo = std::log2(min_ratio), hi = std::log2(max_ratio), step = n_filters > 1 ? (hi - lo) / (n_filters - 1) : 0.0;
    std::vector<float> w;
    std::vector<int32_t> at, first(1, 0);
    int ri = 0, rj = 0;
    for (int f = 0; f < n_filters; ++f) {
        const double e = f == 0 ? lo : (f == n_filters - 1 ? hi : lo + f * step);
        Table t;
        if (!diagonal_table(window, n, std::exp2(e), zero_mean != 0, &t)) return fail(JSGX_ERR_INVALID, who, "a filter has no positive sum");
        float largest = 0.f;
        for (double v : t.v) largest = std::fmax(largest, std::fabs((float)v));
        for (int a = 0; a < t.h; ++a)
            for (int b = 0; b < t.w; ++b) {
                const float v = (float)t.v[(size_t)a * t.w + b];
                if (!std::isnormal(v) || std::fabs((double)v) < drop_below * (double)largest) continue;       // zero, subnormal, or trimmed
                const int di = t.h / 2 - a, dj = t.w / 2 - b;
                ri = std::abs(di) > ri ? std::abs(di) : ri;
                rj = std::abs(dj) > rj ? std::abs(dj) : rj;
                w.push_back(v);
                at.push_back((int32_t)(((uint32_t)di << 16) | ((uint32_t)dj & 0xffffu)));
            }
        first.push_back((int32_t)w.size());
    }
    *n_taps = (int32_t)w.size(), *reach_i = ri, *reach_j = rj;
    if (w.empty()) return fail(JSGX_ERR_INVALID, who, "the bank has no tap");
    if (w.size() > JSGX_PE_MAX_TAPS) return fail(JSGX_ERR_INVALID, who, "the bank has more than 1048576 taps");
    if (ri > JSGX_PE_MAX_REACH || rj > JSGX_PE_MAX_REACH) return fail(JSGX_ERR_INVALID, who, "the bank reaches further than 64");
    if (given == 0) return JSGX_OK;
    if (capacity < (int64_t)w.size()) return fail(JSGX_ERR_INVALID, who, "capacity smaller than n_taps");
    for (size_t k = 0; k < w.size(); ++k) tap_w[k] = w[k], tap_at[k] = at[k];
    for (size_t k = 0; k < first.size(); ++k) filter_first[k] = first[k];
    return JSGX_OK;
}

}  // extern "C"
