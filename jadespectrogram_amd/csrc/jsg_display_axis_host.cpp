// Frequency axes of the display: the row table on the host (jsg_freq_axis_build: double arithmetic, like jsg_filterbank_build) and the
// device object (jsg_freq_axis_create: the table and its row tiles uploaded once).  The kernel that draws an image over an axis lives in
// jsg_display_axis.hip; include/jsg.h (section 2c) states the semantics.
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

struct Rows {
    std::vector<int> first, count;
    std::vector<float> t, centre;
};

int check_spec(const jsg_axis_spec* s) {
    if (!s) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: null spec");
    if (!fft_size_supported(s->n)) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: n must be a power of two in 512..8192");
    if (!(s->fs > 0.f) || !std::isfinite(s->fs)) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: fs must be > 0");
    if (s->scale != JSG_AXIS_LINEAR && s->scale != JSG_AXIS_LOG && s->scale != JSG_AXIS_MEL)
        return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: scale must be LINEAR, LOG or MEL");
    if (s->height < 2 || s->height > JSG_AXIS_MAX_HEIGHT) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: height must be in 2..16384");
    if (!(s->fmin >= 0.f)) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: fmin must be >= 0");
    if (!(double(s->fmax) <= 0.5 * double(s->fs))) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: fmax must be <= fs/2");
    if (!(s->fmin < s->fmax)) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: fmin must be < fmax");
    if (s->scale == JSG_AXIS_LOG && !(s->fmin > 0.f)) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis: a LOG axis needs fmin > 0");
    return JSG_OK;
}

double warp(int scale, double f) { return scale == JSG_AXIS_LOG ? std::log(f) : scale == JSG_AXIS_MEL ? slaney_hz_to_mel(f) : f; }
double unwarp(int scale, double u) { return scale == JSG_AXIS_LOG ? std::exp(u) : scale == JSG_AXIS_MEL ? slaney_mel_to_hz(u) : u; }

void build_rows(const jsg_axis_spec* s, Rows& r) {
    const int H = s->height, top = s->n / 2;
    const double n = s->n, fs = s->fs;
    const double u0 = warp(s->scale, s->fmin), du = (warp(s->scale, s->fmax) - u0) / double(H - 1);
    std::vector<double> b(size_t(H) + 1);   // every bound once: row r = [b_r, b_r+1)
    for (int j = 0; j <= H; ++j) b[j] = unwarp(s->scale, u0 + (double(j) - 0.5) * du) * n / fs;
    r.first.resize(H);
    r.count.resize(H);
    r.t.resize(H);
    r.centre.resize(H);
    for (int row = 0; row < H; ++row) {
        const double c = unwarp(s->scale, u0 + double(row) * du);
        r.centre[row] = float(c);
        // integers k in [0, n/2] with b_r <= k < b_r+1
        const double lo = std::max(0.0, std::ceil(b[row]));
        double hi = std::ceil(b[row + 1]) - 1.0;   // the last integer < b_r+1
        hi = std::min(hi, double(top));
        if (hi >= lo) {
            r.first[row] = int(lo);
            r.count[row] = int(hi - lo) + 1;
            r.t[row] = 0.f;
        } else {
            const double x = c * n / fs;
            const int k = std::min(int(std::floor(x)), top - 1);
            r.first[row] = k;
            r.count[row] = 0;
            r.t[row] = float(x - double(k));
        }
    }
}

// Consecutive rows into tiles of at most kAxisTileRows rows whose bins fit kAxisSpan (one reduced row wider than that is a tile of
// its own): each dB value is staged about once, whatever the axis.
std::vector<int> build_tiles(const Rows& r) {
    std::vector<int> tiles;
    const int H = int(r.first.size());
    auto lo_of = [&](int i) { return r.first[i]; };
    auto hi_of = [&](int i) { return r.first[i] + std::max(r.count[i], r.count[i] ? 0 : 2); };   // one past the last bin read
    int row = 0;
    while (row < H) {
        int lo = lo_of(row), hi = hi_of(row), end = row + 1;
        while (end < H && end - row < kAxisTileRows) {
            const int nlo = std::min(lo, lo_of(end)), nhi = std::max(hi, hi_of(end));
            if (nhi - nlo > kAxisSpan) break;
            lo = nlo;
            hi = nhi;
            ++end;
        }
        tiles.insert(tiles.end(), {row, end - row, lo, hi - lo});
        row = end;
    }
    return tiles;
}

}  // namespace

extern "C" {

int jsg_freq_axis_build(const jsg_axis_spec* s, int32_t* first_bin, int32_t* n_bins, float* interp_t, float* centre_hz) {
    int rc = check_spec(s);
    if (rc != JSG_OK) return rc;
    if (!first_bin || !n_bins || !interp_t || !centre_hz) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis_build: null output array");
    Rows r;
    build_rows(s, r);
    const size_t H = size_t(s->height);
    std::memcpy(first_bin, r.first.data(), H * 4);
    std::memcpy(n_bins, r.count.data(), H * 4);
    std::memcpy(interp_t, r.t.data(), H * 4);
    std::memcpy(centre_hz, r.centre.data(), H * 4);
    return JSG_OK;
}

int jsg_freq_axis_create(jsg_freq_axis** out, const jsg_axis_spec* s) {
    if (!out) return jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis_create: null argument");
    *out = nullptr;
    int rc = check_spec(s);
    if (rc != JSG_OK) return rc;
    Rows r;
    build_rows(s, r);
    const std::vector<int> tiles = build_tiles(r);
    static const char* who = "jsg_freq_axis_create";
    std::unique_ptr<jsg_freq_axis> ax(new (std::nothrow) jsg_freq_axis());
    if (!ax) return jsg_fail_who(JSG_ERR_NOMEM, who, "out of host memory");
    ax->n = s->n;
    ax->height = s->height;
    ax->n_tiles = int(tiles.size() / 4);
    const size_t H = size_t(s->height);
    std::vector<int> blob(3 * H + tiles.size());
    std::memcpy(blob.data(), r.first.data(), H * 4);
    std::memcpy(blob.data() + H, r.count.data(), H * 4);
    std::memcpy(blob.data() + 2 * H, r.t.data(), H * 4);
    std::memcpy(blob.data() + 3 * H, tiles.data(), tiles.size() * 4);
    rc = ax->blob.upload(blob.data(), blob.size() * 4, who);
    if (rc != JSG_OK) return rc;
    ax->d_rows = static_cast<const int*>(ax->blob.data());
    ax->d_tiles = ax->d_rows + 3 * H;
    touch_axis_module();
    ax->centre_hz = std::move(r.centre);
    *out = ax.release();
    return JSG_OK;
}

int jsg_freq_axis_destroy(jsg_freq_axis* ax) {
    delete ax;
    return JSG_OK;
}

int jsg_freq_axis_height(const jsg_freq_axis* ax) { return ax ? ax->height : jsg_fail(JSG_ERR_INVALID, "jsg_freq_axis_height: null"); }

}  // extern "C"
