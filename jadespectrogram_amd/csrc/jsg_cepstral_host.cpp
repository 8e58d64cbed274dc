// libjsg.so, cepstral coefficients and delta features (include/jsg.h section 2k): the refusals, the plan of a projection, the DCT
// tables and the Savitzky-Golay weights, on the host and without a device.  The kernels and their launchers are in jsg_cepstral.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

namespace {
const double kPi = 3.14159265358979323846;
}  // namespace

int mfcc_check(const jsg_mfcc_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->table) return jsg_fail_who(JSG_ERR_INVALID, who, "null table");
    if (!g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null out");
    int rc = check_aligned4(who, g->in, g->table, g->out);
    if (rc == JSG_OK) rc = check_rows(g->rows, who);
    if (rc != JSG_OK) return rc;
    if (g->n_in < 1 || g->n_in > JSG_MFCC_MAX_BANDS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_in must be in 1..4096");
    if (g->n_out < 1 || g->n_out > JSG_MFCC_MAX_COEFFS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_out must be in 1..4096");
    if ((long long)g->n_in * g->n_out > JSG_MFCC_MAX_TABLE) return jsg_fail_who(JSG_ERR_INVALID, who, "n_in*n_out must be at most 32768");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (g->chunk_frames < 0 || g->chunk_frames > 65536) return jsg_fail_who(JSG_ERR_INVALID, who, "chunk_frames must be 0 or in 1..65536");
    if (g->frame_pitch < g->n_in) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_pitch smaller than n_in");
    const bool multi = g->rows > 1;
    const i128 in_plane = plane(g->n_frames, g->frame_pitch, g->n_in);
    if (multi && (i128)g->row_pitch < in_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "row_pitch smaller than (n_frames-1)*frame_pitch + n_in");
    if (g->out_frame_pitch < g->n_out) return jsg_fail_who(JSG_ERR_INVALID, who, "out_frame_pitch smaller than n_out");
    const i128 out_plane = plane(g->n_frames, g->out_frame_pitch, g->n_out);
    if (multi && (i128)g->out_row_pitch < out_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "out_row_pitch smaller than (n_frames-1)*out_frame_pitch + n_out");
    const i128 out_bytes = span_bytes(g->rows, g->out_row_pitch, out_plane, 4);
    if (overlap(addr(g->in), span_bytes(g->rows, g->row_pitch, in_plane, 4), addr(g->out), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps in");
    if (overlap(addr(g->table), 4 * (i128)g->n_in * g->n_out, addr(g->out), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps table");
    return JSG_OK;
}

// MB by n_out alone: the smallest of 4, 5, 8, 10, 16 that gives the four waves of a workgroup at most one block each, else 16.  F is
// chunk_frames or kMfccFrames (one frame per lane of a wave), bounded by n_frames and by what the 160 KiB hold next to the table.  One
// frame needs at most 4097 + 4097 floats next to 32768, or 9 + 4097 next to a table of 4096 rows, so 1 <= F always.
void mfcc_resolve(const jsg_mfcc_args* g, MfccPlan* p) {
    const long long B = g->n_in, M = g->n_out;
    static const int blocks[] = {4, 5, 8, 10, 16};
    p->MB = 16;
    for (int mb : blocks)
        if (4 * mb >= M) {
            p->MB = mb;
            break;
        }
    const long long per = (B | 1) + (M | 1);
    long long F = g->chunk_frames ? std::min<long long>(g->chunk_frames, kMfccFrames) : kMfccFrames;
    F = std::min<long long>(F, g->n_frames);
    F = std::max<long long>(1, std::min<long long>(F, (kMfccLdsOne - M * B) / per));
    p->F = (int)F;
    p->chunks = (g->n_frames + F - 1) / F;
    p->lds_floats = (int)(M * B + F * per);
}

const char* mfcc_path_name(const MfccPlan& p) {
    return p.MB == 4 ? "mfcc_block4" : p.MB == 5 ? "mfcc_block5" : p.MB == 8 ? "mfcc_block8" : p.MB == 10 ? "mfcc_block10" : "mfcc_block16";
}

int delta_check(const jsg_delta_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null in");
    if (!g->weights) return jsg_fail_who(JSG_ERR_INVALID, who, "null weights");
    if (!g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null out");
    int rc = check_aligned4(who, g->in, g->weights, g->out);
    if (rc == JSG_OK) rc = check_rows(g->rows, who);
    if (rc != JSG_OK) return rc;
    if (g->n_coeffs < 1 || g->n_coeffs > JSG_DELTA_MAX_COEFFS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_coeffs must be in 1..65536");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (g->width < 3 || g->width > JSG_DELTA_MAX_WIDTH || g->width % 2 == 0) return jsg_fail_who(JSG_ERR_INVALID, who, "width must be odd and in 3..255");
    if (g->mode != JSG_DELTA_EDGE_INTERP && g->mode != JSG_DELTA_EDGE_NEAREST) return jsg_fail_who(JSG_ERR_INVALID, who, "mode must be 0 (interp) or 1 (nearest)");
    if (g->mode == JSG_DELTA_EDGE_INTERP && g->n_frames < g->width) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames smaller than width (interp)");
    if (g->frame_pitch < g->n_coeffs) return jsg_fail_who(JSG_ERR_INVALID, who, "frame_pitch smaller than n_coeffs");
    const bool multi = g->rows > 1;
    const i128 in_plane = plane(g->n_frames, g->frame_pitch, g->n_coeffs);
    if (multi && (i128)g->row_pitch < in_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "row_pitch smaller than (n_frames-1)*frame_pitch + n_coeffs");
    if (g->out_frame_pitch < g->n_coeffs) return jsg_fail_who(JSG_ERR_INVALID, who, "out_frame_pitch smaller than n_coeffs");
    const i128 out_plane = plane(g->n_frames, g->out_frame_pitch, g->n_coeffs);
    if (multi && (i128)g->out_row_pitch < out_plane) return jsg_fail_who(JSG_ERR_INVALID, who, "out_row_pitch smaller than (n_frames-1)*out_frame_pitch + n_coeffs");
    const i128 out_bytes = span_bytes(g->rows, g->out_row_pitch, out_plane, 4);
    if (overlap(addr(g->in), span_bytes(g->rows, g->row_pitch, in_plane, 4), addr(g->out), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps in");
    if (overlap(addr(g->weights), 4 * (i128)g->width, addr(g->out), out_bytes)) return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps weights");
    return JSG_OK;
}

}  // namespace jsg

using namespace jsg;

namespace {
// jsg_mfcc_plan (the name is optional) and jsg_mfcc_kernel_name (the name is all it gives)
int mfcc_plan_call(const char* who, const jsg_mfcc_args* g, char* name, int name_len, bool need_name, int32_t* frames_per_item, int32_t* lds_bytes) {
    int rc = check_name_buffer(who, name, name_len, need_name);
    if (rc == JSG_OK) rc = mfcc_check(g, who);
    if (rc != JSG_OK) return rc;
    MfccPlan p{};
    mfcc_resolve(g, &p);
    put_path_name(name, name_len, mfcc_path_name(p));
    if (frames_per_item) *frames_per_item = p.F;
    if (lds_bytes) *lds_bytes = 4 * p.lds_floats;
    return JSG_OK;
}
}  // namespace

extern "C" {

int jsg_mfcc_plan(const jsg_mfcc_args* g, char* name, int name_len, int32_t* frames_per_item, int32_t* lds_bytes) {
    return mfcc_plan_call("jsg_mfcc_plan", g, name, name_len, false, frames_per_item, lds_bytes);
}

int jsg_mfcc_kernel_name(const jsg_mfcc_args* g, char* out, int out_len) { return mfcc_plan_call("jsg_mfcc_kernel_name", g, out, out_len, true, nullptr, nullptr); }

int jsg_mfcc_table_build(int32_t n_bands, int32_t n_coeffs, int32_t norm, double lifter, int32_t inverse, float* out) {
    static const char* who = "jsg_mfcc_table_build";
    if (!out) return jsg_fail_who(JSG_ERR_INVALID, who, "null out");
    if (n_bands < 1 || n_bands > JSG_MFCC_MAX_BANDS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bands must be in 1..4096");
    if (n_coeffs < 1 || n_coeffs > JSG_MFCC_MAX_COEFFS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_coeffs must be in 1..4096");
    if (n_coeffs > n_bands) return jsg_fail_who(JSG_ERR_INVALID, who, "n_coeffs must be at most n_bands");
    if ((long long)n_bands * n_coeffs > JSG_MFCC_MAX_TABLE) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bands*n_coeffs must be at most 32768");
    if (norm != JSG_DCT_NORM_NONE && norm != JSG_DCT_NORM_ORTHO) return jsg_fail_who(JSG_ERR_INVALID, who, "norm must be 0 (none) or 1 (ortho)");
    if (inverse != 0 && inverse != 1) return jsg_fail_who(JSG_ERR_INVALID, who, "inverse must be 0 or 1");
    if (!std::isfinite(lifter) || lifter < 0) return jsg_fail_who(JSG_ERR_INVALID, who, "lifter must be finite and >= 0");
    const long long B = n_bands, M = n_coeffs;
    std::vector<double> L(M, 1.0);
    if (lifter > 0)
        for (long long m = 0; m < M; ++m) L[m] = 1.0 + (lifter / 2) * std::sin(kPi * (double)(m + 1) / lifter);
    if (inverse)
        for (long long m = 0; m < M; ++m)
            if (L[m] == 0) return jsg_fail_who(JSG_ERR_INVALID, who, "the lifter is zero at a coefficient: no inverse");
    for (long long m = 0; m < M; ++m) {
        const double s = norm == JSG_DCT_NORM_ORTHO ? std::sqrt(1.0 / ((m == 0 ? 4.0 : 2.0) * (double)B)) : 1.0;
        for (long long b = 0; b < B; ++b) {
            const long long k = (m * (2 * b + 1)) % (4 * B);
            const double c = (k == B || k == 3 * B) ? 0.0 : std::cos(kPi * (double)k / (double)(2 * B));     // cos(pi/2) is 0, not 6e-17
            if (!inverse)
                out[m * B + b] = (float)(2 * c * s * L[m]);
            else if (norm == JSG_DCT_NORM_ORTHO)
                out[b * M + m] = (float)(2 * c * s / L[m]);
            else
                out[b * M + m] = (float)((m == 0 ? 1.0 : 2 * c) / (double)(2 * B) / L[m]);
        }
    }
    return JSG_OK;
}

// The normal equations of the fit on x = (j - h) / h (in [-1, 1]: a 5 x 5 system at most, well conditioned), the odd power sums exactly
// zero; the left half is evaluated and mirrored, so the weights are exactly symmetric (even order) or antisymmetric with a zero centre
// (odd order).
int jsg_delta_weights_build(int32_t width, int32_t order, float* out) {
    static const char* who = "jsg_delta_weights_build";
    if (!out) return jsg_fail_who(JSG_ERR_INVALID, who, "null out");
    if (width < 3 || width > JSG_DELTA_MAX_WIDTH || width % 2 == 0) return jsg_fail_who(JSG_ERR_INVALID, who, "width must be odd and in 3..255");
    if (order < 1 || order > JSG_DELTA_MAX_ORDER || order >= width) return jsg_fail_who(JSG_ERR_INVALID, who, "order must be in 1..4 and below width");
    const int h = width / 2, n = order + 1;
    double sums[2 * JSG_DELTA_MAX_ORDER + 1] = {};
    for (int j = 1; j <= h; ++j) {
        const double x = (double)j / h;
        double pw = 1.0;
        for (int k = 0; k <= 2 * order; ++k, pw *= x)
            if (k % 2 == 0) sums[k] += 2 * pw;
    }
    sums[0] += 1.0;     // x = 0
    double G[JSG_DELTA_MAX_ORDER + 1][JSG_DELTA_MAX_ORDER + 2] = {};
    for (int p = 0; p < n; ++p) {
        for (int q = 0; q < n; ++q) G[p][q] = sums[p + q];
        G[p][n] = p == order ? 1.0 : 0.0;
    }
    for (int c = 0; c < n; ++c) {       // Gauss-Jordan with partial pivoting
        int piv = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(G[r][c]) > std::fabs(G[piv][c])) piv = r;
        if (G[piv][c] == 0) return jsg_fail_who(JSG_ERR_INVALID, who, "singular fit");
        for (int q = 0; q <= n; ++q) std::swap(G[c][q], G[piv][q]);
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            const double f = G[r][c] / G[c][c];
            for (int q = c; q <= n; ++q) G[r][q] -= f * G[c][q];
        }
    }
    double scale = 1.0;
    for (int k = 1; k <= order; ++k) scale *= (double)k / h;       // order! / h^order
    for (int j = 0; j <= h; ++j) {
        const double x = (double)(j - h) / h;
        double v = 0, pw = 1.0;
        for (int p = 0; p < n; ++p, pw *= x) v += G[p][n] / G[p][p] * pw;
        const float w = (j == h && order % 2 == 1) ? 0.f : (float)(scale * v);
        out[j] = w;
        out[width - 1 - j] = order % 2 == 1 ? -w : w;
    }
    if (order % 2 == 1) out[h] = 0.f;
    return JSG_OK;
}

}  // extern "C"
