// The host entry points of sections 10 and 11 of libjsgx.so (include/jsgx.h) from C++: the plan, the refusals with their texts in their
// order, and the filter-bank builder with guard bytes round its outputs.  No launch, so no device: built against libjsgx.so (CMake,
// jsg::jsgx) or, for the sanitizers, together with csrc/jsgx_beat_host.cpp and csrc/jsgx_path_enhance_host.cpp themselves
// (tests/test_path_enhance_host.py: -fsanitize=address,undefined).  Exit code 0 and "ok" on success.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "jsgx.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            ++failures;                                                  \
        }                                                                \
    } while (0)

template <class T>
static T* device(int k, int bytes = 0) {       // device pointers that are never dereferenced: every call below is refused or planned
    return reinterpret_cast<T*>((uintptr_t(k) << 44) + bytes);
}

static jsgx_path_enhance_args good() {         // 3 pairs of 100 x 300, 7 filters of 3000 taps in all
    jsgx_path_enhance_args a{};
    a.r = device<const float>(1);
    a.r_pitch = 300;
    a.r_pair_pitch = 100 * 300;
    a.tap_w = device<const float>(2);
    a.tap_at = device<const int32_t>(3);
    a.filter_first = device<const int32_t>(4);
    a.pairs = 3;
    a.n = 100;
    a.m = 300;
    a.n_filters = 7;
    a.n_taps = 3000;
    a.reach_i = 32;
    a.reach_j = 30;
    a.clip = 1;
    a.out = device<float>(5);
    a.out_pitch = 304;
    a.out_pair_pitch = 100 * 304;
    return a;
}

static bool refused(const jsgx_path_enhance_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_path_enhance_plan: %s", text);
    return jsgx_path_enhance_plan(&a, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}

static jsgx_lag_args good_lag() {              // 3 pairs of 100 x 100 to 200 x 100
    jsgx_lag_args a{};
    a.in = device<const float>(1);
    a.in_pitch = 100;
    a.in_pair_pitch = 100 * 100;
    a.pairs = 3;
    a.n = 100;
    a.pad = 1;
    a.axis = 1;
    a.out = device<float>(2);
    a.out_pitch = 104;
    a.out_pair_pitch = 200 * 104;
    return a;
}

#if defined(JSGX_PE_TEST_LAUNCHES)
static bool lag_refused(const jsgx_lag_args& a, const char* text) {
    char want[192];
    std::snprintf(want, sizeof want, "jsgx_lag_launch: %s", text);
    return jsgx_lag_launch(&a, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), want) == 0;
}
#endif

static const float kGuard = -7.25e11f;
static const int32_t kIGuard = -77777;

int main() {
    static_assert(sizeof(jsgx_path_enhance_args) == 104, "include/jsgx.h states the size");
    static_assert(sizeof(jsgx_lag_args) == 72, "include/jsgx.h states the size");
    EXPECT(jsgx_abi_version() == 1);

    // the plan over reaches
    char name[32];
    for (int reach : {0, 1, 25, 32, 64}) {
        jsgx_path_enhance_args d = good();
        d.reach_i = reach, d.reach_j = reach;
        int32_t rows = 0, cols = 0, threads = 0, lds = 0;
        EXPECT(jsgx_path_enhance_plan(&d, name, (int)sizeof name, &rows, &cols, &threads, &lds) == JSGX_OK);
        const int pitch = (64 + 2 * reach + 3) / 4 * 4 + 1;
        EXPECT(std::strcmp(name, "path_enhance_tiles") == 0 && rows == JSGX_PE_TILE && cols == JSGX_PE_TILE && threads == JSGX_PE_THREADS);
        EXPECT(lds == 4 * (64 + 2 * reach) * pitch && lds <= JSGX_PE_LDS_LIMIT && pitch % 4 == 1);
        if (reach == 32) EXPECT(2 * lds <= JSGX_PE_LDS_LIMIT);
    }
    jsgx_path_enhance_args d = good();
    EXPECT(jsgx_path_enhance_plan(&d, name, 31, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_path_enhance_plan: bad argument") == 0);
    EXPECT(jsgx_path_enhance_plan(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_ERR_INVALID &&
           std::strcmp(jsgx_last_error(), "jsgx_path_enhance_plan: null argument") == 0);

    // one refusal of every kind, in the header's order
    d = good(); d.r = nullptr; EXPECT(refused(d, "null r"));
    d = good(); d.tap_w = nullptr; EXPECT(refused(d, "null tap_w"));
    d = good(); d.tap_at = nullptr; EXPECT(refused(d, "null tap_at"));
    d = good(); d.filter_first = nullptr; EXPECT(refused(d, "null filter_first"));
    d = good(); d.out = nullptr; EXPECT(refused(d, "null out"));
    d = good(); d.tap_at = device<const int32_t>(3, 2); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.out = device<float>(5, 1); EXPECT(refused(d, "pointers must be 4-byte aligned"));
    d = good(); d.pairs = 0; EXPECT(refused(d, "pairs must be in 1..65535"));
    d = good(); d.n = 65537; EXPECT(refused(d, "n must be in 1..65536"));
    d = good(); d.m = 0; EXPECT(refused(d, "m must be in 1..65536"));
    d = good(); d.n_filters = 33; EXPECT(refused(d, "n_filters must be in 1..32"));
    d = good(); d.n_filters = 0; EXPECT(refused(d, "n_filters must be in 1..32"));
    d = good(); d.n_taps = 0; EXPECT(refused(d, "n_taps must be in 1..1048576"));
    d = good(); d.n_taps = JSGX_PE_MAX_TAPS + 1; EXPECT(refused(d, "n_taps must be in 1..1048576"));
    d = good(); d.reach_i = 65; EXPECT(refused(d, "reach_i must be in 0..64"));
    d = good(); d.reach_j = -1; EXPECT(refused(d, "reach_j must be in 0..64"));
    d = good(); d.clip = 2; EXPECT(refused(d, "clip must be 0 or 1"));
    d = good(); d.r_pitch = 299; EXPECT(refused(d, "r_pitch smaller than m"));
    d = good(); d.r_pair_pitch = 29999; EXPECT(refused(d, "r_pair_pitch does not cover a plane"));
    d = good(); d.out_pitch = 299; EXPECT(refused(d, "out_pitch smaller than m"));
    d = good(); d.out_pair_pitch = 99 * 304 + 299; EXPECT(refused(d, "out_pair_pitch does not cover a plane"));
    d = good(); d.out = const_cast<float*>(d.r) + 89999; EXPECT(refused(d, "out overlaps r"));
    d = good(); d.out = const_cast<float*>(d.r) + 90000; EXPECT(jsgx_path_enhance_plan(&d, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_OK);
    d = good(); d.out = const_cast<float*>(d.tap_w) + 2999; EXPECT(refused(d, "out overlaps tap_w"));
    d = good(); d.out = const_cast<float*>(d.tap_w) + 3000; EXPECT(jsgx_path_enhance_plan(&d, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_OK);
    d = good(); d.out = reinterpret_cast<float*>(const_cast<int32_t*>(d.tap_at)) - (2 * 100 * 304 + 99 * 304 + 300) + 1; EXPECT(refused(d, "out overlaps tap_at"));
    d = good(); d.out = reinterpret_cast<float*>(const_cast<int32_t*>(d.filter_first)) + 7; EXPECT(refused(d, "out overlaps filter_first"));
    d = good(); d.out = reinterpret_cast<float*>(const_cast<int32_t*>(d.filter_first)) + 8; EXPECT(jsgx_path_enhance_plan(&d, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_OK);
    // an earlier defect is the one reported
    d = good(); d.r = nullptr; d.pairs = 0; d.clip = 7; EXPECT(refused(d, "null r"));
    d = good(); d.n_taps = 0; d.reach_i = 99; d.r_pitch = 1; EXPECT(refused(d, "n_taps must be in 1..1048576"));
    d = good(); d.clip = 3; d.out_pitch = 1; d.out = const_cast<float*>(d.r); EXPECT(refused(d, "clip must be 0 or 1"));
    // one pair: the pair pitches are not looked at
    d = good(); d.pairs = 1; d.r_pair_pitch = d.out_pair_pitch = 0; EXPECT(jsgx_path_enhance_plan(&d, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == JSGX_OK);

    // ---- the builder: the size query, then the arrays between guards
    std::vector<double> window(101);
    for (int n : {3, 7, 31, 51, 101}) {
        for (int k = 0; k < n; ++k) window[k] = 0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * k / (n - 1));
        for (int zero_mean : {0, 1}) {
            if (zero_mean && n > 31) continue;
            int32_t count = -1, ri = -1, rj = -1;
            EXPECT(jsgx_diagonal_filter_build(window.data(), n, 0.5, 2.0, 7, zero_mean, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_OK);
            EXPECT(count > 0 && ri >= (n - 1) / 2 - 1 && ri <= JSGX_PE_MAX_REACH && rj == ri);
            std::vector<float> w(count + 2, kGuard);
            std::vector<int32_t> at(count + 2, kIGuard), first(7 + 1 + 2, kIGuard);
            int32_t count2 = -1, ri2 = -1, rj2 = -1;
            EXPECT(jsgx_diagonal_filter_build(window.data(), n, 0.5, 2.0, 7, zero_mean, 0.0, &count2, &ri2, &rj2, w.data() + 1, at.data() + 1, first.data() + 1, count) == JSGX_OK);
            EXPECT(count2 == count && ri2 == ri && rj2 == rj);
            EXPECT(w[0] == kGuard && w[count + 1] == kGuard && at[0] == kIGuard && at[count + 1] == kIGuard && first[0] == kIGuard && first[9] == kIGuard);
            EXPECT(first[1] == 0 && first[8] == count);
            int max_i = 0, max_j = 0;
            for (int f = 0; f < 7; ++f) {
                EXPECT(first[1 + f] < first[2 + f]);
                double sum = 0.0;
                int prev = INT32_MAX;
                for (int t = first[1 + f]; t < first[2 + f]; ++t) {
                    const int di = at[1 + t] >> 16, dj = (int16_t)(at[1 + t] & 0xffff);
                    EXPECT(std::isnormal(w[1 + t]) && (zero_mean || w[1 + t] > 0.f));
                    const int key = -di * 1024 - dj;              // row-major: a = h / 2 - di ascending, then b = w / 2 - dj
                    EXPECT(prev == INT32_MAX || key > prev);
                    prev = key;
                    max_i = std::abs(di) > max_i ? std::abs(di) : max_i;
                    max_j = std::abs(dj) > max_j ? std::abs(dj) : max_j;
                    sum += w[1 + t];
                }
                EXPECT(std::fabs(sum - (zero_mean ? 0.0 : 1.0)) < 1e-5);
            }
            EXPECT(max_i == ri && max_j == rj);
            // a capacity one short is refused and writes nothing
            std::vector<float> w2(count + 2, kGuard);
            EXPECT(jsgx_diagonal_filter_build(window.data(), n, 0.5, 2.0, 7, zero_mean, 0.0, &count2, &ri2, &rj2, w2.data() + 1, at.data() + 1, first.data() + 1, count - 1) == JSGX_ERR_INVALID);
            EXPECT(std::strcmp(jsgx_last_error(), "jsgx_diagonal_filter_build: capacity smaller than n_taps") == 0 && w2[1] == kGuard);
            // the dense table of one filter between guards
            int32_t rows = 0, cols = 0;
            EXPECT(jsgx_diagonal_filter_table(window.data(), n, 2.0, zero_mean, &rows, &cols, nullptr, 0) == JSGX_OK && rows == cols && rows >= n);
            std::vector<double> table((size_t)rows * cols + 2, -1.0e300);
            EXPECT(jsgx_diagonal_filter_table(window.data(), n, 2.0, zero_mean, &rows, &cols, table.data() + 1, (int64_t)rows * cols) == JSGX_OK);
            EXPECT(table[0] == -1.0e300 && table[(size_t)rows * cols + 1] == -1.0e300);
            double total = 0.0;
            for (size_t k = 1; k <= (size_t)rows * cols; ++k) total += table[k];
            EXPECT(std::fabs(total - (zero_mean ? 0.0 : 1.0)) < 1e-12);
            EXPECT(jsgx_diagonal_filter_table(window.data(), n, 2.0, zero_mean, &rows, &cols, table.data() + 1, (int64_t)rows * cols - 1) == JSGX_ERR_INVALID);
        }
    }
    // the builder's refusals, in their order
    {
        int32_t count = 0, ri = 0, rj = 0;
        float w1[1];
        auto text = [](const char* t) {
            char want[160];
            std::snprintf(want, sizeof want, "jsgx_diagonal_filter_build: %s", t);
            return std::strcmp(jsgx_last_error(), want) == 0;
        };
        const double* win = window.data();
        EXPECT(jsgx_diagonal_filter_build(nullptr, 7, 0.5, 2.0, 7, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("null window"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, 2.0, 7, 0, 0.0, nullptr, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("null n_taps"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, 2.0, 7, 0, 0.0, &count, nullptr, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("null reach_i"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, 2.0, 7, 0, 0.0, &count, &ri, nullptr, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("null reach_j"));
        EXPECT(jsgx_diagonal_filter_build(win, 2, 0.5, 2.0, 7, 0, 0.0, &count, &ri, &rj, w1, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("tap_w, tap_at and filter_first go together"));
        EXPECT(jsgx_diagonal_filter_build(win, 2, -1.0, 2.0, 7, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("n must be in 3..101"));
        EXPECT(jsgx_diagonal_filter_build(win, 102, 0.5, 2.0, 7, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("n must be in 3..101"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.0, NAN, 7, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("min_ratio must be finite and > 0"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, INFINITY, 0, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("max_ratio must be finite and > 0"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 2.5, 2.0, 0, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("min_ratio above max_ratio"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, 2.0, 33, 2, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("n_filters must be in 1..32"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, 2.0, 7, 2, -1.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("zero_mean must be 0 or 1"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, 2.0, 7, 0, 1.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("drop_below must be in [0, 1)"));
        EXPECT(jsgx_diagonal_filter_build(win, 7, 0.5, 2.0, 7, 0, NAN, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("drop_below must be in [0, 1)"));
        std::vector<double> bad(7, 0.0);
        EXPECT(jsgx_diagonal_filter_build(bad.data(), 7, 0.5, 2.0, 7, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("a filter has no positive sum"));
        bad[3] = INFINITY;
        EXPECT(jsgx_diagonal_filter_build(bad.data(), 7, 0.5, 2.0, 7, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("window must be finite"));
        for (int k = 0; k < 101; ++k) window[k] = 1.0;
        EXPECT(jsgx_diagonal_filter_build(win, 101, 0.02, 50.0, 3, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_ERR_INVALID && text("the bank reaches further than 64"));
        EXPECT(ri > 64 && count > 0);            // the size query still answers
        // a single slope-1 filter of a boxcar: the diagonal itself
        EXPECT(jsgx_diagonal_filter_build(win, 5, 1.0, 1.0, 1, 0, 0.0, &count, &ri, &rj, nullptr, nullptr, nullptr, 0) == JSGX_OK && count == 5 && ri == 2 && rj == 2);
    }

#if defined(JSGX_PE_TEST_LAUNCHES)
    // the launches' refusals, decided before any device call (the shipped library only: the launchers are HIP units)
    d = good(); d.r = nullptr;
    EXPECT(jsgx_path_enhance_launch(&d, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_path_enhance_launch: null r") == 0);
    jsgx_lag_args g = good_lag();
    EXPECT(jsgx_lag_launch(nullptr, nullptr) == JSGX_ERR_INVALID && std::strcmp(jsgx_last_error(), "jsgx_lag_launch: null argument") == 0);
    g = good_lag(); g.in = nullptr; EXPECT(lag_refused(g, "null in"));
    g = good_lag(); g.out = nullptr; EXPECT(lag_refused(g, "null out"));
    g = good_lag(); g.out = device<float>(2, 2); EXPECT(lag_refused(g, "pointers must be 4-byte aligned"));
    g = good_lag(); g.pairs = 65536; EXPECT(lag_refused(g, "pairs must be in 1..65535"));
    g = good_lag(); g.n = 0; EXPECT(lag_refused(g, "n must be in 1..65536"));
    g = good_lag(); g.pad = 2; EXPECT(lag_refused(g, "pad must be 0 or 1"));
    g = good_lag(); g.axis = -1; EXPECT(lag_refused(g, "axis must be 0 or 1"));
    g = good_lag(); g.inverse = 2; EXPECT(lag_refused(g, "inverse must be 0 or 1"));
    g = good_lag(); g.reserved0 = 1; EXPECT(lag_refused(g, "reserved0 must be 0"));
    g = good_lag(); g.in_pitch = 99; EXPECT(lag_refused(g, "in_pitch smaller than the input's columns"));
    g = good_lag(); g.in_pair_pitch = 9999; EXPECT(lag_refused(g, "in_pair_pitch does not cover a plane"));
    g = good_lag(); g.out_pitch = 99; EXPECT(lag_refused(g, "out_pitch smaller than the output's columns"));
    g = good_lag(); g.out_pair_pitch = 199 * 104 + 99; EXPECT(lag_refused(g, "out_pair_pitch does not cover a plane"));
    g = good_lag(); g.axis = 0; g.out_pitch = 199; EXPECT(lag_refused(g, "out_pitch smaller than the output's columns"));       // axis 0: 100 x 200
    g = good_lag(); g.inverse = 1; g.in_pair_pitch = 199 * 100 + 99; EXPECT(lag_refused(g, "in_pair_pitch does not cover a plane"));     // from lag: in is 200 x 100
    g = good_lag(); g.out = const_cast<float*>(g.in) + 29999; EXPECT(lag_refused(g, "out overlaps in"));
    g = good_lag(); g.pad = 3; g.out = const_cast<float*>(g.in); EXPECT(lag_refused(g, "pad must be 0 or 1"));
#else
    (void)good_lag;
#endif

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
