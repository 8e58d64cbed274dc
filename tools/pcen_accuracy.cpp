// E and L of include/jsgx.h section 13 (jsgx::exp_any and jsgx::log_pos of csrc/jsgx_internal.h, the shipped routines) against exp and log
// in double over EVERY float32 of their ranges: E over [-87, 88.72] (relative error), L over every positive finite float32, subnormals
// included (|L(x) - ln x| / max(1, |ln x|), the measure of JSGX_LOG_ABS_BOUND); and the bits of E against the routine of section 1 as it
// was before section 13 (one product by 2^n) over every float32 in [-87, 0].  Host arithmetic only: the routines are stated operation by
// operation and the device gives the same bits (tests/test_gpu_pcen.py), so the error is a property of the statement.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -march=native -pthread -I include -I jadespectrogram_amd/csrc tools/pcen_accuracy.cpp -o pcen_accuracy
//   ./pcen_accuracy            (prints the tables of profiles/pcen_accuracy.md; tools/pcen_accuracy.py runs it)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <thread>
#include <vector>

#include "jsgx_internal.h"

namespace {
struct Worst {
    double err = 0;
    float at = 0;
    uint64_t count = 0, differ = 0;
};

// section 1's routine as it stood: the scale is one factor
float exp_one_factor(float x) {
    if (x < -87.0f) return 0.f;
    const float n = __builtin_floorf(__builtin_fmaf(x, 1.44269502162933349609375f, 0.5f));
    float r = __builtin_fmaf(n, -0.693145751953125f, x);
    r = __builtin_fmaf(n, -1.42860676533018704503775e-06f, r);
    float p = 1.984127011382952332496643e-04f;
    for (float c : {1.388888922519981861114502e-03f, 8.333333767950534820556641e-03f, 4.166666790843009948730469e-02f, 1.666666716337203979492188e-01f, 0.5f, 1.0f, 1.0f})
        p = __builtin_fmaf(p, r, c);
    return p * jsgx::float_of_bits((unsigned)((int)n + 127) << 23);
}

double exp_error(float x, Worst& w) {
    const float got = jsgx::exp_any(x);
    if (x <= 0.f && jsgx::bits_of_float(got) != jsgx::bits_of_float(exp_one_factor(x))) ++w.differ;
    const double want = std::exp((double)x);
    return std::fabs((double)got - want) / want;
}
double log_error(float x, Worst&) {
    const double want = std::log((double)x), size = std::fabs(want) > 1.0 ? std::fabs(want) : 1.0;
    return std::fabs((double)jsgx::log_pos(x) - want) / size;
}

// the bit patterns first..last (floats of one sign, ascending in magnitude) among 16 threads
Worst sweep(uint32_t first, uint32_t last, double (*error)(float, Worst&)) {
    const unsigned n_threads = 16;
    std::vector<Worst> part(n_threads);
    std::vector<std::thread> pool;
    const uint64_t total = (uint64_t)last - first + 1;
    for (unsigned t = 0; t < n_threads; ++t) {
        const uint64_t a = first + total * t / n_threads, b = first + total * (t + 1) / n_threads;
        pool.emplace_back([&part, t, a, b, error] {
            Worst& w = part[t];
            for (uint64_t bits = a; bits < b; ++bits) {
                const float x = jsgx::float_of_bits((unsigned)bits);
                const double e = error(x, w);
                if (e > w.err) w.err = e, w.at = x;
                ++w.count;
            }
        });
    }
    for (auto& th : pool) th.join();
    Worst w;
    for (const Worst& p : part) {
        if (p.err > w.err) w.err = p.err, w.at = p.at;
        w.count += p.count, w.differ += p.differ;
    }
    return w;
}

struct Band {
    const char* name;
    uint32_t first, last;
};

Worst table(const char* title, const char* measure, const std::vector<Band>& bands, double (*error)(float, Worst&), const char* all_name) {
    std::printf("%s\n\n| range of x | float32 values | %s | at x |\n|---|---|---|---|\n", title, measure);
    Worst all;
    for (const Band& band : bands) {
        const Worst w = sweep(band.first, band.last, error);
        std::printf("| %s | %llu | %.3e | %.9g |\n", band.name, (unsigned long long)w.count, w.err, (double)w.at);
        if (w.err > all.err) all.err = w.err, all.at = w.at;
        all.count += w.count, all.differ += w.differ;
    }
    std::printf("| %s | %llu | %.3e | %.9g |\n\n", all_name, (unsigned long long)all.count, all.err, (double)all.at);
    return all;
}
}  // namespace

int main() {
    using jsgx::bits_of_float;
    const std::vector<Band> exp_bands = {{"[-87, -1)", bits_of_float(-1.0f) + 1, bits_of_float(-87.0f)},
                                         {"[-1, -0] (denormals included)", 0x80000000u, bits_of_float(-1.0f)},
                                         {"[+0, 1) (denormals included)", 0u, bits_of_float(1.0f) - 1},
                                         {"[1, 64)", bits_of_float(1.0f), bits_of_float(64.0f) - 1},
                                         {"[64, 88.72]", bits_of_float(64.0f), bits_of_float(88.72f)}};
    const Worst e = table("E against `exp` in double over every float32 in [-87, 88.72] (the shipped routine, `jsgx::exp_any`):", "worst relative error", exp_bands,
                          exp_error, "[-87, 88.72], all");
    std::printf("JSGX_EXP_REL_BOUND = %.1e: %s.  Over every float32 in [-87, 0] the bits of E differ from section 1's one-factor routine at %llu values.\n\n",
                (double)JSGX_EXP_REL_BOUND, e.err <= JSGX_EXP_REL_BOUND ? "holds over the whole range" : "EXCEEDED", (unsigned long long)e.differ);
    const std::vector<Band> log_bands = {{"subnormals, (0, 2^-126)", 1u, 0x007fffffu},
                                         {"[2^-126, 2^-10)", 0x00800000u, bits_of_float(0.0009765625f) - 1},
                                         {"[2^-10, 1)", bits_of_float(0.0009765625f), bits_of_float(1.0f) - 1},
                                         {"[1, 2^10)", bits_of_float(1.0f), bits_of_float(1024.0f) - 1},
                                         {"[2^10, the largest float32]", bits_of_float(1024.0f), 0x7f7fffffu}};
    const Worst l = table("L against `log` in double over every positive finite float32 (the shipped routine, `jsgx::log_pos`):", "worst abs. error / max(1, abs(ln x))",
                          log_bands, log_error, "every positive float32");
    std::printf("JSGX_LOG_ABS_BOUND = %.1e: %s.\n", (double)JSGX_LOG_ABS_BOUND, l.err <= JSGX_LOG_ABS_BOUND ? "holds over the whole range" : "EXCEEDED");
    return e.err <= JSGX_EXP_REL_BOUND && l.err <= JSGX_LOG_ABS_BOUND && e.differ == 0 ? 0 : 1;
}
