// jsgx_exp (include/jsgx.h section 1, jsgx_internal.h exp_neg) against exp in double over EVERY float32 in [-87, 0]: the arguments the
// affinity mode of jsgx_recurrence_launch can meet (section 7).  Host arithmetic only: the routine is stated operation by operation and
// the device gives the same bits (tests/test_gpu_knn.py, tests/test_gpu_beat.py), so the error is a property of the statement.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -march=native -pthread -I include -I jadespectrogram_amd/csrc tools/knn_exp_accuracy.cpp -o knn_exp_accuracy
//   ./knn_exp_accuracy            (prints the markdown of profiles/knn_accuracy.md)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "jsgx_internal.h"

namespace {
struct Worst {
    double rel = 0;
    float at = 0;
    uint64_t count = 0;
};

Worst scan(uint32_t first, uint32_t last) {      // bit patterns of negative floats, ascending in magnitude
    Worst w;
    for (uint64_t b = first; b <= last; ++b) {
        const float x = jsgx::float_of_bits((unsigned)b);
        const double want = std::exp((double)x), got = (double)jsgx::exp_neg(x);
        const double rel = std::fabs(got - want) / want;
        if (rel > w.rel) {
            w.rel = rel;
            w.at = x;
        }
        ++w.count;
    }
    return w;
}
}  // namespace

int main() {
    const uint32_t lo = 0x80000000u, hi = jsgx::bits_of_float(-87.0f);        // -0 .. -87
    const unsigned n_threads = 16;
    // bands: [-2^e, -2^(e+1)) by exponent, and the whole; each band split among the threads
    struct Band {
        const char* name;
        uint32_t first, last;
    };
    const std::vector<Band> bands = {{"[-87, -64)", jsgx::bits_of_float(-64.0f) + 1, hi},
                                     {"[-64, -8)", jsgx::bits_of_float(-8.0f) + 1, jsgx::bits_of_float(-64.0f)},
                                     {"[-8, -1)", jsgx::bits_of_float(-1.0f) + 1, jsgx::bits_of_float(-8.0f)},
                                     {"[-1, -2^-10)", jsgx::bits_of_float(-0.0009765625f) + 1, jsgx::bits_of_float(-1.0f)},
                                     {"[-2^-10, -0] (denormals included)", lo, jsgx::bits_of_float(-0.0009765625f)}};
    std::printf("| range of x | float32 values | worst relative error | at x |\n|---|---|---|---|\n");
    Worst all;
    for (const Band& band : bands) {
        std::vector<Worst> part(n_threads);
        std::vector<std::thread> pool;
        const uint64_t total = (uint64_t)band.last - band.first + 1;
        for (unsigned t = 0; t < n_threads; ++t) {
            const uint64_t a = band.first + total * t / n_threads, b = band.first + total * (t + 1) / n_threads;
            pool.emplace_back([&part, t, a, b] {
                if (b > a) part[t] = scan((uint32_t)a, (uint32_t)(b - 1));
            });
        }
        for (auto& th : pool) th.join();
        Worst w;
        for (const Worst& p : part) {
            if (p.rel > w.rel) {
                w.rel = p.rel;
                w.at = p.at;
            }
            w.count += p.count;
        }
        std::printf("| %s | %llu | %.3e | %.9g |\n", band.name, (unsigned long long)w.count, w.rel, (double)w.at);
        if (w.rel > all.rel) {
            all.rel = w.rel;
            all.at = w.at;
        }
        all.count += w.count;
    }
    std::printf("| [-87, 0], all | %llu | %.3e | %.9g |\n", (unsigned long long)all.count, all.rel, (double)all.at);
    std::printf("\nJSGX_EXP_REL_BOUND = %.1e: %s\n", (double)JSGX_EXP_REL_BOUND, all.rel <= JSGX_EXP_REL_BOUND ? "holds over the whole range" : "EXCEEDED");
    return 0;
}
