// L (jsgx::log_pos of csrc/jsgx_internal.h, include/jsgx.h section 5b) against log in double over EVERY float32 in (0, 1]: the largest
// |L(x) - ln x| / max(1, |ln x|), where it is, and the largest error in ulps of the result.  Host only; tools/pyin_accuracy.py builds
// and runs it (-O2 -ffp-contract=off) and writes profiles/pyin_accuracy.md from its output.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "jsgx_internal.h"

struct Worst {
    double err = 0.0, ulps = 0.0;
    uint32_t at = 0, ulps_at = 0;
    uint64_t count = 0;
};

static void sweep(uint32_t first, uint32_t last, Worst* out) {      // bit patterns first..last inclusive
    Worst w;
    for (uint64_t b = first; b <= last; ++b) {
        float x;
        const uint32_t bits = (uint32_t)b;
        std::memcpy(&x, &bits, 4);
        const double got = jsgx::log_pos(x), want = std::log((double)x);
        const double scale = std::fabs(want) > 1.0 ? std::fabs(want) : 1.0;
        const double err = std::fabs(got - want) / scale;
        if (err > w.err) w.err = err, w.at = bits;
        if (want != 0.0) {
            int e;
            std::frexp(want, &e);
            const double ulps = std::fabs(got - want) / std::ldexp(1.0, e - 24);
            if (ulps > w.ulps) w.ulps = ulps, w.ulps_at = bits;
        }
        ++w.count;
    }
    *out = w;
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 8;
    const uint32_t lo = 1, hi = 0x3f800000u;        // the smallest denormal .. 1.0f
    std::vector<Worst> parts(n);
    std::vector<std::thread> pool;
    const uint64_t span = (uint64_t)hi - lo + 1;
    for (int i = 0; i < n; ++i)
        pool.emplace_back(sweep, (uint32_t)(lo + span * i / n), (uint32_t)(lo + span * (i + 1) / n - 1), &parts[i]);
    for (auto& t : pool) t.join();
    Worst w;
    for (const Worst& p : parts) {
        if (p.err > w.err) w.err = p.err, w.at = p.at;
        if (p.ulps > w.ulps) w.ulps = p.ulps, w.ulps_at = p.ulps_at;
        w.count += p.count;
    }
    float x, y;
    std::memcpy(&x, &w.at, 4);
    std::memcpy(&y, &w.ulps_at, 4);
    std::printf("count %llu\nworst_scaled %.6e at 0x%08x (%.9g)\nworst_ulps %.4f at 0x%08x (%.9g)\n", (unsigned long long)w.count, w.err, w.at, (double)x, w.ulps,
                w.ulps_at, (double)y);
    return 0;
}
