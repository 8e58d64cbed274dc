// CPU check of the two-population grid of the 1024-point runs kernel (csrc/jsg_runs_grid.h): every (block, step) of the partition is walked
// with the kernel's own index arithmetic (stft_db_kernel STREAM == 2: XCD remap, runs_group) for a spread of launch sizes and CU counts.
//   - every super-group is covered, - only steps of the fill wrap, - a wrapped step lands on a real group of the fill's range,
//   - n_long is a multiple of 256 and the XCD remap maps [0, n_long) onto itself, - nblk <= 2^20.
#include <cstdio>
#include <vector>

#include "jsg_runs_grid.h"

static int g_bad = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (++g_bad <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                               \
    } while (0)

// stft_db_kernel's block remap (chunks of 32 workgroups per XCD)
static unsigned remap(unsigned b, unsigned nblk) {
    const unsigned CL = 5, xcd = b & 7, jb = b >> 3, full = nblk & ~255u;
    if (b < full && b < (nblk & ~((8u << CL) - 1u))) return ((jb >> CL) << (CL + 3)) + (xcd << CL) + (jb & ((1u << CL) - 1u));
    if (b < full) return b;
    const unsigned t = nblk - full, q = t >> 3, r = t & 7;
    return full + (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + ((b - full) >> 3);
}

static long long g_cases = 0;

static void walk(long long want, int n_cu, int fill16, int its) {
    jsg::RunsGrid rg{};
    const bool two = jsg::runs_two_populations(want, n_cu, fill16, its, &rg);
    const long long thr = jsg::runs_two_pop_threshold(n_cu);
    CHECK(two == (thr > 0 && want >= thr && want <= (1ll << 20)), "want %lld n_cu %d: form %d, threshold %lld", want, n_cu, int(two), thr);
    if (!two) return;
    ++g_cases;
    const unsigned n_groups = unsigned(want);
    CHECK(rg.n_long % 256 == 0 && rg.n_long > 0, "n_long %u", rg.n_long);
    CHECK(rg.n_long <= unsigned(jsg::kRunsResidentPerCu * n_cu), "n_long %u is more than one resident generation of %d CUs", rg.n_long, n_cu);
    CHECK(rg.nblk <= (1u << 20) && rg.nblk > rg.n_long, "nblk %u", rg.nblk);
    CHECK(rg.it_long >= 1 && rg.it_short == its, "steps %d / %d", rg.it_long, rg.it_short);
    CHECK(rg.g0 == rg.n_long * unsigned(rg.it_long) && rg.g0 < n_groups, "g0 %u", rg.g0);
    CHECK((long long)(n_groups - rg.g0) * 16 >= want * fill16, "the fill holds %u of %lld steps, less than %d/16", n_groups - rg.g0, want, fill16);
    std::vector<unsigned char> cover(n_groups, 0), seen(rg.nblk, 0);
    long long wrapped = 0;
    for (unsigned b = 0; b < rg.nblk; ++b) {
        const unsigned lb = remap(b, rg.nblk);
        CHECK(lb < rg.nblk && !seen[lb < rg.nblk ? lb : 0], "remap: block %u -> %u", b, lb);
        if (lb >= rg.nblk) continue;
        seen[lb] = 1;
        CHECK((b < rg.n_long) == (lb < rg.n_long), "remap takes block %u across the populations (-> %u)", b, lb);
        // the kernel's scalars (rg_fill, rg_base, rg_stride, rg_iters) from StftKArgs pop_nl, pop_g0, pop_iters, iters and nblk
        const bool fill = lb >= rg.n_long;
        const unsigned base = fill ? rg.g0 + (lb - rg.n_long) : lb, stride = fill ? rg.nblk - rg.n_long : rg.n_long;
        const int iters = fill ? rg.it_short : rg.it_long;
        for (int sg = 0; sg < iters; ++sg) {
            unsigned g = base + unsigned(sg) * stride;
            if (g >= n_groups) {
                CHECK(fill, "a bulk step wraps: block %u step %d", lb, sg);
                g = g - n_groups + rg.g0;
                ++wrapped;
                CHECK(g >= rg.g0, "wrapped step outside the fill's range: %u", g);
            }
            CHECK(g < n_groups, "block %u step %d -> group %u of %u", lb, sg, g, n_groups);
            if (g < n_groups) {
                CHECK(fill == (g >= rg.g0), "block %u (fill %d) step %d in the other population's range: %u", lb, int(fill), sg, g);
                if (cover[g] < 255) ++cover[g];
            }
        }
    }
    CHECK(wrapped < its, "%lld surplus steps with %d steps per fill block", wrapped, its);
    long long twice = 0;
    for (unsigned g = 0; g < n_groups; ++g) {
        CHECK(cover[g] >= 1, "group %u not covered (want %lld n_cu %d fill %d/16 its %d)", g, want, n_cu, fill16, its);
        CHECK(cover[g] <= 2 && (cover[g] == 1 || g >= rg.g0), "group %u covered %d times", g, int(cover[g]));
        twice += cover[g] == 2;
    }
    CHECK(twice == wrapped, "%lld groups stored twice, %lld wrapped steps", twice, wrapped);
}

int main() {
    const int cus[] = {8, 64, 256, 304};
    for (int n_cu : cus) {
        const long long thr = jsg::runs_two_pop_threshold(n_cu);
        CHECK((n_cu == 8) == (thr == 0), "n_cu %d: threshold %lld", n_cu, thr);
        std::vector<long long> wants = {1, 255, 1279, 1280, 8191, 8192, 8193, 10007, 65521, 99991, 262144, 1048573, 1ll << 20, (1ll << 20) + 1};
        for (long long d = -3; d <= 3; ++d)
            if (thr + d > 0) wants.push_back(thr + d);
        for (long long w : wants)
            for (int fill16 : {1, 2, 3, 4})
                for (int its : {1, 2, 4}) walk(w, n_cu, fill16, its);
    }
    // the C2 dispatch and the C4 shard on 256 CUs with the product's setting
    jsg::RunsGrid rg{};
    CHECK(jsg::runs_two_populations(32768, 256, JSG_X_POP_FILL16, JSG_X_POP_ITS, &rg) && rg.n_long == 1280, "C2: n_long %u", rg.n_long);
    std::printf("{\"cases\": %lld, \"bad\": %d}\n", g_cases, g_bad);
    return g_bad ? 1 : (g_cases >= 300 ? 0 : 3);
}
