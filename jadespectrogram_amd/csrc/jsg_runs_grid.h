// The grid of a strided launch of the 1024-point "runs" kernel (stft_db_kernel STREAM == 2) as TWO POPULATIONS of workgroups in one launch.
// Plain C++ (no HIP): stft_launch_impl uses it, and tests/cpp/runs_grid_test.cpp walks every (block, step) of it on the CPU.
//
// A launch is `want` workgroup steps (super-groups of TPB * kRunLen columns).  The uniform grid gives every workgroup the same few steps
// (32 workgroups per CU: 6.4 generations of resident workgroups on a C2 dispatch, each paying its tables and its first frame's round trip).
// Here the first n_long blocks -- one resident generation, handed out first -- are the BULK: block lb walks it_long steps
// g = lb + sg * n_long of the super-groups [0, g0).  The blocks behind them are the FILL: short-lived (it_short steps), they queue behind the
// bulk, are handed out as bulk workgroups finish and cover the rest, g = g0 + (lb - n_long) + sg * n_short; the surplus steps of the last
// round start over with the first groups of the fill's range (the same bits stored twice, as in the uniform grid).
// n_long is a multiple of 256, so the XCD remap of stft_db_kernel maps [0, n_long) onto itself.
#pragma once

namespace jsg {

struct RunsGrid {
    unsigned nblk;     // workgroups of the launch = n_long + n_short
    unsigned n_long;   // bulk blocks [0, n_long)
    unsigned g0;       // first super-group of the fill = n_long * it_long
    int it_long;       // steps of a bulk block
    int it_short;      // steps of a fill block
};

constexpr int kRunsResidentPerCu = 5;      // four-wave workgroups of the runs kernel resident on a CU (five waves per SIMD)
constexpr int kRunsTwoPopulations = 1;     // the product's default: 1 = strided launches of the runs kernel take the two-population form
constexpr int kRunsPopMinGenerations = 4;  // the two-population form starts at this many resident generations of steps
#ifndef JSG_X_POP_FILL16
#define JSG_X_POP_FILL16 2                 // share of the steps left to the fill, in sixteenths (variant builds sweep it)
#endif
#ifndef JSG_X_POP_ITS
#define JSG_X_POP_ITS 2                    // steps of a fill block
#endif

// smallest `want` that takes the two-population form on a device of n_cu CUs (0: never -- fewer than 256 resident workgroups)
inline long long runs_two_pop_threshold(int n_cu) {
    const long long nl = ((long long)kRunsResidentPerCu * n_cu) & ~255ll;
    return nl * kRunsPopMinGenerations;
}

// The partition of `want` steps; false: the launch keeps the uniform grid (too small, or no whole 256 resident workgroups).
inline bool runs_two_populations(long long want, int n_cu, int fill16, int it_short, RunsGrid* out, int min_generations = kRunsPopMinGenerations) {
    const long long nl = ((long long)kRunsResidentPerCu * n_cu) & ~255ll;
    if (nl <= 0 || fill16 < 1 || fill16 > 8 || it_short < 1 || min_generations < 2 ||
        want < nl * min_generations || want > (1ll << 20))
        return false;
    long long fill = (want * fill16 + 15) / 16;
    if (fill < it_short) fill = it_short;   // (so that a wrapped step finds a group of the fill's own range)
    const long long it_long = (want - fill) / nl;
    if (it_long < 1) return false;
    const long long g0 = nl * it_long, n_fill = want - g0, ns = (n_fill + it_short - 1) / it_short;
    out->nblk = unsigned(nl + ns);
    out->n_long = unsigned(nl);
    out->g0 = unsigned(g0);
    out->it_long = int(it_long);
    out->it_short = it_short;
    return true;
}

}  // namespace jsg
