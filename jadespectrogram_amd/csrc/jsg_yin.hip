// libjsg.so, YIN fundamental-frequency tracking (include/jsg.h, section 2i): the difference function by direct evaluation in the time
// domain, the cumulative-mean normalisation, the choice of the lag and its parabolic refinement, in one kernel.  A unit of its own;
// the refusals and the plan of a call are in jsg_yin_host.cpp.
//
// 256 threads (four waves) per workgroup, no scratch, no atomics, no workgroup waits on another.  A work item is (row, F consecutive
// frames); workgroups walk the items with a grid stride.  An item stages the span of its frames into LDS with coalesced loads (the
// contiguous span where hop < w + tau_max, else the frames back to back), then its waves take tiles (frame, block of 64 NL lags):
// lane l of the wave owns the NL lags b + l + 64 q and walks j in the order of the header, j = jb + j0 + 64 jj.  For one j0 it reads
// the 8 samples x[j] (one address for the wave: a broadcast) and the 8 + NL - 1 samples x[jb + j0 + b + l + 64 k] (lane-consecutive
// addresses: conflict-free wherever the frame starts), and they serve 8 NL pairs: 23 LDS reads per 64 pairs at NL = 8.  Each pair is a
// subtraction and a fused multiply-add into the accumulator of its lag.  Lanes whose lag lies past tau_max read on into kYinPad floats
// behind the span and are not stored.  d goes to LDS; after a barrier one wave per frame scans it in groups of 64 lags, turns it into
// d' in place (and stores it to cmnd where asked), keeps the first lag below the threshold and the minimum, walks to the local
// minimum with ballots, and fits the parabola; lane 0 stores f0 and aper.
//
// Every float operation of the definition is written out (contraction is off; the fused multiply-add is explicit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

constexpr int YN_J = 8;                     // samples x[j] a lane has in flight: j0, j0 + 64, ..., j0 + 448
constexpr int YN_BLOCK = 64 * YN_J;

struct YnArgs {
    const float* in;
    long long in_pitch;
    float* f0;
    float* aper;
    long long out_pitch;
    float* cmnd;
    long long cmnd_frame_pitch, cmnd_row_pitch;
    long long n_items;
    int chunks, T, hop, w, tau_min, tau_max, F, S;     // chunks = ceil(T / F) <= T < 2^31
    float threshold, sample_rate;
};

// the pairs of j = j0 + 64 jj (jj < 8) with the NL lags of the lane; y = &x[j0], v = &x[j0 + b + l].  FULL: every j lies below w,
// else those with 64 jj < rem do
template <int NL, bool FULL>
__device__ __forceinline__ void yin_block(const float* y, const float* v, int rem, float (&acc)[NL]) {
#pragma clang fp contract(off)
    float Y[YN_J], V[YN_J + NL - 1];
#pragma unroll
    for (int jj = 0; jj < YN_J; ++jj) Y[jj] = y[64 * jj];
#pragma unroll
    for (int k = 0; k < YN_J + NL - 1; ++k) V[k] = v[64 * k];
#pragma unroll
    for (int jj = 0; jj < YN_J; ++jj) {
        if (FULL || 64 * jj < rem) {
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const float e = Y[jj] - V[jj + q];
                acc[q] = __builtin_fmaf(e, e, acc[q]);
            }
        }
    }
}

template <int NL>
__global__ __launch_bounds__(kYinThreads) void yin_kernel(const YnArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float yn_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = a.w, tau_max = a.tau_max, S = a.S;
    const int span = w + tau_max, row = tau_max + 1;
    float* const dp = yn_lds + (a.F - 1) * S + span + kYinPad;
    const int blocks = (tau_max + 64 * NL - 1) / (64 * NL);
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int r = (int)(item / a.chunks), chunk = (int)(item - (long long)r * a.chunks);
        const int t0 = chunk * a.F;        // < T
        const int Fc = min(a.F, a.T - t0);
        const float* src = a.in + (long long)r * a.in_pitch + (long long)t0 * a.hop;
        const int total = (Fc - 1) * S + span;
        __syncthreads();        // the item before has been read
#pragma unroll 4
        for (int e = tid; e < total; e += kYinThreads) {
            long long m = e;
            if (S != a.hop) {       // frames back to back
                const int fe = e / S;
                m = (long long)fe * a.hop + (e - fe * S);
            }
            yn_lds[e] = src[m];
        }
        __syncthreads();
        for (int tile = wave; tile < Fc * blocks; tile += kYinThreads / 64) {
            const int f = tile / blocks, b = 1 + (tile - f * blocks) * (64 * NL);
            const float* y = yn_lds + f * S;
            const float* v = y + b + lane;
            float acc[NL];
#pragma unroll
            for (int q = 0; q < NL; ++q) acc[q] = 0.f;
            int jb = 0;
            for (; jb + YN_BLOCK <= w; jb += YN_BLOCK)
                for (int j0 = 0; j0 < 64; ++j0) yin_block<NL, true>(y + jb + j0, v + jb + j0, 0, acc);
            const int left = min(64, w - jb);
            for (int j0 = 0; j0 < left; ++j0) yin_block<NL, false>(y + jb + j0, v + jb + j0, w - jb - j0, acc);
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const int tau = b + lane + 64 * q;
                if (tau <= tau_max) dp[f * row + tau] = acc[q];
            }
        }
        __syncthreads();
        for (int f = wave; f < Fc; f += kYinThreads / 64) {
            float* d = dp + f * row;
            float* cm = a.cmnd ? a.cmnd + (long long)r * a.cmnd_row_pitch + (long long)(t0 + f) * a.cmnd_frame_pitch : nullptr;
            float carry = 0.f, best = __builtin_inff();
            int first = INT_MAX, best_tau = INT_MAX;
            bool nan = false;
            if (lane == 0) {
                d[0] = 1.f;
                if (cm) cm[0] = 1.f;
            }
            for (int c0 = 1; c0 <= tau_max; c0 += 64) {
                const int tau = c0 + lane;
                const bool live = tau <= tau_max;
                const float dv = live ? d[tau] : 0.f;
                float s = dv;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const float below = __shfl_up(s, o);
                    if (lane >= o) s = s + below;
                }
                s = carry + s;
                carry = __shfl(s, 63);
                const float scaled = dv * (float)tau;
                const float q = s == 0.f ? 1.f : scaled / s;
                if (live) {
                    d[tau] = q;
                    if (cm) cm[tau] = q;
                }
                const bool in_range = live && tau >= a.tau_min;
                nan = nan || (in_range && q != q);
                const unsigned long long under = __ballot(in_range && q < a.threshold);
                if (first == INT_MAX && under) first = c0 + __builtin_ctzll(under);
                if (in_range && q < best) {
                    best = q;
                    best_tau = tau;
                }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const float ob = __shfl_xor(best, o);
                const int ot = __shfl_xor(best_tau, o);
                if (ob < best || (ob == best && ot < best_tau)) {
                    best = ob;
                    best_tau = ot;
                }
            }
            const bool any_nan = __any(nan);
            __threadfence_block();              // d' of the other lanes is read below
            __builtin_amdgcn_wave_barrier();
            int tau = first != INT_MAX ? first : best_tau != INT_MAX ? best_tau : a.tau_min;
            if (first != INT_MAX) {
                for (;;) {
                    const int t = tau + lane;
                    const bool down = t + 1 <= tau_max && d[t + 1] < d[t];
                    const unsigned long long m = __ballot(down);
                    const int steps = ~m ? __builtin_ctzll(~m) : 64;
                    tau += steps;
                    if (steps < 64) break;
                }
            }
            if (lane == 0) {
                const float bq = d[tau];
                float s = 0.f;
                if (tau + 1 <= tau_max) {
                    const float aq = d[tau - 1], cq = d[tau + 1];
                    const float den = (aq - bq) + (cq - bq);
                    if (den > 0.f) {
                        const float num = 0.5f * (aq - cq);
                        s = num / den;
                        if (!(__builtin_fabsf(s) <= 1.f)) s = 0.f;
                    }
                }
                const float period = (float)tau + s;
                const float nanv = __builtin_nanf("");
                const long long at = (long long)r * a.out_pitch + t0 + f;
                if (a.f0) a.f0[at] = any_nan ? nanv : a.sample_rate / period;
                if (a.aper) a.aper[at] = any_nan ? nanv : bq;
            }
        }
    }
}

}  // namespace jsg

using namespace jsg;

extern "C" int jsg_yin_launch(const jsg_yin_args* g, void* stream) {
    static const char* who = "jsg_yin_launch";
    int dev = -1;
    int rc = yin_check(g, who);
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    YinPlan p{};
    yin_resolve(g, &p);
    YnArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.in_pitch = multi ? g->in_pitch : 0;
    k.f0 = g->f0;
    k.aper = g->aper;
    k.out_pitch = multi ? g->out_pitch : 0;
    k.cmnd = g->cmnd;
    k.cmnd_frame_pitch = g->cmnd_frame_pitch;
    k.cmnd_row_pitch = multi ? g->cmnd_row_pitch : 0;
    k.n_items = (long long)g->rows * p.chunks;
    k.chunks = (int)p.chunks;
    k.T = (int)g->n_frames;
    k.hop = (int)g->hop;
    k.w = g->window;
    k.tau_min = g->tau_min;
    k.tau_max = g->tau_max;
    k.F = p.F;
    k.S = p.S;
    k.threshold = g->threshold;
    k.sample_rate = g->sample_rate;
    const size_t lds_bytes = sizeof(float) * (size_t)p.lds_floats;
    const dim3 grid(resident_grid(k.n_items, dev, per_cu_by_lds(kYinLdsOne, p.lds_floats, 8)));      // 2048 threads per compute unit
    static void (*const kernels[4])(YnArgs) = {yin_kernel<1>, yin_kernel<2>, yin_kernel<4>, yin_kernel<8>};      // the code object holds them in this order
    const int path = p.NL == 1 ? 0 : p.NL == 2 ? 1 : p.NL == 4 ? 2 : 3;
    static OncePerDevice told;      // a bit per path
    const hipError_t err = launch_large_lds(told, dev, 1u << path, kernels[path], kYinLdsOne * 4, grid, dim3(kYinThreads), lds_bytes, reinterpret_cast<hipStream_t>(stream), k);
    return err == hipSuccess ? JSG_OK : jsg_fail_hip(err, who);
}
