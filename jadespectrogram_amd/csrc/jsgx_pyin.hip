// libjsgx.so, pYIN (include/jsgx.h section 5): the observation kernel, the factored forward kernel of the decoder and their launchers.
// The refusals, the plans and the table builders are in jsgx_pyin_host.cpp; the backtrace is section 4's (jsgx_viterbi.hip).
//
// pyin_observe_kernel.  One wavefront per frame, nobody waits for anybody.  The frame's d' goes to LDS once; the lanes mark the troughs
// and pack their lags in ascending order with a ballot; a lane owns the thresholds k = l, l + 64, l + 128, l + 192 and counts the
// troughs below each (n_k); then the troughs are met in ascending lag order, every lane adds its thresholds' terms with the running
// rank of the trough among those below the threshold, and an xor tree over the lanes gives the trough's probability.  Periods and bins
// are a lane per trough (a binary search in the descending table of period edges), the sums into obs are one lane in lag order, and
// the logarithms are a lane per bin.
//
// pyin_forward_kernel.  One workgroup per sequence from frame 0 to T-1.  The transition is Tp(p, p') Ts(u, u'), so the maximum over the
// sources of (u', p') is max over u of (switch(u, u') + max over p of (U[u][p] + window[p' - p + W])) with U[u][p] = V[t-1][uP + p] +
// src_offset[p]: the inner maxima m_0 and m_1 are taken once per p' and serve both u'.  U of both u lies in LDS in two copies swapped by
// the parity of t, each row padded by W words of -inf at both ends, so that the inner loop has neither a bounds test nor a table row
// per destination: the window of 2W + 1 words is all it reads besides U.  G lanes of a wavefront share a p' and split the offsets
// (the plan's rule keeps eight offsets or more per lane and the workgroup within 512 lanes where it splits at all: measured); the
// pair rule of section 4 joins them.  U is kept as pairs (U[0][p], U[1][p]) read 8 bytes at a time.  U of frame t is written where
// V[t] is, so a frame costs one barrier, and the emissions of frame t + 1 are loaded before frame t computes.
#include <hip/hip_runtime.h>

#include <climits>

#include "jsgx_internal.h"

namespace jsgx {

// How the forward kernel keeps and reads U (profiles/pyin_bench.md has the three measured side by side; tools/pyin_bench.py builds the others):
//   0  two rows per copy, U[0][.] and U[1][.]; the offsets of u = 0, then those of u = 1
//   1  the same rows; one pass over the offsets serves both u, so a window word is read once
//   2  one row of pairs (U[0][p], U[1][p]) per copy, read 8 bytes at a time; one pass over the offsets
#ifndef JSGX_PYIN_LOOP
#define JSGX_PYIN_LOOP 2
#endif

constexpr int kObserveThreads = JSGX_PYIN_OBSERVE_THREADS;
constexpr int kThresholdsPerLane = JSGX_PYIN_MAX_THRESHOLDS / kObserveThreads;
constexpr int kDecodeThreads = JSGX_PYIN_THREADS;
static_assert(kObserveThreads == 64 && kThresholdsPerLane == 4, "a wavefront per frame, four thresholds per lane");
static_assert(JSGX_PYIN_MAX_BINS <= kDecodeThreads && 2 * JSGX_PYIN_MAX_BINS <= 65536, "a lane per pitch bin at the least; psi is uint16");
static_assert(4 * (JSGX_PYIN_MAX_LAG + 1 + 3 * (JSGX_PYIN_MAX_LAG / 2 + 1) + JSGX_PYIN_MAX_BINS) <= 65536, "the observation kernel's LDS needs no opt-in");
static_assert(4 * (4 * (JSGX_PYIN_MAX_BINS + 2 * JSGX_PYIN_MAX_BAND_HALF) + 2 * JSGX_PYIN_MAX_BAND_HALF + 1) <= 65536, "the forward kernel's LDS needs no opt-in");

struct ObserveArgs {
    const float* cmnd;
    long long cmnd_frame_pitch, cmnd_row_pitch;
    const float* prior;
    const float* decay;
    const float* norm;
    const float* edges;
    int tau_min, tau_max, N, P, max_troughs;
    float no_trough_prob;
    float* log_emit;
    long long emit_frame_pitch, emit_row_pitch;
    float* obs;
    long long obs_frame_pitch, obs_row_pitch;
    float* voiced;
    long long voiced_pitch;
};

// the sum over the 64 lanes as the halving tree of the header: every lane ends with acc_0 (the additions are commutative)
__device__ __forceinline__ float wave_sum(float v) {
#pragma clang fp contract(off)
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(kObserveThreads) void pyin_observe_kernel(ObserveArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int l = threadIdx.x;
    const long long t = blockIdx.x, r = blockIdx.y;
    const int tau_min = a.tau_min, tau_max = a.tau_max, N = a.N, P = a.P;
    float* h = lds;                                                    // [tau_max + 1]
    int* lag = reinterpret_cast<int*>(lds + tau_max + 1);              // [max_troughs + 1] each
    float* prob = reinterpret_cast<float*>(lag + a.max_troughs + 1);
    int* bin = reinterpret_cast<int*>(prob + a.max_troughs + 1);
    float* obs = reinterpret_cast<float*>(bin + a.max_troughs + 1);    // [P]
    const float* src = a.cmnd + r * a.cmnd_row_pitch + t * a.cmnd_frame_pitch;
    float* emit = a.log_emit + r * a.emit_row_pitch + t * a.emit_frame_pitch;
    float* obs_out = a.obs ? a.obs + r * a.obs_row_pitch + t * a.obs_frame_pitch : nullptr;
    const float minus_inf = -__builtin_inff();

    bool nan = false;
    for (int tau = l; tau <= tau_max; tau += kObserveThreads) {
        const float v = src[tau];
        h[tau] = v;
        nan |= tau >= tau_min && v != v;
    }
    for (int b = l; b < P; b += kObserveThreads) obs[b] = 0.f;
    __syncthreads();
    if (__any(nan)) {           // the frame is unobserved
        const float unv = log_pos(1.0f / (float)P);
        for (int b = l; b < P; b += kObserveThreads) {
            emit[b] = minus_inf;
            emit[P + b] = unv;
            if (obs_out) obs_out[b] = 0.f;
        }
        if (a.voiced && l == 0) a.voiced[r * a.voiced_pitch + t] = __builtin_nanf("");
        return;
    }

    // the troughs, their lags packed in ascending order
    int n_troughs = 0;
    for (int base = tau_min; base < tau_max; base += kObserveThreads) {
        const int tau = base + l;
        bool is = false;
        if (tau < tau_max) is = tau == tau_min ? h[tau] < h[tau + 1] : (h[tau - 1] > h[tau] && h[tau] <= h[tau + 1]);
        const unsigned long long mask = __ballot(is);
        if (is) lag[n_troughs + __popcll(mask & ((1ull << l) - 1))] = tau;
        n_troughs += __popcll(mask);
    }
    __syncthreads();

    // the thresholds of this lane; n_k, the troughs below each
    float th[kThresholdsPerLane], pr[kThresholdsPerLane];
    int n_below[kThresholdsPerLane], rank[kThresholdsPerLane];
#pragma unroll
    for (int i = 0; i < kThresholdsPerLane; ++i) {
        const int k = l + kObserveThreads * i;
        th[i] = (float)((double)(k + 1) / (double)N);
        pr[i] = k < N ? a.prior[k] : 0.f;
        n_below[i] = rank[i] = 0;
    }
    for (int j = 0; j < n_troughs; ++j) {
        const float hj = h[lag[j]];
#pragma unroll
        for (int i = 0; i < kThresholdsPerLane; ++i) n_below[i] += l + kObserveThreads * i < N && hj < th[i];
    }
    float nk[kThresholdsPerLane];
#pragma unroll
    for (int i = 0; i < kThresholdsPerLane; ++i) nk[i] = a.norm[n_below[i]];        // n_below <= max_troughs <= boltz_len; norm has boltz_len + 1 words

    // the probability of every trough, in ascending lag order; the lowest trough on the way
    float lowest = 0.f;
    int lowest_j = -1;
    for (int j = 0; j < n_troughs; ++j) {
        const float hj = h[lag[j]];
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < kThresholdsPerLane; ++i) {
            const bool below = l + kObserveThreads * i < N && hj < th[i];
            float term = 0.f;
            if (below) term = pr[i] * (nk[i] * a.decay[rank[i]]);                  // rank < n_below <= boltz_len
            acc = acc + term;
            rank[i] += below;
        }
        acc = wave_sum(acc);
        if (l == 0) prob[j] = acc;
        if (lowest_j < 0 || hj < lowest) {
            lowest = hj;
            lowest_j = j;
        }
    }
    if (lowest_j >= 0) {        // uniform over the wavefront
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < kThresholdsPerLane; ++i) {
            float term = 0.f;
            if (l + kObserveThreads * i < N && !(lowest < th[i])) term = pr[i];
            acc = acc + term;
        }
        acc = wave_sum(acc);
        if (l == 0) prob[lowest_j] = prob[lowest_j] + a.no_trough_prob * acc;
    }

    // period and bin, a lane per trough
    for (int j = l; j < n_troughs; j += kObserveThreads) {
        const int tau = lag[j];                                                   // tau_min <= tau < tau_max, tau_min >= 1
        const float ya = h[tau - 1], yb = h[tau], yc = h[tau + 1];
        const float den = (ya - yb) + (yc - yb);
        float s = 0.f;
        if (den > 0.f) {
            s = (0.5f * (ya - yc)) / den;
            if (!(__builtin_fabsf(s) <= 1.0f)) s = 0.f;
        }
        const float period = (float)tau + s;
        // the number of b in 1..P-1 with period <= edges[b]: the table descends, so these are the first ones
        int lo = 0, hi = P - 1;               // the count lies in lo..hi
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;         // 1..P-1
            if (period <= a.edges[mid]) lo = mid;
            else hi = mid - 1;
        }
        bin[j] = lo;
    }
    __syncthreads();
    if (l == 0)
        for (int j = 0; j < n_troughs; ++j) obs[bin[j]] = obs[bin[j]] + prob[j];
    __syncthreads();

    float acc = 0.f;
    for (int b = l; b < P; b += kObserveThreads) acc = acc + obs[b];
    acc = wave_sum(acc);
    const float voiced = acc > 1.0f ? 1.0f : acc;
    const float unv = log_pos((1.0f - voiced) / (float)P);
    for (int b = l; b < P; b += kObserveThreads) {
        const float o = obs[b];
        emit[b] = log_pos(o);
        emit[P + b] = unv;
        if (obs_out) obs_out[b] = o;
    }
    if (a.voiced && l == 0) a.voiced[r * a.voiced_pitch + t] = voiced;
}

struct DecodeArgs {
    const float* emit;
    long long emit_frame_pitch, emit_seq_pitch;
    const float* init;
    const float* log_window;
    const float* src_offset;
    const float* log_switch;
    int P, T, W, G;
    unsigned short* psi;            // [seqs][T][2P]; row 0 is not written
    float* vlast;                   // [seqs][2P]: V[T-1]
    float* value;                   // or null
    long long value_frame_pitch, value_seq_pitch;
};

// the word of U[copy][u][pp] in LDS, pp = W + p the place in the padded row of `row` words
__device__ __forceinline__ int u_word(int copy, int u, int pp, int row) { return JSGX_PYIN_LOOP == 2 ? (copy * row + pp) * 2 + u : (2 * copy + u) * row + pp; }

// the pair rule of include/jsgx.h section 4: (w, i) beats (best, best_i)
__device__ __forceinline__ bool beats(float w, int i, float best, int best_i) { return w > best || (w == best && i < best_i); }

__global__ __launch_bounds__(kDecodeThreads) void pyin_forward_kernel(DecodeArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int P = a.P, T = a.T, W = a.W, G = a.G;
    const int tid = threadIdx.x, threads = blockDim.x;
    const int q = blockIdx.x;
    const int row = P + 2 * W;                  // a padded row of U; U[copy][u][p] is at lds[u_word(copy, u, W + p, row)]
    float* win = lds + 4 * row;                 // [2W + 1]
    const float minus_inf = -__builtin_inff();
    const float* emit = a.emit + q * a.emit_seq_pitch;
    float* value = a.value ? a.value + q * a.value_seq_pitch : nullptr;
    unsigned short* psi = a.psi + (long long)q * T * 2 * P;
    float* vlast = a.vlast + (long long)q * 2 * P;

    for (int i = tid; i < 4 * row; i += threads) lds[i] = minus_inf;
    for (int k = tid; k <= 2 * W; k += threads) win[k] = a.log_window[k];
    __syncthreads();

    const int g = tid & (G - 1), d = tid / G;
    const bool owns = d < P && g == 0;
    const int pc = d < P ? d : P - 1;           // a lane past the last bin computes the last bin again and stores nothing
    const float off = a.src_offset[pc];
    float sw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sw[i] = a.log_switch[i];
    if (owns) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float v = a.init[u * P + pc] + emit[u * P + pc];
            lds[u_word(0, u, W + pc, row)] = v + off;
            if (value) value[u * P + pc] = v;
            if (T == 1) vlast[u * P + pc] = v;
        }
    }
    // The offsets of this lane are k = g, g + G, ... <= 2W, the source of k is p = pc - W + k.  Where none of its sources is above -inf
    // the lane holds its lowest source inside 0..P-1, and INT_MAX where it has none there.
    const int k_lo = W - pc > 0 ? W - pc : 0, k_hi = P - 1 - pc + W < 2 * W ? P - 1 - pc + W : 2 * W;
    const int k_first = k_lo + ((g - k_lo) & (G - 1));
    const int p_first = k_first <= k_hi ? pc - W + k_first : INT_MAX;
    float b_next[2] = {0.f, 0.f};
    if (T > 1) {
        b_next[0] = emit[a.emit_frame_pitch + pc];
        b_next[1] = emit[a.emit_frame_pitch + P + pc];
    }
    __syncthreads();

    for (int t = 1; t < T; ++t) {
        const float* prev = lds + ((t - 1) & 1) * 2 * row;
        const int cur = t & 1;
        const float b_cur[2] = {b_next[0], b_next[1]};
        const long long t_next = t + 1 < T ? t + 1 : t;
        b_next[0] = emit[t_next * a.emit_frame_pitch + pc];                 // in flight while this frame computes
        b_next[1] = emit[t_next * a.emit_frame_pitch + P + pc];
        // A lane meets its sources in ascending order, so inside the lane the pair rule is "strictly greater"; a NaN is never greater,
        // which is what counting it as -inf comes to.  The padding holds -inf and never wins.
        float m[2] = {minus_inf, minus_inf};
        int at[2] = {-1, -1};                                               // the offset k of the best source, -1: none above -inf
#if JSGX_PYIN_LOOP == 0
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float* src = prev + u * row + pc;                         // src[k] = U[u][pc - W + k]
#pragma unroll 4
            for (int k = g; k <= 2 * W; k += G) {
                const float v = src[k] + win[2 * W - k];
                if (v > m[u]) {
                    m[u] = v;
                    at[u] = k;
                }
            }
        }
#elif JSGX_PYIN_LOOP == 1
        {
            const float* src0 = prev + pc;
            const float* src1 = prev + row + pc;
#pragma unroll 4
            for (int k = g; k <= 2 * W; k += G) {
                const float lw = win[2 * W - k];
                const float v0 = src0[k] + lw, v1 = src1[k] + lw;
                if (v0 > m[0]) {
                    m[0] = v0;
                    at[0] = k;
                }
                if (v1 > m[1]) {
                    m[1] = v1;
                    at[1] = k;
                }
            }
        }
#else
        {
            const float2* src = reinterpret_cast<const float2*>(prev) + pc;  // src[k] = (U[0][pc - W + k], U[1][pc - W + k])
#pragma unroll 4
            for (int k = g; k <= 2 * W; k += G) {
                const float lw = win[2 * W - k];
                const float2 x = src[k];
                const float v0 = x.x + lw, v1 = x.y + lw;
                if (v0 > m[0]) {
                    m[0] = v0;
                    at[0] = k;
                }
                if (v1 > m[1]) {
                    m[1] = v1;
                    at[1] = k;
                }
            }
        }
#endif
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float best = m[u];
            const int best_k = at[u];
            int best_p = best_k >= 0 ? pc - W + best_k : p_first;
            for (int s = G >> 1; s >= 1; s >>= 1) {                          // the G lanes of a bin lie in one wavefront
                const float other = __shfl_xor(best, s);
                const int other_p = __shfl_xor(best_p, s);
                if (beats(other, other_p, best, best_p)) {
                    best = other;
                    best_p = other_p;
                }
            }
            m[u] = best;
            at[u] = best_p;
        }
        if (owns) {
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                float c0 = m[0] + sw[v], c1 = m[1] + sw[2 + v];
                c0 = c0 != c0 ? minus_inf : c0;
                c1 = c1 != c1 ? minus_inf : c1;
                const bool second = c1 > c0;
                const float x = (second ? c1 : c0) + b_cur[v];
                lds[u_word(cur, v, W + pc, row)] = x + off;
                psi[(long long)t * 2 * P + v * P + pc] = (unsigned short)(second ? P + at[1] : at[0]);
                if (value) value[t * a.value_frame_pitch + v * P + pc] = x;
                if (t == T - 1) vlast[v * P + pc] = x;
            }
        }
        __syncthreads();
    }
}

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_pyin_observe_launch(const jsgx_pyin_observe_args* g, void* stream) {
    static const char* who = "jsgx_pyin_observe_launch";
    int rc = pyin_observe_check(g, who);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    const bool multi = g->rows > 1;
    ObserveArgs k{};
    k.cmnd = g->cmnd;
    k.cmnd_frame_pitch = g->cmnd_frame_pitch;
    k.cmnd_row_pitch = multi ? g->cmnd_row_pitch : 0;
    k.prior = g->prior, k.decay = g->decay, k.norm = g->norm, k.edges = g->edges;
    k.tau_min = g->tau_min, k.tau_max = g->tau_max, k.N = g->n_thresholds, k.P = g->n_bins;
    k.max_troughs = pyin_max_troughs(g->tau_min, g->tau_max);
    k.no_trough_prob = g->no_trough_prob;
    k.log_emit = g->log_emit;
    k.emit_frame_pitch = g->emit_frame_pitch;
    k.emit_row_pitch = multi ? g->emit_row_pitch : 0;
    k.obs = g->obs;
    k.obs_frame_pitch = g->obs ? g->obs_frame_pitch : 0;
    k.obs_row_pitch = g->obs && multi ? g->obs_row_pitch : 0;
    k.voiced = g->voiced_prob;
    k.voiced_pitch = g->voiced_prob && multi ? g->voiced_pitch : 0;
    hipLaunchKernelGGL(pyin_observe_kernel, dim3((unsigned)g->n_frames, (unsigned)g->rows), dim3(kObserveThreads),
                       (size_t)pyin_observe_lds_bytes(g->tau_min, g->tau_max, g->n_bins), reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who, hipGetLastError());
}

extern "C" int jsgx_pyin_decode_launch(const jsgx_pyin_decode_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_pyin_decode_launch";
    int rc = pyin_decode_check(g, who);
    if (rc != JSGX_OK) return rc;
    const PyinDecodePlan p = pyin_decode_plan(g);
    if ((rc = check_scratch(who, scratch, scratch_bytes, p.back.scratch_bytes, "jsgx_pyin_decode_scratch_bytes")) != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    const bool multi = g->seqs > 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    DecodeArgs f{};
    f.emit = g->log_emit;
    f.emit_frame_pitch = g->emit_frame_pitch;
    f.emit_seq_pitch = multi ? g->emit_seq_pitch : 0;
    f.init = g->log_init;
    f.log_window = g->log_window, f.src_offset = g->src_offset, f.log_switch = g->log_switch;
    f.P = g->n_bins, f.T = g->n_frames, f.W = g->band_half, f.G = p.G;
    f.psi = reinterpret_cast<unsigned short*>(base + p.back.off_psi);
    f.vlast = reinterpret_cast<float*>(base);
    f.value = g->value;
    f.value_frame_pitch = g->value ? g->value_frame_pitch : 0;
    f.value_seq_pitch = g->value && multi ? g->value_seq_pitch : 0;
    hipLaunchKernelGGL(pyin_forward_kernel, dim3((unsigned)g->seqs), dim3((unsigned)p.threads), (size_t)p.lds_bytes, s, f);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = viterbi_backtrace_enqueue(base, p.back, g->seqs, 2 * g->n_bins, g->n_frames, g->states, multi ? g->states_pitch : 0, g->logp, s);
    return finish_launch(who, err);
}
