// libjsg.so, onset strength, autocorrelation tempogram and tempo (include/jsg.h, section 2j).  A unit of its own; the refusals, the
// plan of a tempogram call and the prior table are in jsg_rhythm_host.cpp.
//
// onset_kernel: 256 threads; a group of W lanes (W = 64 where B > 32, else the smallest power of two >= B) takes four frames that lie
// 256 / W apart, so a workgroup takes 4 * 256 / W consecutive frames of a row.  Lane l walks b = l, l + W, ...: S[t][b] is read once
// from memory, the m neighbours of S[t-lag] come from the cache (the same lines were S[t] of the group `lag` frames before).  Where
// max_size is 1 the loads of the four frames are issued together and frames outside the row or below the lag are masked, not
// branched around (eight loads in flight per lane).  Bound by memory.
//
// tempogram_kernel: the structure of jsg_yin.hip.  256 threads (four waves), no scratch, no atomics.  A work item is (row, F
// consecutive frames); workgroups walk the items with a grid stride.  An item stages the span of its frames of the envelope into LDS
// with coalesced loads (zeros outside the row; the window table is staged once per workgroup), multiplies it into F rows of windowed
// samples y (out-of-row samples are +0, not products), then its waves take tiles (frame, block of 64 NL lags): lane l owns the NL
// consecutive lags b + NL l + q and walks j upwards, 8 at a time.  For one step it reads the 8 samples y[j .. j + 8) (one address for
// the wave: a broadcast) and the 8 + NL - 1 samples y[j + tau0 .. ), and they serve 8 NL pairs.  Where NL is 4 or 8 the reads are 16
// bytes wide and the last NL second samples of a step are kept in registers for the next, so a step reads 8 new ones: 4 LDS reads of
// 16 bytes per 64 fused multiply-adds at NL = 8.  A lane leaves the loop when its block would reach past the
// window (lanes of larger lags leave earlier: the triangle of the sum), then adds the at most 8 + NL - 2 samples that remain one by
// one, each pair tested.  So no pair past the window is ever multiplied, and per lag j simply ascends.  The sums go to LDS; after a
// barrier all threads normalise and store them coalesced.
//
// tempo_kernel: one workgroup per row; a thread owns the lags tid, tid + 256, ... and adds their frames in blocks of 64; the best lag
// is reduced through the wave and four LDS words.  Small: no claim is made for it.
//
// Every float operation of the definitions is written out (contraction is off; the fused multiply-add is explicit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

constexpr int TG_J = 8;                     // samples y[j] of one step

struct OnArgs {
    const float* in;
    long long frame_pitch, row_pitch;
    float* out;
    long long out_pitch;
    long long n_items;
    long long groups;                       // ceil(T / (ON_K * 256 / W)) per row
    int T, B, lag, lo, hi, W;
};

constexpr int ON_K = 4;                     // frames a group of lanes has in flight

// M1: max_size is 1 (the reference of a band is the band itself)
template <bool M1>
__global__ __launch_bounds__(256) void onset_kernel(const OnArgs a) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, W = a.W, l = tid & (W - 1), sub = tid / W, per = 256 / W;
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long r = item / a.groups;
        const long long t0 = (item - r * a.groups) * (per * ON_K) + sub;
        const float* row = a.in + r * a.row_pitch;
        float acc[ON_K];
        bool live[ON_K];
#pragma unroll
        for (int k = 0; k < ON_K; ++k) {
            acc[k] = 0.f;
            const long long t = t0 + k * per;
            live[k] = t < a.T && t >= a.lag;
        }
        if constexpr (M1) {
            const float *cur[ON_K], *prev[ON_K];
#pragma unroll
            for (int k = 0; k < ON_K; ++k) {        // a frame that does not count reads frame 0 twice and adds +0
                const long long t = t0 + k * per;
                cur[k] = row + (live[k] ? t : 0) * a.frame_pitch;
                prev[k] = row + (live[k] ? t - a.lag : 0) * a.frame_pitch;
            }
            for (int b = l; b < a.B; b += W) {
                float c[ON_K], p[ON_K];
#pragma unroll
                for (int k = 0; k < ON_K; ++k) c[k] = cur[k][b], p[k] = prev[k][b];
#pragma unroll
                for (int k = 0; k < ON_K; ++k) {
                    const float e = c[k] - p[k];
                    acc[k] = acc[k] + ((live[k] && (e > 0.f || e != e)) ? e : 0.f);
                }
            }
        } else {
#pragma unroll 1
            for (int k = 0; k < ON_K; ++k) {
                if (!live[k]) continue;
                const float* cur = row + (t0 + k * per) * a.frame_pitch;
                const float* prev = cur - a.lag * a.frame_pitch;
                float sum = 0.f;
                for (int b = l; b < a.B; b += W) {
                    const int b0 = max(0, b - a.lo), b1 = min(a.B - 1, b + a.hi);
                    float mx = prev[b0];
                    for (int c = b0 + 1; c <= b1; ++c) {
                        const float v = prev[c];
                        if (v > mx || v != v) mx = v;
                    }
                    const float e = cur[b] - mx;
                    sum = sum + ((e > 0.f || e != e) ? e : 0.f);
                }
                acc[k] = sum;
            }
        }
#pragma unroll
        for (int k = 0; k < ON_K; ++k) {
            float s = acc[k];
            for (int o = W >> 1; o >= 1; o >>= 1) s = s + __shfl_xor(s, o);
            const long long t = t0 + k * per;
            if (l == 0 && t < a.T) a.out[r * a.out_pitch + t] = live[k] ? s / (float)a.B : 0.f;
        }
    }
}

struct TgArgs {
    const float* in;
    long long in_pitch;
    const float* window;
    float* out;
    long long frame_pitch, row_pitch;
    long long n_items;
    int chunks, T, frames, hop, Wn, Lg, F, S, normalise;     // chunks = ceil(frames / F) < 2^31
};

// n floats (a multiple of 4) from 16-byte aligned LDS
template <int N>
__device__ __forceinline__ void tg_read(const float* p, float* to) {
#pragma unroll
    for (int i = 0; i < N; i += 4) {
        const float4 t = *reinterpret_cast<const float4*>(p + i);
        to[i] = t.x, to[i + 1] = t.y, to[i + 2] = t.z, to[i + 3] = t.w;
    }
}

// The pairs of j = 0 .. whole - 1 (a multiple of 8; all inside the window for the NL lags of the lane) with those lags; y = the row
// (16-byte aligned), v = &y[tau0].  Per lag the pairs come in ascending j.  NL 4 or 8: v is 16-byte aligned, a step keeps the second
// samples v[j0 .. j0 + 8 + NL) and hands the last NL of them to the next step (the last float read may lie one past the window and is
// not used).
template <int NL>
__device__ __forceinline__ void tg_whole(const float* y, const float* v, int whole, float (&acc)[NL]) {
#pragma clang fp contract(off)
    float Y[TG_J];
    if constexpr (NL % 4 == 0) {
        float V[TG_J + NL];
        if (whole > 0) tg_read<NL>(v, V);
        for (int j0 = 0; j0 < whole; j0 += TG_J) {
            tg_read<TG_J>(v + j0 + NL, V + NL);
            tg_read<TG_J>(y + j0, Y);
#pragma unroll
            for (int jj = 0; jj < TG_J; ++jj) {
#pragma unroll
                for (int q = 0; q < NL; ++q) acc[q] = __builtin_fmaf(Y[jj], V[jj + q], acc[q]);
            }
#pragma unroll
            for (int i = 0; i < NL; ++i) V[i] = V[TG_J + i];
        }
    } else {
        float V[TG_J + NL - 1];
        for (int j0 = 0; j0 < whole; j0 += TG_J) {
            tg_read<TG_J>(y + j0, Y);
#pragma unroll
            for (int k = 0; k < TG_J + NL - 1; ++k) V[k] = v[j0 + k];
#pragma unroll
            for (int jj = 0; jj < TG_J; ++jj) {
#pragma unroll
                for (int q = 0; q < NL; ++q) acc[q] = __builtin_fmaf(Y[jj], V[jj + q], acc[q]);
            }
        }
    }
}

template <int NL>
__global__ __launch_bounds__(kTgThreads) void tempogram_kernel(const TgArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float tg_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Wn = a.Wn, Lg = a.Lg, S = a.S, half = Wn / 2;
    const int Wp = (Wn + 3) & ~3;           // rows of y start on 16 bytes
    float* const yp = tg_lds;
    float* const dp = yp + a.F * Wp;
    float* const wp = dp + a.F * Lg + kTgPad;
    float* const sp = wp + Wn;
    const int blocks = (Lg + 64 * NL - 1) / (64 * NL);
    for (int e = tid; e < Wn; e += kTgThreads) wp[e] = a.window[e];
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int r = (int)(item / a.chunks), chunk = (int)(item - (long long)r * a.chunks);
        const int t0 = chunk * a.F;        // < frames
        const int Fc = min(a.F, a.frames - t0);
        const float* src = a.in + (long long)r * a.in_pitch;
        const long long first = (long long)t0 * a.hop - half;      // the sample of the row at sp[0]
        const int total = (Fc - 1) * S + Wn;
        __syncthreads();        // the item before has been read
#pragma unroll 4
        for (int e = tid; e < total; e += kTgThreads) {
            long long m = e;
            if (S != a.hop) {       // frames back to back
                const int fe = e / S;
                m = (long long)fe * a.hop + (e - fe * S);
            }
            m += first;
            sp[e] = m >= 0 && m < a.T ? src[m] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < Fc * Wn; e += kTgThreads) {
            const int f = e / Wn, j = e - f * Wn;
            const long long m = first + (long long)f * a.hop + j;
            yp[f * Wp + j] = m >= 0 && m < a.T ? sp[f * S + j] * wp[j] : 0.f;
        }
        __syncthreads();
        for (int tile = wave; tile < Fc * blocks; tile += kTgThreads / 64) {
            const int f = tile / blocks, tau0 = (tile - f * blocks) * (64 * NL) + NL * lane;
            const float* y = yp + f * Wp;
            const float* v = y + tau0;
            const int room = tau0 < Lg ? Wn - tau0 : 0;         // the j of lag tau0: j < room; of lag tau0 + q: j + q < room
            const int whole = max(0, room - (NL - 1)) / TG_J * TG_J;      // the j whose blocks of 8 lie inside the window for all NL lags
            float acc[NL];
#pragma unroll
            for (int q = 0; q < NL; ++q) acc[q] = 0.f;
            tg_whole<NL>(y, v, whole, acc);
            for (int j = whole; j < room; ++j) {
                const float yj = y[j];
#pragma unroll
                for (int q = 0; q < NL; ++q)
                    if (j + q < room) acc[q] = __builtin_fmaf(yj, v[j + q], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                const int tau = tau0 + q;
                if (tau < Lg) dp[f * Lg + tau] = acc[q];
            }
        }
        __syncthreads();
        float* dst = a.out + (long long)r * a.row_pitch + (long long)t0 * a.frame_pitch;
        for (int e = tid; e < Fc * Lg; e += kTgThreads) {
            const int f = e / Lg, tau = e - f * Lg;
            float val = dp[e];
            if (a.normalise) {
                const float a0 = dp[f * Lg];
                val = a0 == 0.f ? 0.f : val / a0;
            }
            dst[(long long)f * a.frame_pitch + tau] = val;
        }
    }
}

struct TpArgs {
    const float* in;
    long long frame_pitch, row_pitch;
    const float* prior;
    float* bpm;
    int* lag;
    float* profile;
    long long profile_pitch;
    int N, Lg;
    float rate60;
};

__device__ __forceinline__ bool tp_better(float s, int tau, float best, int best_tau) { return s > best || (s == best && tau < best_tau); }

__global__ __launch_bounds__(256) void tempo_kernel(const TpArgs a) {
#pragma clang fp contract(off)
    __shared__ float w_best[4];
    __shared__ int w_tau[4];
    __shared__ int w_nan[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long r = blockIdx.x;
    const float* base = a.in + r * a.row_pitch;
    float best = -__builtin_inff();
    int best_tau = INT_MAX;
    bool nan = false;
    for (int tau = tid; tau < a.Lg; tau += 256) {
        const float* col = base + tau;
        float total = 0.f;
        int i0 = 0;
        for (; i0 + 64 <= a.N; i0 += 64) {
            float P = 0.f;
#pragma unroll 16
            for (int i = 0; i < 64; ++i) P = P + col[(long long)(i0 + i) * a.frame_pitch];
            total = total + P;
        }
        if (i0 < a.N) {
            float P = 0.f;
            for (int i = i0; i < a.N; ++i) P = P + col[(long long)i * a.frame_pitch];
            total = total + P;
        }
        const float g = total / (float)a.N;
        if (a.profile) a.profile[r * a.profile_pitch + tau] = g;
        if (tau >= 1) {
            nan = nan || g != g;
            const float s = __builtin_fmaf(1e6f, g, 1.0f) * a.prior[tau];
            if (tp_better(s, tau, best, best_tau)) {
                best = s;
                best_tau = tau;
            }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int ot = __shfl_xor(best_tau, o);
        if (tp_better(ob, ot, best, best_tau)) {
            best = ob;
            best_tau = ot;
        }
    }
    const bool any_nan = __any(nan);
    if (lane == 0) {
        w_best[wave] = best;
        w_tau[wave] = best_tau;
        w_nan[wave] = any_nan;
    }
    __syncthreads();
    if (tid == 0) {
        bool bad = false;
        for (int k = 0; k < 4; ++k) {
            bad = bad || w_nan[k];
            if (k && tp_better(w_best[k], w_tau[k], best, best_tau)) {
                best = w_best[k];
                best_tau = w_tau[k];
            }
        }
        const int tau = best_tau == INT_MAX ? 1 : best_tau;
        if (a.bpm) a.bpm[r] = bad ? __builtin_nanf("") : a.rate60 / (float)tau;
        if (a.lag) a.lag[r] = bad ? -1 : tau;
    }
}

}  // namespace jsg

using namespace jsg;

extern "C" int jsg_onset_strength_launch(const jsg_onset_args* g, void* stream) {
    static const char* who = "jsg_onset_strength_launch";
    int dev = -1;
    int rc = onset_check(g, who);
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    OnArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.frame_pitch = g->frame_pitch;
    k.row_pitch = multi ? g->row_pitch : 0;
    k.out = g->out;
    k.out_pitch = multi ? g->out_pitch : 0;
    k.T = (int)g->n_frames;
    k.B = g->n_bands;
    k.lag = g->lag;
    k.lo = g->max_size / 2;
    k.hi = (g->max_size - 1) / 2;
    k.W = 64;
    if (k.B <= 32) {
        k.W = 1;
        while (k.W < k.B) k.W *= 2;
    }
    const int per = ON_K * (256 / k.W);
    k.groups = (g->n_frames + per - 1) / per;
    k.n_items = (long long)g->rows * k.groups;
    const dim3 grid(resident_grid(k.n_items, dev, 32));
    if (g->max_size == 1)
        hipLaunchKernelGGL(onset_kernel<true>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k);
    else
        hipLaunchKernelGGL(onset_kernel<false>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who);
}

extern "C" int jsg_tempogram_launch(const jsg_tempogram_args* g, void* stream) {
    static const char* who = "jsg_tempogram_launch";
    int dev = -1;
    int rc = tempogram_check(g, who);
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    TgPlan p{};
    tempogram_resolve(g, &p);
    TgArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.in_pitch = multi ? g->in_pitch : 0;
    k.window = g->window;
    k.out = g->out;
    k.frame_pitch = g->frame_pitch;
    k.row_pitch = multi ? g->row_pitch : 0;
    k.n_items = (long long)g->rows * p.chunks;
    k.chunks = (int)p.chunks;
    k.T = (int)g->n_in;
    k.frames = (int)g->n_frames;
    k.hop = (int)g->hop;
    k.Wn = g->win_length;
    k.Lg = g->lags;
    k.F = p.F;
    k.S = p.S;
    k.normalise = g->normalise;
    const size_t lds_bytes = sizeof(float) * (size_t)p.lds_floats;
    const dim3 grid(resident_grid(k.n_items, dev, per_cu_by_lds(kTgLdsOne, p.lds_floats, 8)));      // 2048 threads per compute unit
    static void (*const kernels[4])(TgArgs) = {tempogram_kernel<1>, tempogram_kernel<2>, tempogram_kernel<4>, tempogram_kernel<8>};      // the code object holds them in this order
    const int path = p.NL == 1 ? 0 : p.NL == 2 ? 1 : p.NL == 4 ? 2 : 3;
    static OncePerDevice told;      // a bit per path
    const hipError_t err = launch_large_lds(told, dev, 1u << path, kernels[path], kTgLdsOne * 4, grid, dim3(kTgThreads), lds_bytes, reinterpret_cast<hipStream_t>(stream), k);
    return err == hipSuccess ? JSG_OK : jsg_fail_hip(err, who);
}

extern "C" int jsg_tempo_launch(const jsg_tempo_args* g, void* stream) {
    static const char* who = "jsg_tempo_launch";
    int dev = -1;
    int rc = tempo_check(g, who);
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    TpArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.frame_pitch = g->frame_pitch;
    k.row_pitch = multi ? g->row_pitch : 0;
    k.prior = g->prior;
    k.bpm = g->bpm;
    k.lag = g->lag;
    k.profile = g->profile;
    k.profile_pitch = multi ? g->profile_pitch : 0;
    k.N = (int)g->n_frames;
    k.Lg = g->lags;
    k.rate60 = 60.0f * g->frame_rate;
    hipLaunchKernelGGL(tempo_kernel, dim3((unsigned)g->rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who);
}
