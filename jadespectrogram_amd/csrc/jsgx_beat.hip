// libjsgx.so, beat tracking by dynamic programming (include/jsgx.h section 1): the kernel and its launcher.  The refusals, the scratch
// size, the plan and the logarithm table are in jsgx_beat_host.cpp.
//
// One workgroup of 256 lanes per row.  The row's period comes from device memory (what jsg_tempo_launch wrote), so everything that
// depends on it -- the form, the tables -- is decided inside the kernel, uniformly per workgroup, and the LDS is static and sized for
// the largest period:
//   ring[4096]   C of the latest frames, indexed t & 4095 (a step reads C[t - 2P .. t - a] and writes C[t .. t + F - 1], F <= a <= 512:
//                at most 2P + F <= 2304 live entries); before the recurrence it stages s0 for the smoothing
//   pen[tau]     the penalty, tau = a..2P, filled once per row;   gw[k]  the smoothing weights, k = 0..P
//   red / redi   256 floats / ints of the lane sums, the maxima and the arg-maxima
// The recurrence looks back at least a = (P + 1) / 2 frames, so F <= a frames advance per step, G = 256 / F lanes (one where
// a >= 256) per frame over tau = a + j, a + j + G, ...; consecutive lanes of a frame group read consecutive ring entries and the same
// pen entry.  One barrier per step.  The scratch holds link (and s where smooth); lane 0 walks it twice at the end.
#include <hip/hip_runtime.h>

#include <climits>

#include "jsgx_internal.h"

namespace jsgx {

struct BeatArgs {
    const float* in;
    long long in_pitch;
    const int* period;
    const float* log_table;
    int* beats;
    long long beats_pitch;
    int* n_beats;
    float* local_score;
    long long local_pitch;
    float* cum_score;
    long long cum_pitch;
    int* link;          // scratch: [rows][T]
    float* s;           // scratch: [rows][T] where smooth, else null
    int T, period_all, smooth, normalise, max_beats;
    float tightness;
};

constexpr int kThreads = JSGX_BEAT_THREADS;

__device__ __forceinline__ bool better(float v, int tau, float best, int best_tau) { return v > best || (v == best && tau < best_tau); }

// the lane sum of include/jsgx.h: every lane brings its strided partial sum; the halving tree runs in LDS
__device__ __forceinline__ float tree_sum(float acc, float* red, int tid) {
#pragma clang fp contract(off)
    __syncthreads();
    red[tid] = acc;
    __syncthreads();
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        if (tid < h) red[tid] = red[tid] + red[tid + h];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ float tree_max(float m, float* red, int tid) {
    __syncthreads();
    red[tid] = m;
    __syncthreads();
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        if (tid < h) {
            const float o = red[tid + h];
            if (o > red[tid]) red[tid] = o;
        }
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ int tree_min(int m, int* redi, int tid) {
    __syncthreads();
    redi[tid] = m;
    __syncthreads();
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        if (tid < h) redi[tid] = min(redi[tid], redi[tid + h]);
        __syncthreads();
    }
    return redi[0];
}

__global__ __launch_bounds__(kThreads) void beat_kernel(const BeatArgs a) {
#pragma clang fp contract(off)
    __shared__ float ring[kBeatRing];
    __shared__ float pen[kBeatPen];
    __shared__ float gw[kBeatG];
    __shared__ float red[kThreads];
    __shared__ int redi[kThreads];
    const int tid = threadIdx.x;
    const long long r = blockIdx.x;
    const int T = a.T;
    const int P = a.period ? a.period[r] : a.period_all;
    if (P < 1 || P > JSGX_BEAT_MAX_PERIOD) {         // uniform: the whole workgroup leaves
        if (tid == 0) a.n_beats[r] = -1;
        return;
    }
    const float* o = a.in + r * a.in_pitch;
    int* link = a.link + r * (long long)T;
    float* sbuf = a.s ? a.s + r * (long long)T : nullptr;
    float* ls = a.local_score ? a.local_score + r * a.local_pitch : nullptr;
    float* cs = a.cum_score ? a.cum_score + r * a.cum_pitch : nullptr;

    // ---- pass 1: NaN, and the lane sum of o
    float acc = 0.f;
    int nan = 0;
    for (int t = tid; t < T; t += kThreads) {
        const float v = o[t];
        nan |= v != v;
        acc = acc + v;
    }
    if (__syncthreads_or(nan)) {
        if (tid == 0) a.n_beats[r] = -1;
        return;
    }
    // ---- the divisor of s0: sd, or 0 for "s0 = o"
    float sd = 0.f;
    if (a.normalise && T > 1) {
        const float mean = tree_sum(acc, red, tid) / (float)T;
        acc = 0.f;
        for (int t = tid; t < T; t += kThreads) {
            const float d = o[t] - mean;
            const float q = d * d;
            acc = acc + q;
        }
        sd = __builtin_sqrtf(tree_sum(acc, red, tid) / (float)(T - 1));
    }
    const bool scaled = sd != 0.f;

    // ---- tables
    const BeatForm form = beat_form(P);
    const int lo = form.a, hi = 2 * P;
    const float logP = a.log_table[P];
    for (int tau = lo + tid; tau <= hi; tau += kThreads) {
        const float d = a.log_table[tau] - logP;
        const float td = a.tightness * d;
        pen[tau] = -(td * d);
    }
    if (a.smooth)
        for (int k = tid; k <= P; k += kThreads) {
            const float z = (32.0f * (float)k) / (float)P;
            const float zz = z * z;
            gw[k] = exp_neg(-0.5f * zz);
        }
    __syncthreads();

    // ---- the local score s (into the scratch where smooth), its maximum
    float mx = -__builtin_inff();
    if (a.smooth) {
        for (int t0 = 0; t0 < T; t0 += kThreads) {
            // s0[t0 - P .. t0 + 255 + P] where inside the row, at ring[0 .. 256 + 2P)
            const int first = t0 - P, n = kThreads + 2 * P;
            for (int i = tid; i < n; i += kThreads) {
                const int u = first + i;
                if (u >= 0 && u < T) {
                    const float v = o[u];
                    ring[i] = scaled ? v / sd : v;
                }
            }
            __syncthreads();
            const int t = t0 + tid;
            if (t < T) {
                float sum = 0.f;
                const int k0 = max(-P, -t), k1 = min(P, T - 1 - t);
                for (int k = k0; k <= k1; ++k) sum = __builtin_fmaf(gw[k < 0 ? -k : k], ring[tid + P + k], sum);
                sbuf[t] = sum;
                if (ls) ls[t] = sum;
                if (sum > mx) mx = sum;
            }
            __syncthreads();
        }
    } else {
        for (int t = tid; t < T; t += kThreads) {
            const float v = o[t];
            const float sv = scaled ? v / sd : v;
            if (ls) ls[t] = sv;
            if (sv > mx) mx = sv;
        }
    }
    const float th = 0.01f * tree_max(mx, red, tid);
    // ---- t0: the first t with s[t] >= th
    int first_hit = T;
    for (int t = tid; t < T; t += kThreads) {
        float sv;
        if (a.smooth) {
            sv = sbuf[t];       // written by this lane above
        } else {
            const float v = o[t];
            sv = scaled ? v / sd : v;
        }
        if (sv >= th) {
            first_hit = t;
            break;
        }
    }
    const int t_first = tree_min(first_hit, redi, tid);

    // ---- the recurrence: F frames per step, G lanes per frame
    const int G = form.G, F = form.F;
    const int f = tid / G, j = tid - f * G;
    for (int tb = 0; tb < T; tb += F) {
        const int t = tb + f;
        const bool active = f < F && t < T;
        float sv = 0.f;
        if (active && j == 0) {
            if (a.smooth) {
                sv = sbuf[t];
            } else {
                const float v = o[t];
                sv = scaled ? v / sd : v;
            }
        }
        float best = -__builtin_inff();
        int best_tau = INT_MAX;
        if (active)
            // the reads do not depend on one another: unrolled, and the ring read unconditional (u < 0 reads some slot of the ring and
            // drops it), eight iterations' reads are in flight together; one iteration at a time is one LDS latency each
#pragma unroll 8
            for (int tau = lo + j; tau <= hi; tau += G) {
                const int u = t - tau;
                const float slot = ring[u & (kBeatRing - 1)];
                const float c = u < 0 ? 0.f : slot;
                const float v = pen[tau] + c;
                if (better(v, tau, best, best_tau)) {
                    best = v;
                    best_tau = tau;
                }
            }
        for (int w = G >> 1; w >= 1; w >>= 1) {        // G <= 64 lanes of one wave
            const float ob = __shfl_xor(best, w);
            const int ot = __shfl_xor(best_tau, w);
            if (better(ob, ot, best, best_tau)) {
                best = ob;
                best_tau = ot;
            }
        }
        if (active && j == 0) {
            if (best_tau == INT_MAX) {      // only where every v is NaN (outside the contract): keep the walk inside the row
                best_tau = lo;
                best = __builtin_nanf("");
            }
            const float c = sv + best;
            ring[t & (kBeatRing - 1)] = c;
            if (cs) cs[t] = c;
            const int back = t - best_tau;
            link[t] = (back < 0 || t < t_first) ? -1 : back;
        }
        __syncthreads();
    }

    // ---- the end: the best C of the last period (still in the ring), the lowest t on ties
    const int e0 = max(0, T - P);
    float eb = -__builtin_inff();
    int et = INT_MAX;
    for (int t = e0 + tid; t < T; t += kThreads) {
        const float c = ring[t & (kBeatRing - 1)];
        if (better(c, t, eb, et)) {
            eb = c;
            et = t;
        }
    }
    red[tid] = eb;
    redi[tid] = et;
    __syncthreads();
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
        if (tid < h && better(red[tid + h], redi[tid + h], red[tid], redi[tid])) {
            red[tid] = red[tid + h];
            redi[tid] = redi[tid + h];
        }
        __syncthreads();
    }
    // ---- the backtrace: one lane, two walks (the length, then the beats in ascending order)
    if (tid == 0) {
        const int e = redi[0] == INT_MAX ? e0 : redi[0];
        int n = 0;
        for (int u = e; u >= 0; u = link[u]) ++n;
        a.n_beats[r] = n;
        int* beats = a.beats + r * a.beats_pitch;
        int i = n - 1;
        for (int u = e; u >= 0; u = link[u], --i)
            if (i < a.max_beats) beats[i] = u;
    }
}

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_beat_launch(const jsgx_beat_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_beat_launch";
    int rc = beat_check(g, who);
    if (rc == JSGX_OK) rc = check_scratch(who, scratch, scratch_bytes, beat_scratch_bytes(g), "jsgx_beat_scratch_bytes");
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    BeatArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.in_pitch = multi ? g->in_pitch : 0;
    k.period = g->period;
    k.log_table = g->log_table;
    k.beats = g->beats;
    k.beats_pitch = multi ? g->beats_pitch : 0;
    k.n_beats = g->n_beats;
    k.local_score = g->local_score;
    k.local_pitch = multi ? g->local_pitch : 0;
    k.cum_score = g->cum_score;
    k.cum_pitch = multi ? g->cum_pitch : 0;
    k.link = static_cast<int*>(scratch);
    k.s = g->smooth ? static_cast<float*>(scratch) + (long long)g->rows * g->n_frames : nullptr;
    k.T = g->n_frames;
    k.period_all = g->period_all;
    k.smooth = g->smooth;
    k.normalise = g->normalise;
    k.max_beats = g->max_beats;
    k.tightness = g->tightness;
    hipLaunchKernelGGL(beat_kernel, dim3((unsigned)g->rows), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who, hipGetLastError());
}
