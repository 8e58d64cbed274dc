// libjsgx.so, Viterbi decoding (include/jsgx.h section 4): the forward kernel in its four forms, the three kernels of the blocked
// backtrace and their launcher.  The refusals, the plan and the layout of the scratch are in jsgx_viterbi_host.cpp.
//
// viterbi_forward_kernel<BAND, TABLE_IN_LDS>.  One workgroup decodes one sequence from frame 0 to T-1 and waits for nobody: time is
// serial, and the width of a frame (S destinations x their sources) is what the lanes share.  LDS holds V[t-1] and V[t] (two rows of
// S, swapped by the parity of t, one barrier per frame) and, in the "lds" forms, the transition table behind them with the row pitch
// S.  G lanes of a wavefront share the destination j = lane / G; lane g = lane % G of them takes the sources lo + g, lo + g + G, ...
// and the partial (w, i) are reduced with the pair rule by xor lane moves.  In one step of the source loop the lanes of a wavefront
// read G different V[t-1][i] (a broadcast within the lanes of one i) and 64 / G consecutive words of each of G table rows.  Where
// S > 1024 a lane owns j and j + 1024 (two passes).  The emissions of frame t + 1 are loaded before frame t computes and are first
// used after its barrier.  A lane whose destination lies past S-1 computes the destination S-1 again and stores nothing, so that
// every lane move has a defined source.
//
// The backtrace is blocked over B = JSGX_VITERBI_BLOCK frames (the header gives the three kernels); a chase of T dependent loads
// becomes B dependent loads in parallel over all states and blocks (jump), T / B in one lane (ends), and B again in parallel over
// the blocks (trace).
#include <hip/hip_runtime.h>

#include <climits>

#include "jsgx_internal.h"

namespace jsgx {

constexpr int kMaxThreads = JSGX_VITERBI_THREADS;
constexpr int kBlock = JSGX_VITERBI_BLOCK;
constexpr int kPasses = (JSGX_VITERBI_MAX_STATES + kMaxThreads - 1) / kMaxThreads;      // destinations a lane may own
constexpr int kJumpThreads = 256, kEndsThreads = 256, kTraceThreads = 64;
static_assert(kPasses == 2 && JSGX_VITERBI_MAX_STATES <= 65536, "psi and jump are uint16; a lane owns at most two destinations");
static_assert(4 * (JSGX_VITERBI_LDS_STATES * JSGX_VITERBI_LDS_STATES + 2 * JSGX_VITERBI_LDS_STATES) <= JSGX_VITERBI_LDS_LIMIT, "include/jsgx.h states the LDS");
static_assert(kBlock == 64 || kBlock == 256 || kBlock == 1024, "the block sizes that were measured");

struct ForwardArgs {
    const float* emit;
    long long emit_frame_pitch, emit_seq_pitch;
    const float* init;
    const float* trans;
    long long trans_pitch;
    int S, T, W, G;
    unsigned short* psi;            // [seqs][T][S]; row 0 is not written
    float* vlast;                   // [seqs][S]: V[T-1]
    float* value;                   // or null
    long long value_frame_pitch, value_seq_pitch;
};

struct BackArgs {
    const unsigned short* psi;
    unsigned short* jump;           // [seqs][n_blocks][S]; block 0 is not written
    int* end;                       // [seqs][n_blocks]
    const float* vlast;
    int S, T, n_blocks;
    int* states;
    long long states_pitch;
    float* logp;                    // or null
};

// the pair rule of include/jsgx.h: (w, i) beats (best, best_i)
__device__ __forceinline__ bool better(float w, int i, float best, int best_i) { return w > best || (w == best && i < best_i); }

template <bool BAND, bool TABLE_IN_LDS>
__global__ __launch_bounds__(kMaxThreads) void viterbi_forward_kernel(ForwardArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int S = a.S, T = a.T, W = a.W, G = a.G;
    const int tid = threadIdx.x, threads = blockDim.x;
    const int q = blockIdx.x;
    const float minus_inf = -__builtin_inff();
    float* table_lds = lds + 2 * S;
    const float* emit = a.emit + q * a.emit_seq_pitch;
    float* value = a.value ? a.value + q * a.value_seq_pitch : nullptr;
    unsigned short* psi = a.psi + (long long)q * T * S;

    if (TABLE_IN_LDS) {
        const int rows = BAND ? 2 * W + 1 : S;
        for (int idx = tid; idx < rows * S; idx += threads) {
            const int r = idx / S, j = idx - r * S;
            // a band entry whose source lies outside the matrix is never read, from memory or from LDS
            const bool read = !BAND || (unsigned)(j + r - W) < (unsigned)S;
            table_lds[idx] = read ? a.trans[r * a.trans_pitch + j] : minus_inf;
        }
    }
    for (int j = tid; j < S; j += threads) {
        const float v = a.init[j] + emit[j];
        lds[j] = v;
        if (value) value[j] = v;
        if (T == 1) a.vlast[(long long)q * S + j] = v;
    }
    __syncthreads();

    const float* table = TABLE_IN_LDS ? table_lds : a.trans;
    const long long pitch = TABLE_IN_LDS ? S : a.trans_pitch;
    const int g = tid & (G - 1), dests = threads / G, d = tid / G;
    // the destinations of this lane and, for the band, their first table word: A(i, j) is at table[(i - j + W) * pitch + j]
    int jc[kPasses];
    bool owns[kPasses];
    float b_next[kPasses];
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        const int j = p * dests + d;
        owns[p] = j < S && g == 0;
        jc[p] = j < S ? j : S - 1;
        b_next[p] = T > 1 ? emit[a.emit_frame_pitch + jc[p]] : 0.f;
    }
    for (int t = 1; t < T; ++t) {
        const float* prev = lds + ((t - 1) & 1) * S;
        float* cur = lds + (t & 1) * S;
        float b_cur[kPasses];
        const long long t_next = t + 1 < T ? t + 1 : t;
#pragma unroll
        for (int p = 0; p < kPasses; ++p) {
            b_cur[p] = b_next[p];
            b_next[p] = emit[t_next * a.emit_frame_pitch + jc[p]];         // in flight while this frame computes
        }
#pragma unroll
        for (int p = 0; p < kPasses; ++p) {
            if (p * dests >= S) break;                                      // uniform over the workgroup
            const int j = jc[p];
            const int lo = BAND ? (j - W > 0 ? j - W : 0) : 0, hi = BAND ? (j + W < S - 1 ? j + W : S - 1) : S - 1;
            const long long column = BAND ? (long long)(W - j) * pitch + j : j;      // A(i, j) = table[column + i * pitch]
            // A lane meets its sources in ascending order, so within the lane the pair rule is "strictly greater": an equal w keeps
            // the earlier source, and a NaN v is never greater, which is what counting it as -inf comes to.  The start (-inf, the
            // lane's first source) is that source's pair where its w is -inf; a lane without a source holds (-inf, INT_MAX), which
            // loses to every pair in the reduction below.
            int i = lo + g;
            float best = minus_inf;
            int best_i = i <= hi ? i : INT_MAX;
            const float* entry = table + column + i * pitch;
            const long long entry_step = G * pitch;
#pragma unroll 8
            for (; i <= hi; i += G, entry += entry_step) {
                const float v = prev[i] + *entry;
                if (v > best) {
                    best = v;
                    best_i = i;
                }
            }
            for (int m = G >> 1; m >= 1; m >>= 1) {                         // the G lanes of a destination lie in one wavefront
                const float other = __shfl_xor(best, m);
                const int other_i = __shfl_xor(best_i, m);
                if (better(other, other_i, best, best_i)) {
                    best = other;
                    best_i = other_i;
                }
            }
            if (owns[p]) {
                const float v = best + b_cur[p];
                cur[j] = v;
                psi[(long long)t * S + j] = (unsigned short)best_i;
                if (value) value[t * a.value_frame_pitch + j] = v;
                if (t == T - 1) a.vlast[(long long)q * S + j] = v;
            }
        }
        __syncthreads();
    }
}

// jump[k][s], k >= 1: from the state s at the last frame of block k down psi to the state at the last frame of block k - 1
__global__ __launch_bounds__(kJumpThreads) void viterbi_jump_kernel(BackArgs a) {
    const int k = blockIdx.x + 1, q = blockIdx.y;
    const int S = a.S;
    const long long last = (long long)(k + 1) * kBlock < a.T ? (long long)(k + 1) * kBlock - 1 : a.T - 1, before = (long long)k * kBlock - 1;
    const unsigned short* psi = a.psi + (long long)q * a.T * S;
    unsigned short* jump = a.jump + ((long long)q * a.n_blocks + k) * S;
    for (int s0 = threadIdx.x; s0 < S; s0 += kJumpThreads) {
        int s = s0;
        for (long long t = last; t > before; --t) s = psi[t * S + s];
        jump[s0] = (unsigned short)s;
    }
}

// e and logp of a sequence, then the end state of every block: end[n_blocks - 1] = e, end[k - 1] = jump[k][end[k]]
__global__ __launch_bounds__(kEndsThreads) void viterbi_ends_kernel(BackArgs a) {
    __shared__ float red_w[kEndsThreads];
    __shared__ int red_s[kEndsThreads];
    const int q = blockIdx.x, l = threadIdx.x, S = a.S;
    const float minus_inf = -__builtin_inff();
    const float* v = a.vlast + (long long)q * S;
    float best = minus_inf;
    int best_s = INT_MAX;
    for (int s = l; s < S; s += kEndsThreads) {
        const float x = v[s];
        const float w = x != x ? minus_inf : x;
        if (better(w, s, best, best_s)) {
            best = w;
            best_s = s;
        }
    }
    red_w[l] = best;
    red_s[l] = best_s;
    __syncthreads();
    for (int h = kEndsThreads / 2; h >= 1; h >>= 1) {
        if (l < h && better(red_w[l + h], red_s[l + h], red_w[l], red_s[l])) {
            red_w[l] = red_w[l + h];
            red_s[l] = red_s[l + h];
        }
        __syncthreads();
    }
    if (l == 0) {
        int s = red_s[0];                   // S >= 1: lane 0 has seen state 0, so this is a state
        if (a.logp) a.logp[q] = red_w[0];
        int* end = a.end + (long long)q * a.n_blocks;
        const unsigned short* jump = a.jump + (long long)q * a.n_blocks * S;
        end[a.n_blocks - 1] = s;
        for (int k = a.n_blocks - 1; k >= 1; --k) {
            s = jump[(long long)k * S + s];
            end[k - 1] = s;
        }
    }
}

// a lane per block: from the block's end state down its own frames
__global__ __launch_bounds__(kTraceThreads) void viterbi_trace_kernel(BackArgs a) {
    const int k = blockIdx.x * kTraceThreads + threadIdx.x, q = blockIdx.y;
    if (k >= a.n_blocks) return;
    const int S = a.S;
    const long long first = (long long)k * kBlock, last = first + kBlock < a.T ? first + kBlock - 1 : a.T - 1;
    const unsigned short* psi = a.psi + (long long)q * a.T * S;
    int* states = a.states + q * a.states_pitch;
    int s = a.end[(long long)q * a.n_blocks + k];
    states[last] = s;
    for (long long t = last; t > first; --t) {
        s = psi[t * S + s];
        states[t - 1] = s;
    }
}

namespace {
jsg::OncePerDevice g_told;      // a bit per form: the devices that know its LDS limit
}

hipError_t viterbi_backtrace_enqueue(char* base, const ViterbiPlan& p, int seqs, int S, int T, int* states, long long states_pitch, float* logp, hipStream_t s) {
    BackArgs b{};
    b.psi = reinterpret_cast<const unsigned short*>(base + p.off_psi);
    b.jump = reinterpret_cast<unsigned short*>(base + p.off_jump);
    b.end = reinterpret_cast<int*>(base + p.off_end);
    b.vlast = reinterpret_cast<const float*>(base);
    b.S = S, b.T = T, b.n_blocks = p.n_blocks;
    b.states = states;
    b.states_pitch = states_pitch;
    b.logp = logp;
    if (p.n_blocks > 1) hipLaunchKernelGGL(viterbi_jump_kernel, dim3((unsigned)(p.n_blocks - 1), (unsigned)seqs), dim3(kJumpThreads), 0, s, b);
    hipLaunchKernelGGL(viterbi_ends_kernel, dim3((unsigned)seqs), dim3(kEndsThreads), 0, s, b);
    hipLaunchKernelGGL(viterbi_trace_kernel, dim3((unsigned)((p.n_blocks + kTraceThreads - 1) / kTraceThreads), (unsigned)seqs), dim3(kTraceThreads), 0, s, b);
    return hipGetLastError();
}

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_viterbi_launch(const jsgx_viterbi_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_viterbi_launch";
    int rc = viterbi_check(g, who);
    if (rc != JSGX_OK) return rc;
    const ViterbiPlan p = viterbi_plan(g);
    if ((rc = check_scratch(who, scratch, scratch_bytes, p.scratch_bytes, "jsgx_viterbi_scratch_bytes")) != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    const bool multi = g->seqs > 1;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(scratch);
    ForwardArgs f{};
    f.emit = g->log_emit;
    f.emit_frame_pitch = g->emit_frame_pitch;
    f.emit_seq_pitch = multi ? g->emit_seq_pitch : 0;
    f.init = g->log_init;
    f.trans = g->trans;
    f.trans_pitch = g->trans_pitch;
    f.S = g->n_states, f.T = g->n_frames, f.W = g->band_half, f.G = p.G;
    f.psi = reinterpret_cast<unsigned short*>(base + p.off_psi);
    f.vlast = reinterpret_cast<float*>(base);
    f.value = g->value;
    f.value_frame_pitch = g->value ? g->value_frame_pitch : 0;
    f.value_seq_pitch = g->value && multi ? g->value_seq_pitch : 0;
    void (*const forms[4])(ForwardArgs) = {viterbi_forward_kernel<false, false>, viterbi_forward_kernel<false, true>, viterbi_forward_kernel<true, false>,
                                           viterbi_forward_kernel<true, true>};
    const int form = (p.band ? 2 : 0) + (p.table_in_lds ? 1 : 0);
    hipError_t err = jsg::launch_large_lds(g_told, dev, 1u << form, forms[form], JSGX_VITERBI_LDS_LIMIT, dim3((unsigned)g->seqs), dim3((unsigned)p.threads), (size_t)p.lds_bytes, s, f);
    if (err == hipSuccess) err = viterbi_backtrace_enqueue(base, p, g->seqs, g->n_states, g->n_frames, g->states, multi ? g->states_pitch : 0, g->logp, s);
    return finish_launch(who, err);
}
