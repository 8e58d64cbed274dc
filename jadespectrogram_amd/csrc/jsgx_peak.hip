// libjsgx.so, peak picking and onset backtracking (include/jsgx.h section 14): the kernels and the launcher.  A group of lanes (a
// workgroup, or a wavefront for a row of up to JSGX_PEAK_SHORT frames) owns CAP frames of a row in LDS and works through them in steps
// that every lane of the workgroup takes together:
//   candidates   y (normalised on the way in, with a halo of the largest reach where the row goes on) -> c[t] by direct evaluation: the
//                maximum test leaves at the first larger neighbour, the mean is the ascending sum and is taken only where the test held
//   nxt          nxt[t] = the first candidate >= t, a suffix minimum of (c[t] ? t : END) by doubling
//   lm           lm[t] = 1 + the last energy minimum <= t inside the group's frames (0: none), a prefix maximum by doubling
//   tables       lev[0][p] = nxt[p + wait + 1] (END behind the frames), lev[k] = lev[k-1] o lev[k-1]: the pick 2^k picks behind p.  They
//                lie where y lay.  The chain from a pick f: its length and last pick by descending the tables, its i-th pick by the bits of i
// "peak_single" does all of it for a row in one launch; "peak_blocked" cuts the row into blocks ("peak_stats", "peak_row", "peak_cand"),
// walks the blocks of a row with one lane ("peak_carry": one word read per block the chain enters) and writes the peaks with the tables
// built again from the stored candidates ("peak_emit").
#include "jsgx_internal.h"

namespace jsgx {

namespace {

constexpr int kThreads = JSGX_PEAK_THREADS;
constexpr int kB = JSGX_PEAK_BLOCK;
constexpr int kReach = JSGX_PEAK_MAX_REACH;
constexpr int kShort = JSGX_PEAK_SHORT;
constexpr unsigned short kEnd = 0xffff;
constexpr int log2_of(int n) { return n <= 1 ? 0 : 1 + log2_of(n / 2); }
static_assert(kB >= 256 && kB <= 2048 && (kB & (kB - 1)) == 0 && log2_of(kB) == JSGX_PEAK_LOG2_BLOCK, "JSGX_PEAK_BLOCK: a power of two in 256..2048");
static_assert(4 * (kB + 2 * kReach) <= 2 * kB * log2_of(kB), "y and its halo fit where the tables lie");
static_assert(JSGX_PEAK_LDS_BYTES <= JSGX_PEAK_LDS_LIMIT, "include/jsgx.h");

struct PeakK {
    const float* in;
    long long in_pitch;
    const float* energy;
    long long energy_pitch;
    unsigned char* candidate;
    long long candidate_pitch;
    int* peaks;
    int* back;
    long long peaks_pitch;
    int* n_peaks;
    PeakRecord* rec;
    unsigned* words;
    unsigned char* flags;
    int rows, T, blocks, offsets;
    int pre_max, post_max, pre_avg, post_avg;
    float delta;
    int wait, normalise, max_peaks;
};

// minimum, maximum and the non-finite vote over a group of TPR lanes, lane l of it: every lane gets all three.  red: three floats a wavefront
template <int TPR>
__device__ __forceinline__ void reduce3(float& mn, float& mx, int& bad, float* red, int l) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, d));
        mx = fmaxf(mx, __shfl_xor(mx, d));
        bad |= __shfl_xor(bad, d);
    }
    if (TPR > 64) {
        if ((l & 63) == 0) red[3 * (l >> 6)] = mn, red[3 * (l >> 6) + 1] = mx, red[3 * (l >> 6) + 2] = __int_as_float(bad);
        __syncthreads();
#pragma unroll
        for (int w = 0; w < TPR / 64; ++w) mn = fminf(mn, red[3 * w]), mx = fmaxf(mx, red[3 * w + 1]), bad |= __float_as_int(red[3 * w + 2]);
        __syncthreads();
    }
}

// The LDS of a group of TPR lanes that owns up to CAP frames
template <int CAP, int TPR>
struct Group {
    static constexpr int LOG = log2_of(CAP), E = CAP / TPR;
    static constexpr int kBytes = 2 * CAP * LOG + 2 * (CAP + 4) + 2 * CAP;
    static_assert(4 * CAP <= 2 * CAP * LOG && kBytes % 8 == 0, "y fits where the tables lie; the groups stay aligned");
    float* y;                     // aliases lev: read before the tables are written
    unsigned short* lev;          // [LOG][CAP]
    unsigned short* nxt;          // [CAP + 4]
    unsigned short* lm;           // [CAP]; three floats a wavefront for the reduction first
    int l;                        // the lane of the group

    __device__ __forceinline__ Group(char* base, int lane) : l(lane) {
        y = reinterpret_cast<float*>(base);
        lev = reinterpret_cast<unsigned short*>(base);
        nxt = lev + CAP * LOG;
        lm = nxt + CAP + 4;
    }

    // minimum, maximum and the non-finite vote over the group: every lane gets all three
    __device__ __forceinline__ void reduce(float& mn, float& mx, int& bad) { reduce3<TPR>(mn, mx, bad, reinterpret_cast<float*>(lm), l); }

    // c[t] of the row's frame t from y, whose first element is the row's frame lo
    __device__ __forceinline__ bool candidate(const PeakK& g, int t, int lo) const {
#pragma clang fp contract(off)
        const float yt = y[t - lo];
        int a = t - g.pre_max > 0 ? t - g.pre_max : 0, b = t + g.post_max < g.T - 1 ? t + g.post_max : g.T - 1;
        for (int j = a; j <= b; ++j)
            if (y[j - lo] > yt) return false;
        a = t - g.pre_avg > 0 ? t - g.pre_avg : 0, b = t + g.post_avg < g.T - 1 ? t + g.post_avg : g.T - 1;
        float acc = 0.f;
        for (int j = a; j <= b; ++j) acc = acc + y[j - lo];
        const float avg = acc / (float)(b - a + 1);
        return yt >= avg + g.delta;
    }

    // nxt and lm from their per-frame starts over the first n frames (n the same in every lane of the workgroup)
    __device__ __forceinline__ void scans(int n, bool with_lm) {
        for (int d = 1; d < n; d <<= 1) {
            unsigned short v[E], m[E];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int t = l + j * TPR;
                v[j] = t + d < CAP ? nxt[t + d] : kEnd;
                m[j] = with_lm && t >= d ? lm[t - d] : 0;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int t = l + j * TPR;
                if (v[j] < nxt[t]) nxt[t] = v[j];
                if (with_lm && m[j] > lm[t]) lm[t] = m[j];
            }
            __syncthreads();
        }
    }

    // the tables over the first n frames; y is gone behind this
    __device__ __forceinline__ void tables(int n, int wait) {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int p = l + j * TPR;
            lev[p] = p + wait + 1 < n ? nxt[p + wait + 1] : kEnd;
        }
        __syncthreads();
        for (int k = 1; k < LOG; ++k) {
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const int p = l + j * TPR;
                const unsigned short a = lev[(k - 1) * CAP + p];
                lev[k * CAP + p] = a == kEnd ? kEnd : lev[(k - 1) * CAP + a];
            }
            __syncthreads();
        }
    }

    // the picks of the chain whose first pick is f (END: none), and the last of them
    __device__ __forceinline__ int chain(unsigned short f, int* last) const {
        if (f == kEnd) return 0;
        int q = f, c = 0;
#pragma unroll
        for (int k = LOG - 1; k >= 0; --k) {
            const unsigned short a = lev[k * CAP + q];
            if (a != kEnd) q = a, c += 1 << k;
        }
        *last = q;
        return c + 1;
    }
    // its i-th pick, i below the count
    __device__ __forceinline__ int pick(unsigned short f, int i) const {
        int q = f;
#pragma unroll
        for (int k = 0; k < LOG; ++k)
            if ((i >> k) & 1) q = lev[k * CAP + q];
        return q;
    }
};

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) < __builtin_inff(); }          // false for a NaN

// y of x, with the row's minimum and range
__device__ __forceinline__ float normalised(float x, float mn, float range, int normalise) {
#pragma clang fp contract(off)
    if (!normalise) return x;
    return range == 0.f ? 0.f : (x - mn) / range;
}

// frame t of the row e of T frames is a local minimum
__device__ __forceinline__ bool is_minimum(const float* e, int t, int T) {
    if (t == 0) return true;
    if (t >= T - 1) return false;
    const float v = e[t];
    return v <= e[t - 1] && v < e[t + 1];
}

// T <= CAP: a group a row, G = kThreads / TPR rows a workgroup
template <int CAP, int TPR>
__global__ __launch_bounds__(kThreads) void peak_single_kernel(PeakK g) {
    using Grp = Group<CAP, TPR>;
    constexpr int E = Grp::E;
    __shared__ __attribute__((aligned(16))) char smem[JSGX_PEAK_LDS_BYTES];
    static_assert(Grp::kBytes * (kThreads / TPR) <= JSGX_PEAK_LDS_BYTES, "the groups of a workgroup fit");
    const int grp = threadIdx.x / TPR;
    Grp s(smem + grp * Grp::kBytes, threadIdx.x % TPR);
    const int r = blockIdx.x * (kThreads / TPR) + grp, n = g.T;
    const bool valid = r < g.rows;
    const float* x = g.in + (valid ? r : 0) * g.in_pitch;
    const float* e = g.energy ? g.energy + (valid ? r : 0) * g.energy_pitch : nullptr;
    float xv[E], mn = __builtin_inff(), mx = -__builtin_inff();
    int bad = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int t = s.l + j * TPR;
        xv[j] = t < n ? x[t] : 0.f;
        if (t < n) {
            mn = fminf(mn, xv[j]), mx = fmaxf(mx, xv[j]);
            bad |= !is_finite(xv[j]) || (e && !is_finite(e[t]));
        }
    }
    s.reduce(mn, mx, bad);
    const bool active = valid && !bad;
    const float range = mx - mn;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int t = s.l + j * TPR;
        if (t < n) s.y[t] = normalised(xv[j], mn, range, g.normalise);
    }
    __syncthreads();
    bool c[E], m[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int t = s.l + j * TPR;
        c[j] = t < n && s.candidate(g, t, 0);
        m[j] = t < n && e && is_minimum(e, t, n);
        if (active && g.candidate && t < n) g.candidate[r * g.candidate_pitch + t] = c[j];
    }
    __syncthreads();          // y has been read
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int t = s.l + j * TPR;
        s.nxt[t] = c[j] ? t : kEnd;
        s.lm[t] = m[j] ? t + 1 : 0;
    }
    if (s.l < 4) s.nxt[CAP + s.l] = kEnd;
    __syncthreads();
    s.scans(n, e != nullptr);
    s.tables(n, g.wait);
    const unsigned short f = s.nxt[0];
    int last = 0;
    const int count = s.chain(f, &last);
    if (!valid) return;
    if (s.l == 0) g.n_peaks[r] = bad ? -1 : count;
    if (bad) return;
    const int most = count < g.max_peaks ? count : g.max_peaks;
    for (int i = s.l; i < most; i += TPR) {
        const int p = s.pick(f, i);
        g.peaks[r * g.peaks_pitch + i] = p;
        if (g.back) g.back[r * g.peaks_pitch + i] = s.lm[p] - 1;
    }
}

// the block's minimum, maximum and non-finite vote into its record
__global__ __launch_bounds__(kThreads) void peak_stats_kernel(PeakK g) {
    __shared__ float red[3 * kThreads / 64];
    const int k = blockIdx.x, r = blockIdx.y, t0 = k * kB;
    const float* x = g.in + r * g.in_pitch;
    const float* e = g.energy ? g.energy + r * g.energy_pitch : nullptr;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int bad = 0;
    for (int t = t0 + threadIdx.x; t < t0 + kB && t < g.T; t += kThreads) {
        const float v = x[t];
        mn = fminf(mn, v), mx = fmaxf(mx, v);
        bad |= !is_finite(v) || (e && !is_finite(e[t]));
    }
    reduce3<kThreads>(mn, mx, bad, red, threadIdx.x);
    if (threadIdx.x == 0) {
        PeakRecord* rec = g.rec + (long long)r * g.blocks + k;
        rec->mn = mn, rec->mx = mx, rec->bad = bad;
    }
}

// the row's three out of its blocks', into every record of the row
__global__ __launch_bounds__(kThreads) void peak_row_kernel(PeakK g) {
    __shared__ float red[3 * kThreads / 64];
    PeakRecord* rec = g.rec + (long long)blockIdx.x * g.blocks;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int bad = 0;
    for (int k = threadIdx.x; k < g.blocks; k += kThreads) mn = fminf(mn, rec[k].mn), mx = fmaxf(mx, rec[k].mx), bad |= rec[k].bad;
    reduce3<kThreads>(mn, mx, bad, red, threadIdx.x);          // its barriers stand between the reads above and the writes below
    for (int k = threadIdx.x; k < g.blocks; k += kThreads) rec[k].mn = mn, rec[k].mx = mx, rec[k].bad = bad;
}

// a block: the candidates into the scratch (and the plane), for every entering offset the count and the last pick, the last minimum
__global__ __launch_bounds__(kThreads) void peak_cand_kernel(PeakK g) {
    using Grp = Group<kB, kThreads>;
    constexpr int E = Grp::E;
    __shared__ __attribute__((aligned(16))) char smem[JSGX_PEAK_LDS_BYTES];
    Grp s(smem, threadIdx.x);
    const int k = blockIdx.x, r = blockIdx.y, t0 = k * kB;
    const long long block = (long long)r * g.blocks + k;
    PeakRecord* rec = g.rec + block;
    if (rec->bad) return;
    const int n = g.T - t0 < kB ? g.T - t0 : kB;
    const float* x = g.in + r * g.in_pitch;
    const float* e = g.energy ? g.energy + r * g.energy_pitch : nullptr;
    int halo = g.pre_max > g.post_max ? g.pre_max : g.post_max;
    halo = halo > g.pre_avg ? halo : g.pre_avg;
    halo = halo > g.post_avg ? halo : g.post_avg;
    const int lo = t0 - halo > 0 ? t0 - halo : 0, hi = t0 + n + halo < g.T ? t0 + n + halo : g.T;          // hi - lo <= kB + 2 kReach
    const float mn = rec->mn, range = rec->mx - mn;
    for (int t = lo + threadIdx.x; t < hi; t += kThreads) s.y[t - lo] = normalised(x[t], mn, range, g.normalise);
    __syncthreads();
    bool c[E], m[E];
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int o = s.l + j * kThreads;
        c[j] = o < n && s.candidate(g, t0 + o, lo);
        m[j] = o < n && e && is_minimum(e, t0 + o, g.T);
        g.flags[block * kB + o] = c[j];
        if (g.candidate && o < n) g.candidate[r * g.candidate_pitch + t0 + o] = c[j];
    }
    __syncthreads();          // y has been read
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int o = s.l + j * kThreads;
        s.nxt[o] = c[j] ? o : kEnd;
        s.lm[o] = m[j] ? o + 1 : 0;
    }
    if (s.l < 4) s.nxt[kB + s.l] = kEnd;
    __syncthreads();
    s.scans(n, e != nullptr);
    s.tables(n, g.wait);
    for (int o = s.l; o < g.offsets; o += kThreads) {
        int last = 0;
        const int count = s.chain(o < n ? s.nxt[o] : kEnd, &last);
        g.words[block * g.offsets + o] = (unsigned)count << 16 | (unsigned)last;
    }
    if (s.l == 0) rec->block_min = e && s.lm[n - 1] ? t0 + s.lm[n - 1] - 1 : -1;
}

// a lane a row: the chain through the blocks.  One dependent read per block the chain enters; a wait that passes whole blocks reads nothing there.
__global__ __launch_bounds__(64) void peak_carry_kernel(PeakK g) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= g.rows) return;
    PeakRecord* rec = g.rec + (long long)r * g.blocks;
    if (rec[0].bad) {
        g.n_peaks[r] = -1;
        return;
    }
    const unsigned* words = g.words + (long long)r * g.blocks * g.offsets;
    int enter = 0, run = 0, carried = -1;          // the chain enters at `enter`, a frame at or behind the block's first
    for (int k = 0; k < g.blocks; ++k) {
        const int t0 = k * kB, end = t0 + kB < g.T ? t0 + kB : g.T;
        const int block_min = g.energy ? rec[k].block_min : -1;
        int count = 0, at = end;
        if (enter < end) {
            at = enter;
            const unsigned w = words[(long long)k * g.offsets + (enter - t0)];
            count = (int)(w >> 16);
            if (count) enter = t0 + (int)(w & 0xffff) + g.wait + 1;
            enter = enter > end ? enter : end;
        }
        rec[k].enter = at, rec[k].run = run, rec[k].count = count, rec[k].carried_min = carried;
        run += count;
        carried = block_min >= 0 ? block_min : carried;
    }
    g.n_peaks[r] = run;
}

// a block: the tables again, lane i writes the block's i-th peak and its back()
__global__ __launch_bounds__(kThreads) void peak_emit_kernel(PeakK g) {
    using Grp = Group<kB, kThreads>;
    constexpr int E = Grp::E;
    __shared__ __attribute__((aligned(16))) char smem[JSGX_PEAK_LDS_BYTES];
    Grp s(smem, threadIdx.x);
    const int k = blockIdx.x, r = blockIdx.y, t0 = k * kB;
    const long long block = (long long)r * g.blocks + k;
    const PeakRecord rec = g.rec[block];
    if (rec.bad || rec.count == 0 || rec.run >= g.max_peaks) return;
    const int n = g.T - t0 < kB ? g.T - t0 : kB;
    const float* e = g.energy ? g.energy + r * g.energy_pitch : nullptr;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int o = s.l + j * kThreads;
        s.nxt[o] = g.flags[block * kB + o] ? o : kEnd;
        s.lm[o] = o < n && e && is_minimum(e, t0 + o, g.T) ? o + 1 : 0;
    }
    if (s.l < 4) s.nxt[kB + s.l] = kEnd;
    __syncthreads();
    s.scans(n, e != nullptr);
    s.tables(n, g.wait);
    const unsigned short f = s.nxt[rec.enter - t0];
    for (int i = s.l; i < rec.count && rec.run + i < g.max_peaks; i += kThreads) {
        const int p = s.pick(f, i);
        const long long at = r * g.peaks_pitch + rec.run + i;
        g.peaks[at] = t0 + p;
        if (g.back) g.back[at] = s.lm[p] ? t0 + s.lm[p] - 1 : rec.carried_min;
    }
}

}  // namespace

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_peak_launch(const jsgx_peak_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_peak_launch";
    PeakSpans spans;
    int rc = peak_check(g, who, &spans);
    if (rc == JSGX_OK) rc = peak_check_scratch(g, who, spans, scratch, scratch_bytes);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const PeakPlan plan = peak_plan(g);
    const bool many = g->rows > 1;
    PeakK k{};
    k.in = g->in, k.in_pitch = many ? g->in_pitch : 0;
    k.energy = g->energy, k.energy_pitch = many ? g->energy_pitch : 0;
    k.candidate = g->candidate, k.candidate_pitch = many ? g->candidate_pitch : 0;
    k.peaks = g->peaks, k.back = g->backtracked, k.peaks_pitch = many ? g->peaks_pitch : 0;
    k.n_peaks = g->n_peaks;
    char* base = static_cast<char*>(scratch);
    k.rec = reinterpret_cast<PeakRecord*>(base), k.words = reinterpret_cast<unsigned*>(base + plan.off_words);
    k.flags = reinterpret_cast<unsigned char*>(base + plan.off_flags);
    k.rows = g->rows, k.T = g->n_frames, k.blocks = (int)plan.blocks, k.offsets = (int)plan.offsets;
    k.pre_max = g->pre_max, k.post_max = g->post_max, k.pre_avg = g->pre_avg, k.post_avg = g->post_avg;
    k.delta = g->delta, k.wait = g->wait, k.normalise = g->normalise, k.max_peaks = g->max_peaks;
    const dim3 lanes(kThreads);
    if (plan.blocks == 1) {
        if (g->n_frames <= kShort)
            hipLaunchKernelGGL((peak_single_kernel<kShort, 64>), dim3((unsigned)((g->rows + 3) / 4)), lanes, 0, s, k);
        else
            hipLaunchKernelGGL((peak_single_kernel<kB, kThreads>), dim3((unsigned)g->rows), lanes, 0, s, k);
    } else {
        const dim3 per_block((unsigned)plan.blocks, (unsigned)g->rows);
        hipLaunchKernelGGL(peak_stats_kernel, per_block, lanes, 0, s, k);
        hipLaunchKernelGGL(peak_row_kernel, dim3((unsigned)g->rows), lanes, 0, s, k);
        hipLaunchKernelGGL(peak_cand_kernel, per_block, lanes, 0, s, k);
        hipLaunchKernelGGL(peak_carry_kernel, dim3((unsigned)((g->rows + 63) / 64)), dim3(64), 0, s, k);
        hipLaunchKernelGGL(peak_emit_kernel, per_block, lanes, 0, s, k);
    }
    return finish_launch(who, hipGetLastError());
}
