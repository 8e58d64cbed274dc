// libjsgx.so, per-channel energy normalisation (include/jsgx.h section 13): the kernels and the launcher.  A lane owns one chain: one
// band of one chunk of JSGX_PCEN_CHUNK frames of one row.  The chains are numbered (row, chunk, band) with the band fastest and dealt to
// the lanes in that order, so a wavefront reads 64 neighbouring floats of a frame wherever 64 bands or more lie side by side, and with
// fewer bands it holds several chunks or rows: no lane idles but in the last workgroup.  The scratch is indexed by the same number.
//
//   "pcen_scan"   every chunk but a row's last: the 256 dependent fmaf of p from +0; the loads and the b * M products do not depend
//                 on the chain and are issued 16 frames ahead.  The last p goes to the scratch.
//   "pcen_carry"  one lane a (row, band): s_(c+1) = fmaf(q[255], s_c, p_c) over the chunks; the entering state replaces p in the scratch
//   "pcen_apply"  every chunk: p again, S = fmaf(q[j], s, p), the compression, the stores; the row's last frame goes to state_out.
//                 The compression is some 170 vector operations a value and p is two, so here four lanes share a chain: each runs
//                 p from the chunk's start (the same chain, the same bits) and compresses its own 64 frames.  A small plane has
//                 four times the wavefronts for it, a large one pays a few per cent.
// A row of one chunk takes "pcen_apply" alone, with the entering state read where "pcen_carry" reads it.
#include "jsgx_internal.h"

namespace jsgx {

namespace {

constexpr int kThreads = JSGX_PCEN_THREADS;
constexpr int kChunk = JSGX_PCEN_CHUNK;
constexpr int kAhead = 16;          // frames of a chain in flight in "pcen_scan"
constexpr int kParts = 4, kPart = kChunk / kParts;          // "pcen_apply": the lanes of a chain and the frames of each
static_assert(kChunk % kAhead == 0 && kPart % kAhead == 0, "a chunk and a part are whole groups of loads");

struct PcenK {
    const float* in;
    long long frame_pitch, row_pitch;
    const float* decay;
    const float* state_in;
    long long state_in_pitch;
    float* state_out;
    long long state_out_pitch;
    float* smooth;
    long long smooth_frame_pitch, smooth_row_pitch;
    float* out;
    long long out_frame_pitch, out_row_pitch;
    float* scratch;
    long long chains, chunks;
    int bands, frames;
    float a, b, neg_gain, bias, power, eps;
};

// the chain of a lane
struct Chain {
    long long row, chunk, band;
};
__device__ __forceinline__ Chain chain_of(const PcenK& g, long long i) {
    Chain c;
    if (g.chains <= 0x7fffffffLL) {          // the common case: 32-bit division
        const unsigned u = (unsigned)i, rc = u / (unsigned)g.bands;
        c.band = u % (unsigned)g.bands, c.chunk = rc % (unsigned)g.chunks, c.row = rc / (unsigned)g.chunks;
    } else {
        const long long rc = i / g.bands;
        c.band = i % g.bands, c.chunk = rc % g.chunks, c.row = rc / g.chunks;
    }
    return c;
}

// the state that enters a row: state_in where given, else the row's first frame
__device__ __forceinline__ float entering(const PcenK& g, long long row, long long band) {
    return g.state_in ? g.state_in[row * g.state_in_pitch + band] : g.in[row * g.row_pitch + band];
}

// out of M and S as the header states it: every product and sum rounded on its own
__device__ __forceinline__ float compress(const PcenK& g, float m, float s, float d) {
#pragma clang fp contract(off)
    const float gn = exp_any(g.neg_gain * log_pos(g.eps + s));
    const float y = g.bias + m * gn;
    return exp_any(g.power * log_pos(y)) - d;
}

__global__ __launch_bounds__(kThreads) void pcen_scan_kernel(PcenK g) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= g.chains) return;
    const Chain c = chain_of(g, i);
    if (c.chunk == g.chunks - 1) return;          // nothing follows a row's last chunk; every other chunk is whole
    const float* x = g.in + c.row * g.row_pitch + c.chunk * kChunk * g.frame_pitch + c.band;
    float now[kAhead], next[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) now[u] = x[u * g.frame_pitch];
    float p = 0.f;
    for (int j = 0; j < kChunk; j += kAhead) {
        const float* ahead = x + (j + kAhead < kChunk ? j + kAhead : j) * g.frame_pitch;          // the last group reads itself again
#pragma unroll
        for (int u = 0; u < kAhead; ++u) next[u] = ahead[u * g.frame_pitch];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) p = __builtin_fmaf(g.a, p, g.b * now[u]);
#pragma unroll
        for (int u = 0; u < kAhead; ++u) now[u] = next[u];
    }
    g.scratch[i] = p;
}

__global__ __launch_bounds__(kThreads) void pcen_carry_kernel(PcenK g) {
    const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (k >= g.chains / g.chunks) return;
    const long long row = k / g.bands, band = k % g.bands;
    float s = entering(g, row, band);
    float* e = g.scratch + row * g.chunks * g.bands + band;
    const float q = g.decay[kChunk - 1];
    const long long n = g.chunks - 1;          // the chunks whose p the scan left
    long long c = 0;
    for (; c + 8 <= n; c += 8) {
        float p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = e[(c + u) * g.bands];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            e[(c + u) * g.bands] = s;
            s = __builtin_fmaf(q, s, p[u]);
        }
    }
    for (; c < n; ++c) {
        const float p = e[c * g.bands];
        e[c * g.bands] = s;
        s = __builtin_fmaf(q, s, p);
    }
    e[n * g.bands] = s;
}

template <bool SINGLE>
__global__ __launch_bounds__(kThreads) void pcen_apply_kernel(PcenK g) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= g.chains * kParts) return;
    // (row, chunk, part, band), the band fastest
    long long row, chunk, band;
    int part;
    if (g.chains * kParts <= 0x7fffffffLL) {          // the common case: 32-bit division
        const unsigned u = (unsigned)i, t = u / (unsigned)g.bands, rc = t / kParts;
        band = u % (unsigned)g.bands, part = (int)(t % kParts), chunk = rc % (unsigned)g.chunks, row = rc / (unsigned)g.chunks;
    } else {
        const long long t = i / g.bands, rc = t / kParts;
        band = i % g.bands, part = (int)(t % kParts), chunk = rc % g.chunks, row = rc / g.chunks;
    }
    const long long t0 = chunk * kChunk;
    const int len = g.frames - t0 < kChunk ? (int)(g.frames - t0) : kChunk;
    const int first = part * kPart, last = first + kPart < len ? first + kPart : len;          // this lane's frames of the chunk
    if (first >= len) return;
    const float* x = g.in + row * g.row_pitch + t0 * g.frame_pitch + band;
    float* out = g.out + row * g.out_row_pitch + t0 * g.out_frame_pitch + band;
    float* smooth = g.smooth ? g.smooth + row * g.smooth_row_pitch + t0 * g.smooth_frame_pitch + band : nullptr;
    const float s = SINGLE ? entering(g, row, band) : g.scratch[(row * g.chunks + chunk) * g.bands + band];
    const float d = exp_any(g.power * log_pos(g.bias));
    float p = 0.f, S = s;
    // p up to this lane's first frame: whole groups, as in "pcen_scan"
    for (int j = 0; j < first; j += kAhead) {
        float v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = x[(j + u) * g.frame_pitch];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) p = __builtin_fmaf(g.a, p, g.b * v[u]);
    }
    int j = first;
    // the next four frames are on their way from memory while these four are compressed
    float m[4], next[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) m[u] = x[(j + u < last ? j + u : j) * g.frame_pitch];
    for (; j + 4 <= last; j += 4) {
        float sm[4], o[4];
        const float* ahead = x + (j + 8 <= last ? j + 4 : j) * g.frame_pitch;          // the last whole group reads itself again
#pragma unroll
        for (int u = 0; u < 4; ++u) next[u] = ahead[u * g.frame_pitch];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            p = __builtin_fmaf(g.a, p, g.b * m[u]);
            sm[u] = __builtin_fmaf(g.decay[j + u], s, p);
        }
        // four independent compressions in one block, for the scheduler to interleave; the stores behind them
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = compress(g, m[u], sm[u], d);
#pragma unroll
        for (int u = 0; u < 4; ++u) out[(j + u) * g.out_frame_pitch] = o[u];
        if (smooth) {
#pragma unroll
            for (int u = 0; u < 4; ++u) smooth[(j + u) * g.smooth_frame_pitch] = sm[u];
        }
        S = sm[3];
#pragma unroll
        for (int u = 0; u < 4; ++u) m[u] = next[u];
    }
    for (; j < last; ++j) {
        const float v = x[j * g.frame_pitch];
        p = __builtin_fmaf(g.a, p, g.b * v);
        S = __builtin_fmaf(g.decay[j], s, p);
        out[j * g.out_frame_pitch] = compress(g, v, S, d);
        if (smooth) smooth[j * g.smooth_frame_pitch] = S;
    }
    if (g.state_out && chunk == g.chunks - 1 && last == len) g.state_out[row * g.state_out_pitch + band] = S;
}

}  // namespace

}  // namespace jsgx

using namespace jsgx;

extern "C" int jsgx_pcen_launch(const jsgx_pcen_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsgx_pcen_launch";
    PcenSpans spans;
    int rc = pcen_check(g, who, &spans);
    if (rc == JSGX_OK) rc = pcen_check_scratch(g, who, spans, scratch, scratch_bytes);
    if (rc != JSGX_OK) return rc;
    int dev = -1;
    if ((rc = current_device(&dev, who)) != JSGX_OK) return rc;
    // every refusal is behind us
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const PcenPlan plan = pcen_plan(g);
    const bool many = g->rows > 1;
    PcenK k{};
    k.in = g->in, k.frame_pitch = g->frame_pitch, k.row_pitch = many ? g->row_pitch : 0;
    k.decay = g->decay;
    k.state_in = g->state_in, k.state_in_pitch = many ? g->state_in_pitch : 0;
    k.state_out = g->state_out, k.state_out_pitch = many ? g->state_out_pitch : 0;
    k.smooth = g->smooth_out, k.smooth_frame_pitch = g->smooth_frame_pitch, k.smooth_row_pitch = many ? g->smooth_row_pitch : 0;
    k.out = g->out, k.out_frame_pitch = g->out_frame_pitch, k.out_row_pitch = many ? g->out_row_pitch : 0;
    k.scratch = static_cast<float*>(scratch);
    k.chains = plan.chains, k.chunks = plan.chunks;
    k.bands = g->n_bands, k.frames = g->n_frames;
    k.a = 1.0f - g->b, k.b = g->b, k.neg_gain = -g->gain, k.bias = g->bias, k.power = g->power, k.eps = g->eps;
    const dim3 per_chain((unsigned)((plan.chains + kThreads - 1) / kThreads)), per_part((unsigned)((plan.chains * kParts + kThreads - 1) / kThreads));
    if (plan.chunks == 1) {
        hipLaunchKernelGGL(pcen_apply_kernel<true>, per_part, dim3(kThreads), 0, s, k);
    } else {
        const long long states = (long long)g->rows * g->n_bands;
        hipLaunchKernelGGL(pcen_scan_kernel, per_chain, dim3(kThreads), 0, s, k);
        hipLaunchKernelGGL(pcen_carry_kernel, dim3((unsigned)((states + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, k);
        hipLaunchKernelGGL(pcen_apply_kernel<false>, per_part, dim3(kThreads), 0, s, k);
    }
    return finish_launch(who, hipGetLastError());
}
