// libjsg.so, constant-Q and variable-Q spectrograms by direct evaluation in the time domain (include/jsg.h, section 2h).  A unit of its
// own: no kernel, launcher or table of the other units is touched.  The standard basis is built in jsg_cqt_host.cpp.
//
// One kernel, 256 threads (four waves) per workgroup, no scratch, no atomics, no workgroup waits on another.  Bins are served in
// classes by length (class c: 2^(c-1) < N_k <= 2^c), longest class first.  A work item is (row, chunk of F consecutive frames, bin);
// F is sized on the host per class, inversely to the class's length and within the LDS, so that items carry similar work, and
// workgroups walk the items with a grid stride.  Neighbouring items are the bins of one class over the same frames: they read the
// same input span, which L2 serves.
//
// An item stages the input its frames need into LDS with coalesced loads: the contiguous span where hop < taps of a pass (the
// windows overlap), else the F windows back to back.  Then lanes lie along the taps: with W = 64 (N_k > 32) or the smallest power
// of two >= N_k, lane l of a group of W takes the taps i = l, l + W, ..., loads each coefficient once (through L2, coalesced) and
// uses it for CQ_FR frames, whose input it reads from LDS at consecutive addresses (conflict-free for any hop).  A wave holds 64 / W
// groups, so short bins fill the wave with frames.  One cross-lane halving tree per (bin, frame) ends the sum; lane 0 of a group
// stores.  Where N_k exceeds CQ_PASS_TAPS the taps are walked in passes (stage, accumulate, stage, ...) with the lane accumulators
// kept across the passes; such an item holds at most one sweep of frames (4 waves x CQ_FR).  The order of every sum thus depends
// on k and the tap index alone.
//
// Every float operation of the definition is written out (contraction is off; the fused multiply-adds are explicit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "jsg_internal.h"

namespace jsg {
struct CqBin {
    long long offset;          // of the bin's first tap, in complex elements
    int half, k;
};
}  // namespace jsg

struct jsg_cqt {
    int K = 0;
    long long total = 0;
    jsg::DeviceBlob blob;                  // taps[2 * total] floats, then bins[K]
    const float2* d_taps = nullptr;
    const jsg::CqBin* d_bins = nullptr;    // the bins, longest class first (ascending k inside a class)
    std::vector<int32_t> half;             // host copy
};

namespace jsg {

constexpr int CQ_THREADS = 256;
constexpr int CQ_WAVES = CQ_THREADS / 64;
constexpr int CQ_FR = 4;                    // frames a lane accumulates at a time
constexpr int CQ_UNROLL = 8;                // taps of a lane in flight at a time on frames without an edge
constexpr int CQ_STAGE = 4;                 // input samples a thread has in flight while a span is staged
constexpr int CQ_LDS_FLOATS = 20480;        // 80 KiB: two workgroups per compute unit
constexpr int CQ_PASS_TAPS = 12288;         // taps staged at a time, at most
constexpr int CQ_ITEM_WORK = 1 << 17;       // taps x frames an item aims at
constexpr int CQ_MAX_FRAMES = 4096;         // frames per item, at most, where the caller does not say

struct CqClass {
    int n_max;                 // the largest N_k of the class
    int n_bins, first;         // bins of the class: bins[first .. first + n_bins)
    int F, P, S;               // frames per item, taps per pass, LDS floats between the windows of neighbouring frames
    long long chunks;          // ceil(T / F)
    int lds_floats;
};

struct CqArgs {
    const float* in;
    long long in_pitch;
    float* out;
    long long frame_pitch, row_pitch;      // in output elements
    const float2* taps;
    const CqBin* bins;
    long long n_items;
    int L, T, hop;                         // L, T < 2^31, hop <= 2^20
    int power, n_classes;
    long long first_item[JSG_CQT_MAX_CLASSES + 1];
    int chunks[JSG_CQT_MAX_CLASSES];       // ceil(T / F) < 2^31
    int n_bins[JSG_CQT_MAX_CLASSES], first[JSG_CQT_MAX_CLASSES], F[JSG_CQT_MAX_CLASSES], P[JSG_CQT_MAX_CLASSES], S[JSG_CQT_MAX_CLASSES];
};

__host__ __device__ inline int cq_lane_width(int N) {        // W_k of the header
    int W = 1;
    while (W < 64 && W < N) W <<= 1;
    return W;
}

// taps i = i0, i0 + W, ... below i1 of one lane for its CQ_FR frames.  EDGE: some tap of some frame of the wave may be not live.
// W64: W is 64 and no frame has an edge: the hot form, unrolled with constant offsets
template <bool EDGE, bool W64>
__device__ __forceinline__ void cq_accumulate(const float2* __restrict__ ck, const float* xs, int i0, int i1, int Wk, const int (&base)[CQ_FR],
                                     const int (&lo)[CQ_FR], const int (&hi)[CQ_FR], float (&re)[CQ_FR], float (&im)[CQ_FR]) {
#pragma clang fp contract(off)
    const int W = W64 ? 64 : Wk;
    int i = i0;
    if (W64) {
        // CQ_UNROLL coefficients and their input samples are in flight at a time (the loads come first, the sums follow in tap order)
        for (; i + (CQ_UNROLL - 1) * W < i1; i += CQ_UNROLL * W) {
            float2 c[CQ_UNROLL];
            float x[CQ_FR][CQ_UNROLL];
#pragma unroll
            for (int u = 0; u < CQ_UNROLL; ++u) c[u] = ck[i + u * W];
#pragma unroll
            for (int q = 0; q < CQ_FR; ++q)
#pragma unroll
                for (int u = 0; u < CQ_UNROLL; ++u) x[q][u] = xs[base[q] + i + u * W];
#pragma unroll
            for (int u = 0; u < CQ_UNROLL; ++u)
#pragma unroll
                for (int q = 0; q < CQ_FR; ++q) {
                    re[q] = __builtin_fmaf(x[q][u], c[u].x, re[q]);
                    im[q] = __builtin_fmaf(x[q][u], c[u].y, im[q]);
                }
        }
    }
    for (; i < i1; i += W) {
        const float2 c = ck[i];
#pragma unroll
        for (int q = 0; q < CQ_FR; ++q) {
            if (!EDGE || (i >= lo[q] && i < hi[q])) {
                const float x = xs[base[q] + i];
                re[q] = __builtin_fmaf(x, c.x, re[q]);
                im[q] = __builtin_fmaf(x, c.y, im[q]);
            }
        }
    }
}

__global__ __launch_bounds__(CQ_THREADS) void cqt_kernel(const CqArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float cq_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        int c = 0;
#pragma nounroll
        while (c + 1 < a.n_classes && item >= a.first_item[c + 1]) ++c;      // read from the argument block one at a time
        const long long local = item - a.first_item[c];
        const int nb = a.n_bins[c];
        const long long rest = local / nb;
        const CqBin bin = a.bins[a.first[c] + (int)(local - rest * nb)];
        const int k = bin.k;
        const int row = (int)(rest / a.chunks[c]), chunk = (int)(rest - (long long)row * a.chunks[c]);
        const int F = a.F[c], P = a.P[c], S = a.S[c];
        const int h = bin.half, N = 2 * h + 1;
        const float2* ck = a.taps + bin.offset;
        const int W = cq_lane_width(N), G = 64 / W;
        const int g = lane / W, j = lane - g * W;
        const int t0 = chunk * F;          // < T
        const int Fc = min(F, a.T - t0);
        const float* src = a.in + (long long)row * a.in_pitch;
        const int per_sweep = CQ_WAVES * G * CQ_FR;
        // N > P (passes): the host gives such a class F <= per_sweep, one sweep
        for (int s0 = 0; s0 < Fc; s0 += per_sweep) {
            int f[CQ_FR], lo[CQ_FR], hi[CQ_FR], base[CQ_FR];
            float re[CQ_FR], im[CQ_FR];
            bool edge = false;
#pragma unroll
            for (int q = 0; q < CQ_FR; ++q) {
                f[q] = s0 + q * (CQ_WAVES * G) + wave * G + g;
                re[q] = im[q] = 0.f;
                lo[q] = hi[q] = 0;
                if (f[q] < Fc) {
                    const long long pos = (long long)(t0 + f[q]) * a.hop - h;        // the sample under tap 0
                    lo[q] = (int)min(max(-pos, 0ll), (long long)N);
                    hi[q] = (int)min(max((long long)a.L - pos, 0ll), (long long)N);
                }
                edge = edge || lo[q] != 0 || hi[q] != N;
            }
            const bool any_edge = __any(edge);
            for (int p0 = 0; p0 < N; p0 += P) {
                const int Np = min(P, N - p0);
                if (p0 > 0 || s0 == 0) {
                    __syncthreads();        // the span of the item or pass before has been read
                    const int total = (Fc - 1) * S + Np;
                    const long long origin = (long long)t0 * a.hop - h + p0;
                    for (int e0 = tid; e0 < total; e0 += CQ_STAGE * CQ_THREADS) {
                        float v[CQ_STAGE];
                        unsigned ok = 0;        // one bit per sample, not a lane mask each in scalar registers
#pragma unroll
                        for (int u = 0; u < CQ_STAGE; ++u) {
                            const int e = e0 + u * CQ_THREADS;
                            long long m = origin + e;
                            if (S != a.hop) {       // windows back to back
                                const int fe = min(e / S, Fc - 1);
                                m = origin + (long long)fe * a.hop + (e - fe * S);
                            }
                            const bool in = e < total && m >= 0 && m < a.L;
                            ok |= (in ? 1u : 0u) << u;
                            v[u] = in ? src[m] : 0.f;
                        }
#pragma unroll
                        for (int u = 0; u < CQ_STAGE; ++u)
                            if (ok >> u & 1u) cq_lds[e0 + u * CQ_THREADS] = v[u];
                    }
                    __syncthreads();
                }
#pragma unroll
                for (int q = 0; q < CQ_FR; ++q) base[q] = f[q] * S - p0;
                if (any_edge)
                    cq_accumulate<true, false>(ck, cq_lds, p0 + j, p0 + Np, W, base, lo, hi, re, im);
                else if (W == 64)
                    cq_accumulate<false, true>(ck, cq_lds, p0 + j, p0 + Np, W, base, lo, hi, re, im);
                else
                    cq_accumulate<false, false>(ck, cq_lds, p0 + j, p0 + Np, W, base, lo, hi, re, im);
            }
#pragma unroll
            for (int q = 0; q < CQ_FR; ++q) {
                if (W == 64) {
#pragma unroll
                    for (int s = 32; s >= 1; s >>= 1) {
                        re[q] = re[q] + __shfl_xor(re[q], s);
                        im[q] = im[q] + __shfl_xor(im[q], s);
                    }
                } else {
                    for (int s = W >> 1; s >= 1; s >>= 1) {
                        re[q] = re[q] + __shfl_xor(re[q], s);
                        im[q] = im[q] + __shfl_xor(im[q], s);
                    }
                }
                if (j == 0 && f[q] < Fc) {
                    const long long at = (long long)row * a.row_pitch + (long long)(t0 + f[q]) * a.frame_pitch + k;       // in output elements
                    if (a.power) {
                        const float rr = re[q] * re[q], ii = im[q] * im[q];
                        a.out[at] = rr + ii;
                    } else {
                        reinterpret_cast<float2*>(a.out)[at] = make_float2(re[q], im[q]);
                    }
                }
            }
        }
    }
}

}  // namespace jsg

using namespace jsg;

namespace {

int cq_class_of(int N) {        // 2^(c-1) < N <= 2^c
    int c = 0;
    while ((1 << c) < N) ++c;
    return c;
}

// the refusals that need no basis
int cqt_check(const jsg_cqt_args* g, const char* who) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in || !g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null data pointer");
    if (g->out_power != 0 && g->out_power != 1) return jsg_fail_who(JSG_ERR_INVALID, who, "out_power must be 0 or 1");
    const uintptr_t pi = reinterpret_cast<uintptr_t>(g->in), po = reinterpret_cast<uintptr_t>(g->out);
    if ((pi & 3) != 0) return jsg_fail_who(JSG_ERR_INVALID, who, "in must be 4-byte aligned");
    if ((po & (g->out_power ? 3 : 7)) != 0) return jsg_fail_who(JSG_ERR_INVALID, who, "out must be 8-byte aligned (power: 4-byte)");
    if (const int rc = check_rows(g->rows, who); rc != JSG_OK) return rc;
    if (g->in_samples < 1 || g->in_samples >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "in_samples must be in 1..2^31-1");
    if (g->hop < 1 || g->hop > (1ll << 20)) return jsg_fail_who(JSG_ERR_INVALID, who, "hop must be in 1..2^20");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (g->chunk_frames < 0 || g->chunk_frames > 65536) return jsg_fail_who(JSG_ERR_INVALID, who, "chunk_frames must be 0 or in 1..65536");
    if (g->rows > 1 && g->in_pitch < g->in_samples) return jsg_fail_who(JSG_ERR_INVALID, who, "in_pitch smaller than in_samples");
    return JSG_OK;
}

// the refusals that need K
int cqt_check_out(int K, const jsg_cqt_args* g, const char* who) {
    if (g->out_frame_pitch < K) return jsg_fail_who(JSG_ERR_INVALID, who, "out_frame_pitch smaller than the number of bins");
    const i128 row_min = plane(g->n_frames, g->out_frame_pitch, K);
    if (g->rows > 1 && (i128)g->out_row_pitch < row_min) return jsg_fail_who(JSG_ERR_INVALID, who, "out_row_pitch smaller than (n_frames-1)*out_frame_pitch + bins");
    if (overlap(addr(g->in), span_bytes(g->rows, g->in_pitch, g->in_samples, 4), addr(g->out), span_bytes(g->rows, g->out_row_pitch, row_min, g->out_power ? 4 : 8)))
        return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps in");
    return JSG_OK;
}

int cqt_check_sizes(int K, const int32_t* half, const char* who, long long* total) {
    if (K < 1 || K > JSG_CQT_MAX_BINS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bins must be in 1..4096");
    if (!half) return jsg_fail_who(JSG_ERR_INVALID, who, "null half_len");
    long long sum = 0;
    for (int k = 0; k < K; ++k) {
        if (half[k] < 0 || half[k] > JSG_CQT_MAX_HALF_LEN) return jsg_fail_who(JSG_ERR_INVALID, who, "half_len must be in 0..131072");
        sum += 2ll * half[k] + 1;
    }
    if (sum > JSG_CQT_MAX_TAPS) return jsg_fail_who(JSG_ERR_INVALID, who, "the basis has more than 2^24 taps");
    if (total) *total = sum;
    return JSG_OK;
}

// Frames per item, taps per pass and the LDS of one class of largest length n_max.  A pass stages P = min(n_max, CQ_PASS_TAPS) taps per
// frame; the windows of neighbouring frames lie S = min(hop, P) floats apart (the contiguous span, or back to back), so F frames need
// (F - 1) S + P floats.  F aims at CQ_ITEM_WORK / n_max frames, in whole sweeps, is bounded by chunk_frames, by T and by what
// CQ_LDS_FLOATS holds, and by one sweep where the taps take several passes (the accumulators of one sweep live in registers).
// P <= 12288 leaves room for (F - 1) S of at least 8192 floats: 1 <= F, 1 <= P, lds_floats <= CQ_LDS_FLOATS always.
void cqt_size_class(CqClass* c, const jsg_cqt_args* g) {
    const int N = c->n_max;
    const int per_sweep = CQ_WAVES * (64 / cq_lane_width(N)) * CQ_FR;
    c->P = std::min(N, CQ_PASS_TAPS);
    c->S = (int)std::min<long long>(g->hop, c->P);
    long long want = g->chunk_frames;
    if (!want) {
        want = (CQ_ITEM_WORK + N - 1) / N;
        want = std::min<long long>(CQ_MAX_FRAMES, (want + per_sweep - 1) / per_sweep * per_sweep);
    }
    if (N > c->P) want = std::min<long long>(want, per_sweep);
    want = std::min<long long>(want, g->n_frames);
    const long long fit = 1 + (CQ_LDS_FLOATS - c->P) / c->S;
    long long F = std::max<long long>(1, std::min(want, fit));
    if (!g->chunk_frames && F > per_sweep) F = F / per_sweep * per_sweep;
    c->F = (int)F;
    c->chunks = (g->n_frames + F - 1) / F;
    c->lds_floats = (int)((F - 1) * c->S + c->P);
}

struct CqPlan {
    int n_classes = 0;
    CqClass cls[JSG_CQT_MAX_CLASSES];
    bool passes = false;
    int lds_floats = 0;
};

// the classes that hold bins, longest first, sized for the call
int cqt_resolve(int K, const int32_t* half, const jsg_cqt_args* g, const char* who, CqPlan* p) {
    int count[JSG_CQT_MAX_CLASSES] = {}, n_max[JSG_CQT_MAX_CLASSES] = {};
    for (int k = 0; k < K; ++k) {
        const int N = 2 * half[k] + 1, c = cq_class_of(N);
        ++count[c];
        n_max[c] = std::max(n_max[c], N);
    }
    int first = 0;
    for (int c = JSG_CQT_MAX_CLASSES - 1; c >= 0; --c) {
        if (!count[c]) continue;
        CqClass& o = p->cls[p->n_classes++];
        o.n_max = n_max[c];
        o.n_bins = count[c];
        o.first = first;
        first += count[c];
        cqt_size_class(&o, g);
        p->passes = p->passes || o.n_max > o.P;
        p->lds_floats = std::max(p->lds_floats, o.lds_floats);
        // a pass of no frames or no taps would never end on the device and an LDS request above the limit fails at the launch
        if (o.F < 1 || o.P < 1 || o.S < 1 || o.lds_floats > CQ_LDS_FLOATS) return jsg_fail_who(JSG_ERR_INVALID, who, "internal: no pass of this call fits the LDS");
    }
    return JSG_OK;
}

const char* path_name(const CqPlan& p) { return p.passes ? "cqt_passes" : "cqt_span"; }

int cqt_make(jsg_cqt** out, int K, const int32_t* half, const float* taps, long long total, const char* who) {
    std::unique_ptr<jsg_cqt> p(new (std::nothrow) jsg_cqt());
    if (!p) return jsg_fail_who(JSG_ERR_NOMEM, who, "out of host memory");
    p->K = K;
    p->total = total;
    p->half.assign(half, half + K);
    int rc = p->blob.bind(who);
    if (rc != JSG_OK) return rc;
    // the kernel may ask for more than 48 KB of dynamic LDS: said once per device, here, so that a first launch may sit inside a capture
    const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(&cqt_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CQ_LDS_FLOATS * 4);
    if (err != hipSuccess) return jsg_fail_hip(err, who);
    (void)cu_count_of_device(p->blob.device());      // read once per device, here and not inside a first launch
    // one allocation: the taps, then the bins in the order they are served
    const size_t taps_bytes = sizeof(float) * 2 * (size_t)total;
    std::vector<char> host(taps_bytes + sizeof(CqBin) * (size_t)K);
    std::memcpy(host.data(), taps, taps_bytes);
    CqBin* bins = reinterpret_cast<CqBin*>(host.data() + taps_bytes);
    std::vector<long long> off(K);
    long long at = 0;
    for (int k = 0; k < K; ++k) {
        off[k] = at;
        at += 2ll * half[k] + 1;
    }
    int n = 0;
    for (int c = JSG_CQT_MAX_CLASSES - 1; c >= 0; --c)
        for (int k = 0; k < K; ++k)
            if (cq_class_of(2 * half[k] + 1) == c) bins[n++] = CqBin{off[k], half[k], k};
    rc = p->blob.upload(host.data(), host.size(), who);
    if (rc != JSG_OK) return rc;
    const char* d = static_cast<const char*>(p->blob.data());
    p->d_taps = reinterpret_cast<const float2*>(d);
    p->d_bins = reinterpret_cast<const CqBin*>(d + taps_bytes);
    *out = p.release();
    return JSG_OK;
}

}  // namespace

extern "C" {

int jsg_cqt_create(jsg_cqt** out, const jsg_cqt_spec* spec) {
    static const char* who = "jsg_cqt_create";
    if (!out) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    *out = nullptr;
    int64_t total = 0;
    int rc = jsg_cqt_basis_build(spec, nullptr, nullptr, nullptr, nullptr, 0, &total);
    if (rc != JSG_OK) return rc;
    std::vector<int32_t> half(spec->n_bins);
    std::vector<float> taps(2 * (size_t)total);
    rc = jsg_cqt_basis_build(spec, half.data(), nullptr, nullptr, taps.data(), total, &total);
    if (rc != JSG_OK) return rc;
    return cqt_make(out, spec->n_bins, half.data(), taps.data(), total, who);
}

int jsg_cqt_create_tables(jsg_cqt** out, int n_bins, const int32_t* half_len, const float* taps) {
    static const char* who = "jsg_cqt_create_tables";
    if (!out) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    *out = nullptr;
    long long total = 0;
    const int rc = cqt_check_sizes(n_bins, half_len, who, &total);
    if (rc != JSG_OK) return rc;
    if (!taps) return jsg_fail_who(JSG_ERR_INVALID, who, "null taps");
    return cqt_make(out, n_bins, half_len, taps, total, who);
}

int jsg_cqt_destroy(jsg_cqt* cq) {
    delete cq;
    return JSG_OK;
}

int jsg_cqt_bins(const jsg_cqt* cq) { return cq ? cq->K : jsg_fail(JSG_ERR_INVALID, "jsg_cqt_bins: null"); }
int64_t jsg_cqt_total_taps(const jsg_cqt* cq) { return cq ? cq->total : jsg_fail(JSG_ERR_INVALID, "jsg_cqt_total_taps: null"); }
int jsg_cqt_half_len(const jsg_cqt* cq, int32_t* out) {
    if (!cq || !out) return jsg_fail(JSG_ERR_INVALID, "jsg_cqt_half_len: null");
    std::copy(cq->half.begin(), cq->half.end(), out);
    return JSG_OK;
}

int64_t jsg_cqt_frames(int64_t in_samples, int64_t hop) {
    if (in_samples < 1 || in_samples >= (1ll << 31)) return jsg_fail(JSG_ERR_INVALID, "jsg_cqt_frames: in_samples must be in 1..2^31-1");
    if (hop < 1 || hop > (1ll << 20)) return jsg_fail(JSG_ERR_INVALID, "jsg_cqt_frames: hop must be in 1..2^20");
    return 1 + in_samples / hop;
}

int jsg_cqt_launch(const jsg_cqt* cq, const jsg_cqt_args* g, void* stream) {
    static const char* who = "jsg_cqt_launch";
    if (g && !cq) return jsg_fail_who(JSG_ERR_INVALID, who, "null basis");
    int dev = -1;
    int rc = cqt_check(g, who);
    // the basis is read only once there is a device
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc == JSG_OK) rc = cqt_check_out(cq->K, g, who);
    if (rc != JSG_OK) return rc;
    if (cq->blob.device() != dev) return jsg_fail_who(JSG_ERR_INVALID, who, "the basis was created on another device");
    CqPlan p;
    rc = cqt_resolve(cq->K, cq->half.data(), g, who, &p);
    if (rc != JSG_OK) return rc;
    CqArgs k{};
    k.in = g->in;
    k.in_pitch = g->rows > 1 ? g->in_pitch : 0;
    k.out = static_cast<float*>(g->out);
    k.frame_pitch = g->out_frame_pitch;
    k.row_pitch = g->rows > 1 ? g->out_row_pitch : 0;
    k.taps = cq->d_taps;
    k.bins = cq->d_bins;
    k.L = (int)g->in_samples;
    k.T = (int)g->n_frames;
    k.hop = (int)g->hop;
    k.power = g->out_power;
    k.n_classes = p.n_classes;
    long long items = 0;
    for (int c = 0; c < p.n_classes; ++c) {
        const CqClass& o = p.cls[c];
        k.first_item[c] = items;
        items += (long long)g->rows * o.chunks * o.n_bins;
        k.chunks[c] = (int)o.chunks;
        k.n_bins[c] = o.n_bins;
        k.first[c] = o.first;
        k.F[c] = o.F;
        k.P[c] = o.P;
        k.S[c] = o.S;
    }
    k.first_item[p.n_classes] = items;
    k.n_items = items;
    const size_t lds_bytes = sizeof(float) * (size_t)p.lds_floats;
    const dim3 grid(resident_grid(items, dev, per_cu_by_lds(160 * 1024, (long long)lds_bytes, 8)));      // 2048 threads per compute unit
    hipLaunchKernelGGL(cqt_kernel, grid, dim3(CQ_THREADS), lds_bytes, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who);
}

int jsg_cqt_plan(int n_bins, const int32_t* half_len, const jsg_cqt_args* g, char* name, int name_len, int32_t* n_classes, int32_t* class_max_taps,
                 int32_t* frames_per_item, int32_t* taps_per_pass, int32_t* lds_bytes) {
    static const char* who = "jsg_cqt_plan";
    int rc = check_name_buffer(who, name, name_len, false);
    if (rc == JSG_OK) rc = cqt_check_sizes(n_bins, half_len, who, nullptr);
    if (rc == JSG_OK) rc = cqt_check(g, who);
    if (rc == JSG_OK) rc = cqt_check_out(n_bins, g, who);
    CqPlan p;
    if (rc == JSG_OK) rc = cqt_resolve(n_bins, half_len, g, who, &p);
    if (rc != JSG_OK) return rc;
    put_path_name(name, name_len, path_name(p));
    if (n_classes) *n_classes = p.n_classes;
    for (int c = 0; c < p.n_classes; ++c) {
        if (class_max_taps) class_max_taps[c] = p.cls[c].n_max;
        if (frames_per_item) frames_per_item[c] = p.cls[c].F;
        if (taps_per_pass) taps_per_pass[c] = p.cls[c].P;
        if (lds_bytes) lds_bytes[c] = 4 * p.cls[c].lds_floats;
    }
    return JSG_OK;
}

int jsg_cqt_kernel_name(const jsg_cqt* cq, const jsg_cqt_args* g, char* out, int out_len) {
    static const char* who = "jsg_cqt_kernel_name";
    if (const int rn = check_name_buffer(who, out, out_len, true); rn != JSG_OK) return rn;
    if (g && !cq) return jsg_fail_who(JSG_ERR_INVALID, who, "null basis");
    int rc = cqt_check(g, who);          // before the basis is read
    if (rc == JSG_OK) rc = cqt_check_out(cq->K, g, who);
    CqPlan p;
    if (rc == JSG_OK) rc = cqt_resolve(cq->K, cq->half.data(), g, who, &p);
    if (rc != JSG_OK) return rc;
    put_path_name(out, out_len, path_name(p));
    return JSG_OK;
}

}  // extern "C"
