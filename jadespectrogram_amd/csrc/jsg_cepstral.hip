// libjsg.so, cepstral coefficients and delta features (include/jsg.h, section 2k).  A unit of its own; the refusals, the plan of a
// projection, the DCT tables and the delta weights are in jsg_cepstral_host.cpp.
//
// mfcc_kernel: 256 threads (four waves), dynamic LDS, no scratch, no atomics.  A workgroup brings the whole table D[M][B] into LDS once
// and then walks work items (row, F <= 64 consecutive frames) with a grid stride.  An item stages its F x B tile with coalesced loads
// (16 bytes wide where the pointer, the pitches and B allow, else 4; the same bits either way) into rows of P = B | 1 floats, so that
// lane f reading S[f][b] meets 64 different banks.  Then lane f of every wave owns frame f and wave w the coefficient blocks w, w + 4,
// ... of MB coefficients: for b ascending it reads S[f][b] (four b at a time) and MB table rows (one address for the wave: a
// broadcast, 16 bytes = four b wide where B is a multiple of 4) and runs acc[q] = fmaf(D[m0+q][b], S[f][b], acc[q]).  Per coefficient b
// simply ascends; two register sets take turns, so the reads of the next four b are under way during the multiply-adds of these (with
// one set every step waited for its own reads).  A block past M repeats row M-1 and is not stored.  The sums go to LDS rows of M | 1 floats; after a barrier all
// threads store them coalesced.  MB (4, 5, 8, 10 or 16, by M alone) is the smallest that gives each wave at most one block, so the
// usual 20 coefficients are four blocks of 5.  Small tiles on purpose: 64 x 128 -> 20 is 48 KB, three workgroups per compute unit, so
// the staging of one overlaps the sums of the others; the kernel is bound by memory and by LDS reads, not by the multiply-adds.  Where a
// thread's share of a tile is at most eight 16-byte pieces, the next item's tile is loaded into registers before the sums of this one
// and written to LDS after them (profiles/cepstral_bench.md has what each step bought).  The grid is what the device holds at a time, by
// the LDS of the call and the registers of the instantiation.
//
// delta_kernel: 256 threads; an item is (row, FC frames) with FC * M about 4096 elements; lanes run along m within a frame and on
// across frames, so loads and stores are coalesced.  The weights sit in LDS (one address for the wave); the Wd-fold re-read of X comes
// from the caches.
//
// Every float operation of the definitions is written out (contraction is off; the fused multiply-add is explicit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

struct MfArgs {
    const float* in;
    long long frame_pitch, row_pitch;
    const float* table;
    float* out;
    long long out_frame_pitch, out_row_pitch;
    long long n_items, chunks;              // chunks = ceil(T / F) per row
    int T, B, M, F, vec, pre;               // vec: 16-byte loads of the tile; pre: through registers, one item ahead
};

// The operands of the four steps b .. b + 3 (b a multiple of 4, rows of the table 16-byte aligned): S[f][b ..] of the lane's frame and
// D[m0 + q][b ..] of the MB rows (one address for the wave), and their multiply-adds, b ascending per coefficient.
template <int MB>
__device__ __forceinline__ void mf_fetch(const float* dp, const int (&row)[MB], const float* s, int b, float4 (&d)[MB], float (&sv)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) sv[i] = s[b + i];
#pragma unroll
    for (int q = 0; q < MB; ++q) d[q] = *reinterpret_cast<const float4*>(dp + row[q] + b);
}

template <int MB>
__device__ __forceinline__ void mf_fma(const float4 (&d)[MB], const float (&sv)[4], float (&acc)[MB]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < MB; ++q) {
        acc[q] = __builtin_fmaf(d[q].x, sv[0], acc[q]);
        acc[q] = __builtin_fmaf(d[q].y, sv[1], acc[q]);
        acc[q] = __builtin_fmaf(d[q].z, sv[2], acc[q]);
        acc[q] = __builtin_fmaf(d[q].w, sv[3], acc[q]);
    }
}

// A thread's share of the tile of Fc frames at src, 16 bytes a piece: the pieces tid, tid + 256, ... in the order (frame, piece of the
// frame), at most kMfccPre of them.
constexpr int kMfccPre = 8;
__device__ __forceinline__ void mf_prefetch(const float* src, long long frame_pitch, int Fc, int f, int q, int df, int dq, int Bq, float4 (&pre)[kMfccPre]) {
#pragma unroll
    for (int i = 0; i < kMfccPre; ++i) {
        if (f < Fc) pre[i] = *reinterpret_cast<const float4*>(src + (long long)f * frame_pitch + q * 4);
        q += dq, f += df;
        if (q >= Bq) q -= Bq, ++f;
    }
}

template <int MB>
__global__ __launch_bounds__(kMfccThreads) void mfcc_kernel(const MfArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float mf_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.B, M = a.M, P = B | 1, MP = M | 1;
    float* const dp = mf_lds;               // the table: 16-byte aligned rows where B % 4 == 0
    float* const sp = dp + M * B;           // the tile
    float* const op = sp + a.F * P;         // the sums
    for (int e = tid; e < M * B; e += kMfccThreads) dp[e] = a.table[e];
    const int mblocks = (M + MB - 1) / MB;
    // thread tid takes the elements tid, tid + 256, ... of a tile of Bq pieces per frame, and of the F x M sums
    const int Wv = a.vec ? 4 : 1, Bq = B / Wv;
    const int lf0 = tid / Bq, lq0 = tid - lf0 * Bq, ldf = kMfccThreads / Bq, ldq = kMfccThreads - ldf * Bq;
    const int sf0 = tid / M, sm0 = tid - sf0 * M, sdf = kMfccThreads / M, sdm = kMfccThreads - sdf * M;
    // pre: where a thread's share of a tile is at most kMfccPre 16-byte pieces (a.pre), the next item's tile travels from memory into
    // these registers while the sums of this one run, and goes to LDS when the waves have left them
    float4 pre[kMfccPre];
    if (a.pre && blockIdx.x < a.n_items) {
        const long long r = blockIdx.x / a.chunks;
        const int t0 = (int)(blockIdx.x - r * a.chunks) * a.F;
        mf_prefetch(a.in + r * a.row_pitch + (long long)t0 * a.frame_pitch, a.frame_pitch, min(a.F, a.T - t0), lf0, lq0, ldf, ldq, Bq, pre);
    }
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long r = item / a.chunks;
        const int t0 = (int)(item - r * a.chunks) * a.F;          // < T
        const int Fc = min(a.F, a.T - t0);
        const float* src = a.in + r * a.row_pitch + (long long)t0 * a.frame_pitch;
        if (a.pre) {
            int f = lf0, q = lq0;
#pragma unroll
            for (int i = 0; i < kMfccPre; ++i) {
                if (f < Fc) {
                    float* to = sp + f * P + q * 4;
                    to[0] = pre[i].x, to[1] = pre[i].y, to[2] = pre[i].z, to[3] = pre[i].w;
                }
                q += ldq, f += ldf;
                if (q >= Bq) q -= Bq, ++f;
            }
        } else {
            for (int f = lf0, q = lq0; f < Fc;) {
                const float* from = src + (long long)f * a.frame_pitch + q * Wv;
                float* to = sp + f * P + q * Wv;
                if (a.vec) {
                    const float4 v = *reinterpret_cast<const float4*>(from);
                    to[0] = v.x, to[1] = v.y, to[2] = v.z, to[3] = v.w;
                } else {
                    to[0] = from[0];
                }
                q += ldq, f += ldf;
                if (q >= Bq) q -= Bq, ++f;
            }
        }
        __syncthreads();
        if (a.pre && item + gridDim.x < a.n_items) {
            const long long rn = (item + gridDim.x) / a.chunks;
            const int tn = (int)(item + gridDim.x - rn * a.chunks) * a.F;
            mf_prefetch(a.in + rn * a.row_pitch + (long long)tn * a.frame_pitch, a.frame_pitch, min(a.F, a.T - tn), lf0, lq0, ldf, ldq, Bq, pre);
        }
        for (int k = wave; k < mblocks; k += kMfccThreads / 64) {
            const int m0 = k * MB;
            const float* s = sp + min(lane, Fc - 1) * P;
            int row[MB];
            float acc[MB];
#pragma unroll
            for (int q = 0; q < MB; ++q) {
                row[q] = min(m0 + q, M - 1) * B;
                acc[q] = 0.f;
            }
            if ((B & 3) == 0) {
                // two register sets in turn: the reads of the next four b are under way while the multiply-adds of these four run
                float4 dA[MB], dB[MB];
                float sA[4], sB[4];
                mf_fetch<MB>(dp, row, s, 0, dA, sA);
                for (int b = 0; b < B; b += 8) {
                    mf_fetch<MB>(dp, row, s, min(b + 4, B - 4), dB, sB);          // past the end: the last four again, not used
                    mf_fma<MB>(dA, sA, acc);
                    if (b + 4 < B) {
                        mf_fetch<MB>(dp, row, s, min(b + 8, B - 4), dA, sA);
                        mf_fma<MB>(dB, sB, acc);
                    }
                }
            } else {
                for (int b = 0; b < B; ++b) {
                    const float sb = s[b];
#pragma unroll
                    for (int q = 0; q < MB; ++q) acc[q] = __builtin_fmaf(dp[row[q] + b], sb, acc[q]);
                }
            }
            if (lane < Fc) {
#pragma unroll
                for (int q = 0; q < MB; ++q)
                    if (m0 + q < M) op[lane * MP + m0 + q] = acc[q];
            }
        }
        __syncthreads();
        float* dst = a.out + r * a.out_row_pitch + (long long)t0 * a.out_frame_pitch;
        for (int f = sf0, m = sm0; f < Fc;) {
            dst[(long long)f * a.out_frame_pitch + m] = op[f * MP + m];
            m += sdm, f += sdf;
            if (m >= M) m -= M, ++f;
        }
        // the next item's tile is written after every wave has left the sums above (the barrier before the stores), and its sums after
        // every thread has left these stores (the barrier after its staging)
    }
}

struct DlArgs {
    const float* in;
    long long frame_pitch, row_pitch;
    const float* weights;
    float* out;
    long long out_frame_pitch, out_row_pitch;
    long long n_items, chunks;              // chunks = ceil(T / FC) per row
    int T, M, Wd, mode, FC;
};

__global__ __launch_bounds__(256) void delta_kernel(const DlArgs a) {
#pragma clang fp contract(off)
    __shared__ float w[JSG_DELTA_MAX_WIDTH + 1];
    const int tid = threadIdx.x;
    for (int e = tid; e < a.Wd; e += 256) w[e] = a.weights[e];
    __syncthreads();
    const int M = a.M, Wd = a.Wd, h = Wd / 2;
    const int f0 = tid / M, m0 = tid - f0 * M, df = 256 / M, dm = 256 - df * M;
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long r = item / a.chunks;
        const long long t0 = (item - r * a.chunks) * a.FC;        // < T
        const int Fc = (int)min((long long)a.FC, a.T - t0);
        const float* row = a.in + r * a.row_pitch;
        float* dst = a.out + r * a.out_row_pitch;
        for (int f = f0, m = m0; f < Fc;) {
            const long long t = t0 + f;
            float acc = 0.f;
            if (a.mode == JSG_DELTA_EDGE_INTERP) {
                const long long s = min(max(t - h, 0ll), (long long)a.T - Wd);
                const float* p = row + s * a.frame_pitch + m;
#pragma unroll 4
                for (int j = 0; j < Wd; ++j) acc = __builtin_fmaf(w[j], p[j * a.frame_pitch], acc);
            } else {
#pragma unroll 4
                for (int j = 0; j < Wd; ++j) {
                    const long long fr = min(max(t - h + j, 0ll), (long long)a.T - 1);
                    acc = __builtin_fmaf(w[j], row[fr * a.frame_pitch + m], acc);
                }
            }
            dst[t * a.out_frame_pitch + m] = acc;
            m += dm, f += df;
            if (m >= M) m -= M, ++f;
        }
    }
}

}  // namespace jsg

using namespace jsg;

namespace {

// The grid is what a compute unit holds at a time, by the LDS of this call and by the registers of this instantiation, so that no
// workgroup waits for another to end (each stages the table and takes a fixed share of the items).
template <int MB>
hipError_t mfcc_enqueue(const MfArgs& k, int dev, long long by_lds, size_t lds_bytes, hipStream_t s) {
    static std::atomic<int> by_regs[64];        // workgroups per compute unit that the registers allow, per device; asked once
    int regs = dev >= 0 && dev < 64 ? by_regs[dev].load(std::memory_order_acquire) : 0;
    if (regs < 1) {
        const hipError_t err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&regs, mfcc_kernel<MB>, kMfccThreads, 0);
        if (err != hipSuccess) return err;
        regs = std::max(1, regs);
        if (dev >= 0 && dev < 64) by_regs[dev].store(regs, std::memory_order_release);
    }
    const dim3 grid(resident_grid(k.n_items, dev, std::max<long long>(1, std::min<long long>(by_lds, regs))));
    static OncePerDevice told;      // of this path: one bit
    return launch_large_lds(told, dev, 1u, mfcc_kernel<MB>, kMfccLdsOne * 4, grid, dim3(kMfccThreads), lds_bytes, s, k);
}

}  // namespace

extern "C" int jsg_mfcc_launch(const jsg_mfcc_args* g, void* stream) {
    static const char* who = "jsg_mfcc_launch";
    int dev = -1;
    int rc = mfcc_check(g, who);
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    MfccPlan p{};
    mfcc_resolve(g, &p);
    MfArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.frame_pitch = g->frame_pitch;
    k.row_pitch = multi ? g->row_pitch : 0;
    k.table = g->table;
    k.out = g->out;
    k.out_frame_pitch = g->out_frame_pitch;
    k.out_row_pitch = multi ? g->out_row_pitch : 0;
    k.n_items = (long long)g->rows * p.chunks;
    k.chunks = p.chunks;
    k.T = (int)g->n_frames;
    k.B = g->n_in;
    k.M = g->n_out;
    k.F = p.F;
    k.vec = (g->n_in % 4 == 0) && (reinterpret_cast<uintptr_t>(g->in) % 16 == 0) && (g->frame_pitch % 4 == 0) && (k.row_pitch % 4 == 0);
    k.pre = k.vec && ((long long)p.F * (g->n_in / 4) + kMfccThreads - 1) / kMfccThreads <= kMfccPre;
    const size_t lds_bytes = sizeof(float) * (size_t)p.lds_floats;
    // tests/test_gpu_cepstral_grid.py reads the cap from the next line
    const long long by_lds = std::min<long long>(8, kMfccLdsOne / p.lds_floats);      // 2048 threads per compute unit
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const hipError_t err = p.MB == 4 ? mfcc_enqueue<4>(k, dev, by_lds, lds_bytes, s)
                         : p.MB == 5 ? mfcc_enqueue<5>(k, dev, by_lds, lds_bytes, s)
                         : p.MB == 8 ? mfcc_enqueue<8>(k, dev, by_lds, lds_bytes, s)
                         : p.MB == 10 ? mfcc_enqueue<10>(k, dev, by_lds, lds_bytes, s)
                                      : mfcc_enqueue<16>(k, dev, by_lds, lds_bytes, s);
    return err == hipSuccess ? JSG_OK : jsg_fail_hip(err, who);
}

extern "C" int jsg_delta_launch(const jsg_delta_args* g, void* stream) {
    static const char* who = "jsg_delta_launch";
    int dev = -1;
    int rc = delta_check(g, who);
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    DlArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.frame_pitch = g->frame_pitch;
    k.row_pitch = multi ? g->row_pitch : 0;
    k.weights = g->weights;
    k.out = g->out;
    k.out_frame_pitch = g->out_frame_pitch;
    k.out_row_pitch = multi ? g->out_row_pitch : 0;
    k.T = (int)g->n_frames;
    k.M = g->n_coeffs;
    k.Wd = g->width;
    k.mode = g->mode;
    k.FC = std::max(1, 4096 / g->n_coeffs);
    k.chunks = (g->n_frames + k.FC - 1) / k.FC;
    k.n_items = (long long)g->rows * k.chunks;
    hipLaunchKernelGGL(delta_kernel, dim3(resident_grid(k.n_items, dev, 8)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), k);
    return finish_launch(who);
}
