// libjsg.so, phase vocoder (include/jsg.h, section 2e): complex frames in, time-stretched complex frames out.  A unit of its own:
// no kernel, launcher or table of the other units is touched.
//
// Lanes run along the bins, so every load and store of a frame is coalesced in the caller's frame-major buffer.  A work item is
// (row, chunk of output frames, tile of 64 bins); one wavefront takes one item at a time and walks the items with a grid stride.
//
//   pvoc_walk_kernel<false>  pass 1: the sum of the phase increments of every chunk but the last, as uint32 fixed point (2^32 units
//                 = one turn), to scratch [row][chunk][bin].
//   pvoc_scan_kernel         pass 2: per (row, bin) the exclusive prefix of the chunk sums, starting from phi_0 = arg X[0], in place.
//                 A workgroup takes 64 bins x 16 segments of the chunk axis: segment totals through LDS, then a second walk.
//   pvoc_walk_kernel<true>   pass 3: the same walk as pass 1 from the chunk's prefix, with the interpolated magnitude and
//                 sincosf of the accumulated phase, 8-byte non-temporal stores.
//
// The phase is summed in integers, so the result has the same bits for every chunk length, grid, row count and pitch; no workgroup
// waits for another one and there are no atomics.  An input frame's angle and magnitude are computed once per chunk where it serves
// as a1 of one step and a0 of the next, and a pair that several output frames share (rate < 1) is computed once with its increment.
// The frames of the next step are loaded before the arithmetic of the current one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

typedef float pv_v2 __attribute__((ext_vector_type(2)));

constexpr int PV_TILE = 64;          // bins per work item = lanes of a wavefront
constexpr int PV_SEGS = 16;          // segments of the chunk axis in the scan kernel
constexpr float PV_INV_2PI = 0.15915494309189533577f;
constexpr float PV_2PI_OVER_2_32 = 1.4629180792671596e-9f;   // 2 pi / 2^32

struct PvArgs {
    const pv_v2* in;
    long long in_frame_pitch, in_row_pitch;     // complex elements
    pv_v2* out;
    long long out_frame_pitch, out_row_pitch;
    unsigned* pre;              // scratch [row][chunk][bin]: chunk sums, then exclusive prefixes
    long long T, T_out;         // input frames, output frames
    long long chunks, n_items;  // n_items = rows * walked chunks * tiles (the scan: rows * tiles)
    double rate;
    int K, tiles, chunk, n, hop;
};

// a phase in turns -> fixed point, 2^32 units per turn (the conversion of section 2e; wraps mod 2^32)
__device__ inline unsigned pv_fixed(double turns) { return (unsigned)(long long)llrint(turns * 4294967296.0); }

// the increment of one step in fixed point: wrap(arg a1 - arg a0 - A_k) + A_k with A_k = adv turns
__device__ inline unsigned pv_increment(float ang0, float ang1, double adv) {
#pragma clang fp contract(off)
    const float df = ang1 - ang0;
    double u = (double)(df * PV_INV_2PI);
    u -= adv;
    u -= round(u);
    u += adv;
    return pv_fixed(u);
}

__device__ inline pv_v2 pv_load(const pv_v2* row, long long pitch, int j, long long T, int k, bool live) {
    return (live && j < T) ? row[(long long)j * pitch + k] : pv_v2{0.f, 0.f};
}

// OUT = false: chunk sums (pass 1, the last chunk of a row is not walked).  OUT = true: the output frames (pass 3).
template <bool OUT>
__global__ __launch_bounds__(PV_TILE) void pvoc_walk_kernel(const PvArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const long long walked = OUT ? a.chunks : a.chunks - 1;
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int tile = (int)(item % a.tiles);
        const long long rc = item / a.tiles;
        const long long c = rc % walked, row = rc / walked;
        const int k = tile * PV_TILE + lane;
        const bool live = k < a.K;
        const long long i0 = c * a.chunk, i1 = min(a.T_out, i0 + a.chunk);
        const pv_v2* src = a.in + row * a.in_row_pitch;
        const double adv = (double)(((long long)a.hop * k) % a.n) / (double)a.n;
        unsigned acc = 0;
        if (OUT && live) acc = a.pre[(row * a.chunks + c) * a.K + k];
        pv_v2* dst = OUT ? a.out + row * a.out_row_pitch + k : nullptr;

        int j = (int)floor((double)i0 * a.rate);   // below T < 2^31
        pv_v2 r0 = pv_load(src, a.in_frame_pitch, j, a.T, k, live), r1 = pv_load(src, a.in_frame_pitch, j + 1, a.T, k, live);
        float ang0 = atan2f(r0.y, r0.x), ang1 = atan2f(r1.y, r1.x);
        float mag0 = OUT ? hypotf(r0.x, r0.y) : 0.f, mag1 = OUT ? hypotf(r1.x, r1.y) : 0.f;
        unsigned inc = pv_increment(ang0, ang1, adv);
        for (long long i = i0; i < i1; ++i) {
            // the frames of step i + 1, requested before the arithmetic of step i (j and jn are the same in every lane)
            const int jn = (i + 1 < i1) ? (int)floor((double)(i + 1) * a.rate) : j;
            if (jn != j) {
                r1 = pv_load(src, a.in_frame_pitch, jn + 1, a.T, k, live);
                if (jn != j + 1) r0 = pv_load(src, a.in_frame_pitch, jn, a.T, k, live);
            }
            if (OUT) {
                const double t = (double)i * a.rate;
                const float alpha = (float)(t - (double)j);
                const float m = alpha * mag1 + (1.0f - alpha) * mag0;
                float sn, cs;
                sincosf((float)(int)acc * PV_2PI_OVER_2_32, &sn, &cs);
                if (live) __builtin_nontemporal_store(pv_v2{m * cs, m * sn}, dst + i * a.out_frame_pitch);
            }
            acc += inc;
            if (jn != j) {
                if (jn == j + 1) {
                    ang0 = ang1;
                    mag0 = mag1;
                } else {
                    ang0 = atan2f(r0.y, r0.x);
                    if (OUT) mag0 = hypotf(r0.x, r0.y);
                }
                ang1 = atan2f(r1.y, r1.x);
                if (OUT) mag1 = hypotf(r1.x, r1.y);
                inc = pv_increment(ang0, ang1, adv);
                j = jn;
            }
        }
        if (!OUT && live) a.pre[(row * a.chunks + c) * a.K + k] = acc;
    }
}

// Exclusive prefixes of the chunk sums of one (row, tile of bins), in place, starting from phi_0: thread (lane, seg) sums the
// chunks of its segment, the segment totals meet in LDS, and a second walk writes the prefixes.  The last chunk has no sum.
__global__ __launch_bounds__(PV_TILE * PV_SEGS) void pvoc_scan_kernel(const PvArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned s_tot[PV_SEGS][PV_TILE];
    const int lane = threadIdx.x % PV_TILE, seg = threadIdx.x / PV_TILE;
    const long long per = (a.chunks + PV_SEGS - 1) / PV_SEGS;
    const long long c0 = min(a.chunks, seg * per), c1 = min(a.chunks, c0 + per);
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long row = item / a.tiles;
        const int k = (int)(item % a.tiles) * PV_TILE + lane;
        const bool live = k < a.K;
        unsigned* p = a.pre + row * a.chunks * a.K + k;
        unsigned tot = 0;
        if (live)
            for (long long c = c0; c < min(c1, a.chunks - 1); ++c) tot += p[c * a.K];
        s_tot[seg][lane] = tot;
        __syncthreads();
        if (live) {
            const pv_v2 x0 = a.in[row * a.in_row_pitch + k];
            unsigned carry = pv_fixed((double)(atan2f(x0.y, x0.x) * PV_INV_2PI));
            for (int s = 0; s < seg; ++s) carry += s_tot[s][lane];
            for (long long c = c0; c < c1; ++c) {
                const unsigned s = c < a.chunks - 1 ? p[c * a.K] : 0u;
                p[c * a.K] = carry;
                carry += s;
            }
        }
        __syncthreads();
    }
}

}  // namespace jsg

using namespace jsg;

namespace {

struct PvCall {
    long long K, tiles, chunk, chunks;
    long long scratch_bytes;
};

// the number of i >= 0 with (double)i * rate < T, for T in 1..2^31-1 and a finite rate > 0; -1 where it exceeds 2^31-1
long long pvoc_count(long long T, double rate) {
#pragma clang fp contract(off)
    const double q = (double)T / rate;
    if (!(q < 4294967296.0)) return -1;
    long long g = (long long)std::ceil(q);
    while (g > 0 && (double)(g - 1) * rate >= (double)T) --g;
    while ((double)g * rate < (double)T) ++g;
    return g < (1ll << 31) ? g : -1;
}

// the default chunk: about 8192 work items (32 wavefronts on each of 256 compute units), 16..1024 output frames.  It depends on the
// sizes of the call only, so the scratch size can be asked for without a device.
long long default_chunk(long long T_out, long long rows, long long tiles) {
    const i128 want = ((i128)T_out * rows * tiles + 8191) / 8192;
    return (long long)std::max<i128>(16, std::min<i128>(1024, want));
}

bool rate_ok(double rate) { return std::isfinite(rate) && rate > 0.0; }

int pvoc_check(const jsg_pvoc_args* g, const char* who, PvCall* c) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in || !g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null data pointer");
    if (g->n < 2 || g->n > 65536 || (g->n & 1)) return jsg_fail_who(JSG_ERR_INVALID, who, "n must be even and in 2..65536");
    if (g->hop < 1 || g->hop > g->n) return jsg_fail_who(JSG_ERR_INVALID, who, "hop must be in 1..n");
    if (const int rc = check_rows(g->rows, who); rc != JSG_OK) return rc;
    if (!rate_ok(g->rate)) return jsg_fail_who(JSG_ERR_INVALID, who, "rate must be finite and > 0");
    if (g->n_frames_in < 1 || g->n_frames_in >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames_in must be in 1..2^31-1");
    const long long T = g->n_frames_in, T_out = pvoc_count(T, g->rate);
    if (T_out < 1) return jsg_fail_who(JSG_ERR_INVALID, who, "the output would have more than 2^31-1 frames");
    if (g->n_frames_out != T_out) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames_out differs from jsg_pvoc_frames(n_frames_in, rate)");
    if (g->chunk_frames < 0 || g->chunk_frames > 65536) return jsg_fail_who(JSG_ERR_INVALID, who, "chunk_frames must be 0 or in 1..65536");
    const long long K = g->n / 2 + 1;
    if (g->in_frame_pitch < K) return jsg_fail_who(JSG_ERR_INVALID, who, "in_frame_pitch smaller than n/2+1");
    if (g->out_frame_pitch < K) return jsg_fail_who(JSG_ERR_INVALID, who, "out_frame_pitch smaller than n/2+1");
    const i128 in_row = plane(T, g->in_frame_pitch, K), out_row = plane(T_out, g->out_frame_pitch, K);
    if (g->rows > 1 && g->in_row_pitch < in_row) return jsg_fail_who(JSG_ERR_INVALID, who, "in_row_pitch smaller than one row of frames");
    if (g->rows > 1 && g->out_row_pitch < out_row) return jsg_fail_who(JSG_ERR_INVALID, who, "out_row_pitch smaller than one row of frames");
    const uintptr_t pi = reinterpret_cast<uintptr_t>(g->in), po = reinterpret_cast<uintptr_t>(g->out);
    if ((pi & 7) != 0 || (po & 7) != 0) return jsg_fail_who(JSG_ERR_INVALID, who, "in and out must be 8-byte aligned (complex float pairs)");
    if (overlap(addr(g->in), span_bytes(g->rows, g->in_row_pitch, in_row, 8), addr(g->out), span_bytes(g->rows, g->out_row_pitch, out_row, 8)))
        return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps in");
    c->K = K;
    c->tiles = (K + PV_TILE - 1) / PV_TILE;
    c->chunk = g->chunk_frames ? g->chunk_frames : default_chunk(T_out, g->rows, c->tiles);
    c->chunks = (T_out + c->chunk - 1) / c->chunk;
    const i128 bytes = ((i128)g->rows * c->chunks * K * 4 + 15) / 16 * 16;
    if (bytes >= ((i128)1 << 62)) return jsg_fail_who(JSG_ERR_INVALID, who, "the scratch of this chunk length would exceed 2^62 bytes");
    c->scratch_bytes = (long long)bytes;
    return JSG_OK;
}

}  // namespace

extern "C" {

int64_t jsg_pvoc_frames(int64_t n_frames_in, double rate) {
    if (n_frames_in < 1 || n_frames_in >= (1ll << 31)) return jsg_fail(JSG_ERR_INVALID, "jsg_pvoc_frames: n_frames_in must be in 1..2^31-1");
    if (!rate_ok(rate)) return jsg_fail(JSG_ERR_INVALID, "jsg_pvoc_frames: rate must be finite and > 0");
    const long long t = pvoc_count(n_frames_in, rate);
    if (t < 1) return jsg_fail(JSG_ERR_INVALID, "jsg_pvoc_frames: the output would have more than 2^31-1 frames");
    return t;
}

int64_t jsg_pvoc_scratch_bytes(const jsg_pvoc_args* g) {
    PvCall c{};
    const int rc = pvoc_check(g, "jsg_pvoc_scratch_bytes", &c);
    return rc != JSG_OK ? rc : c.scratch_bytes;
}

int jsg_pvoc_launch(const jsg_pvoc_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsg_pvoc_launch";
    PvCall c{};
    int rc = pvoc_check(g, who, &c);
    if (rc != JSG_OK) return rc;
    if (!scratch) return jsg_fail_who(JSG_ERR_INVALID, who, "null scratch");
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) != 0) return jsg_fail_who(JSG_ERR_INVALID, who, "scratch must be 16-byte aligned");
    if (scratch_bytes < c.scratch_bytes) return jsg_fail_who(JSG_ERR_INVALID, who, "scratch smaller than jsg_pvoc_scratch_bytes");
    int dev = -1;
    rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    PvArgs k{};
    k.in = reinterpret_cast<const pv_v2*>(g->in);
    k.in_frame_pitch = g->in_frame_pitch;
    k.in_row_pitch = g->rows > 1 ? g->in_row_pitch : 0;
    k.out = reinterpret_cast<pv_v2*>(g->out);
    k.out_frame_pitch = g->out_frame_pitch;
    k.out_row_pitch = g->rows > 1 ? g->out_row_pitch : 0;
    k.pre = static_cast<unsigned*>(scratch);
    k.T = g->n_frames_in;
    k.T_out = g->n_frames_out;
    k.chunks = c.chunks;
    k.rate = g->rate;
    k.K = (int)c.K;
    k.tiles = (int)c.tiles;
    k.chunk = (int)c.chunk;
    k.n = g->n;
    k.hop = g->hop;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long per_cu = 64;   // twice the wavefronts a compute unit holds
    const long long per_chunk = (long long)g->rows * c.tiles;
    if (c.chunks > 1) {
        k.n_items = per_chunk * (c.chunks - 1);
        hipLaunchKernelGGL(pvoc_walk_kernel<false>, dim3(resident_grid(k.n_items, dev, per_cu)), dim3(PV_TILE), 0, s, k);
        rc = finish_launch(who);
        if (rc != JSG_OK) return rc;
    }
    k.n_items = per_chunk;
    hipLaunchKernelGGL(pvoc_scan_kernel, dim3(resident_grid(k.n_items, dev, per_cu)), dim3(PV_TILE * PV_SEGS), 0, s, k);
    rc = finish_launch(who);
    if (rc != JSG_OK) return rc;
    k.n_items = per_chunk * c.chunks;
    hipLaunchKernelGGL(pvoc_walk_kernel<true>, dim3(resident_grid(k.n_items, dev, per_cu)), dim3(PV_TILE), 0, s, k);
    return finish_launch(who);
}

}  // extern "C"
