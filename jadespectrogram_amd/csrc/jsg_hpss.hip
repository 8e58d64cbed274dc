// libjsg.so, harmonic-percussive separation by median filtering (include/jsg.h, section 2f).  A unit of its own: no kernel,
// launcher or table of the other units is touched.
//
// Two kernels, one wavefront per workgroup, work items walked with a grid stride; no atomics, no workgroup waits on another.
//
//   hpss_freq_kernel   item = (row, block of 64 frames, tile of 64 bins).  The power of the block's frames over the tile plus a
//                 halo of h_f bins either side (reflect indices resolved at load, lanes along bins: coalesced) goes to an LDS tile
//                 [64 frames][65 + 2 h_f] as sortable keys.  The pitch is odd, so the transposed reads are conflict-free.  Then a lane
//                 takes one FRAME and slides a sorted window along the bins; the median of output bin m overwrites the tile column
//                 that has just left the window.  The tile is written to the scratch plane C[row][frame][bin] with lanes along bins.
//   hpss_time_kernel   item = (row, chunk of frames, tile of 64 bins), a lane takes one BIN and slides a sorted window along the
//                 frames, starting h_t frames before the chunk.  Each step loads the frame that enters and the one that leaves
//                 (recomputed from the input: the same operations give the same bits), and for the output frame the input, C and the
//                 masks.  The loads of step t + 1 are requested before the window work of step t.
//
// The sorted window of a lane (HpWindow) lives in LDS as [W][64] (lane-major: conflict-free) for a length given at run time.  A step
// replaces the first element equal to the leaving value by the entering one while a forward pass carries the maximum up, then a
// backward pass carries the minimum down: the array is sorted again after 2 W reads and 2 W writes whatever the values.  For the
// default length 31 both kernels have an instantiation that keeps the window in 31 registers (the same three passes, unrolled, no LDS
// traffic).  The elements are keys, a monotone map of the float bits to unsigned integers, so the order is total: a NaN is an
// ordinary (large) key, the leaving value is always found, and nothing of it stays behind once it has left.  A window that holds no
// NaN, Inf or negative value gives the (h+1)-th smallest float exactly.
//
// Every float operation of the definition is written out and rounded separately (contraction is off), so numpy reproduces the bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "jsg_internal.h"

namespace jsg {

typedef float hp_v2 __attribute__((ext_vector_type(2)));

constexpr int HP_TILE = 64;                  // bins per tile = frames per block of the frequency pass = lanes of a wavefront
constexpr unsigned HP_SENT = 0xFFFFFFFFu;    // the largest key: fills a window that is not full yet

struct HpArgs {
    const float* in;
    long long in_frame_pitch, in_row_pitch;     // elements of the input's kind
    float* out_h; float* out_p;
    long long out_frame_pitch, out_row_pitch;
    float* mask_h; float* mask_p;
    long long mask_frame_pitch, mask_row_pitch;
    float* cplane;                              // scratch [row][frame][bin]: the frequency medians
    long long T, n_items, chunks, fblocks;
    float g_h, g_p;
    int K, tiles, chunk, wt, wf;
};

// float bits -> a key whose unsigned order is the order of the floats (negative below positive, NaNs at the two ends), and back
__device__ inline unsigned hp_key(float v) {
    const unsigned b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ inline float hp_unkey(unsigned k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }

// scipy's "reflect" at any distance: (d c b a | a b c d | d c b a).  Mirroring at -1/2 and at L - 1/2 in turn ends at the index the
// definition's i mod 2L gives; no division, and at most a few rounds unless the axis is shorter than the half window.
__device__ inline long long hp_refl(long long i, long long L) {
    while (i < 0 || i >= L) i = i < 0 ? -1 - i : 2 * L - 1 - i;
    return i;
}

template <bool CPLX>
__device__ inline float hp_power(const float* p, long long idx) {
#pragma clang fp contract(off)
    if (CPLX) {
        const hp_v2 x = reinterpret_cast<const hp_v2*>(p)[idx];
        const float a = x.x * x.x, b = x.y * x.y;
        return a + b;
    }
    return p[idx];
}

// A lane's sorted window.  WC = 0: any odd length W at run time, in LDS as win[i * 64] (lane-major).  One step: `old` (present in the
// window) leaves, `nw` enters, 2 W reads and 2 W writes.
template <int WC>
struct HpWindow {
    unsigned* win;
    int W;
    __device__ inline HpWindow(unsigned* lds, int w) : win(lds), W(w) {
        for (int i = 0; i < W; ++i) win[i * HP_TILE] = HP_SENT;
    }
    __device__ inline void slide(unsigned old, unsigned nw) {
        unsigned carry = win[0];
        bool found = carry == old;
        carry = found ? nw : carry;
        for (int i = 1; i < W; ++i) {
            unsigned x = win[i * HP_TILE];
            const bool hit = !found && x == old;
            x = hit ? nw : x;
            found = found || hit;
            win[(i - 1) * HP_TILE] = min(carry, x);
            carry = max(carry, x);
        }
        for (int i = W - 2; i >= 0; --i) {
            const unsigned x = win[i * HP_TILE];
            win[(i + 1) * HP_TILE] = max(carry, x);
            carry = min(carry, x);
        }
        win[0] = carry;
    }
    __device__ inline unsigned median() const { return win[(W >> 1) * HP_TILE]; }
};

// The instantiation for a length known at compile time (the default 31): the window stays in registers, every index is a constant
// after unrolling, and a step is about 6 W vector operations with no LDS traffic.
template <>
struct HpWindow<31> {
    static constexpr int WN = 31;
    unsigned w[WN];
    __device__ inline HpWindow(unsigned*, int) {
#pragma unroll
        for (int i = 0; i < WN; ++i) w[i] = HP_SENT;
    }
    __device__ inline void slide(unsigned old, unsigned nw) {
        // the first element equal to `old`: its lower neighbour differs (the array is sorted); from the top, so neighbours are still the old ones
#pragma unroll
        for (int i = WN - 1; i > 0; --i) w[i] = (w[i] == old && w[i - 1] != old) ? nw : w[i];
        w[0] = w[0] == old ? nw : w[0];
#pragma unroll
        for (int i = 0; i + 1 < WN; ++i) {
            const unsigned lo = min(w[i], w[i + 1]), hi = max(w[i], w[i + 1]);
            w[i] = lo;
            w[i + 1] = hi;
        }
#pragma unroll
        for (int i = WN - 2; i >= 0; --i) {
            const unsigned lo = min(w[i], w[i + 1]), hi = max(w[i], w[i + 1]);
            w[i] = lo;
            w[i + 1] = hi;
        }
    }
    __device__ inline unsigned median() const { return w[WN >> 1]; }
};

template <int WC, bool CPLX>
__global__ __launch_bounds__(HP_TILE) void hpss_freq_kernel(const HpArgs a) {
#pragma clang fp contract(off)
    extern __shared__ unsigned hp_lds[];
    const int lane = threadIdx.x;
    const int W = WC ? WC : a.wf, h = W >> 1;
    const int pitch = HP_TILE + 1 + 2 * h;          // odd
    unsigned* tile = hp_lds;
    unsigned* mine = tile + lane * pitch;
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int tl = (int)(item % a.tiles);
        const long long rb = item / a.tiles;
        const long long fb = rb % a.fblocks, row = rb / a.fblocks;
        const int k0 = tl * HP_TILE;
        const int n_out = min(HP_TILE, a.K - k0);
        const int cols = n_out + 2 * h;             // <= 126: two columns per lane
        const long long f0 = fb * HP_TILE;
        const int n_fr = (int)min((long long)HP_TILE, a.T - f0);
        const float* src = a.in + (CPLX ? 2 : 1) * row * a.in_row_pitch;
        const int c0 = lane, c1 = lane + HP_TILE;
        const long long b0 = hp_refl((long long)k0 - h + c0, a.K), b1 = hp_refl((long long)k0 - h + c1, a.K);
        const bool l0 = c0 < cols, l1 = c1 < cols;
#pragma unroll 4
        for (int f = 0; f < HP_TILE; ++f) {
            float p0 = 0.f, p1 = 0.f;
            if (f < n_fr) {
                const long long base = (f0 + f) * a.in_frame_pitch;
                if (l0) p0 = hp_power<CPLX>(src, base + b0);
                if (l1) p1 = hp_power<CPLX>(src, base + b1);
            }
            if (l0) tile[f * pitch + 1 + c0] = hp_key(p0);
            if (l1) tile[f * pitch + 1 + c1] = hp_key(p1);
        }
        HpWindow<WC> win(hp_lds + HP_TILE * pitch + lane, W);
        __syncthreads();
        // lane = frame f0 + lane; column 1 + t holds bin k0 - h + t
        for (int t = 0; t < cols; ++t) {
            const unsigned nw = mine[1 + t];
            const unsigned old = t >= W ? mine[1 + t - W] : HP_SENT;
            win.slide(old, nw);
            if (t >= W - 1) mine[t - W + 1] = win.median();     // the column that has just left (or the spare one in front)
        }
        __syncthreads();
        float* dst = a.cplane + (row * a.T + f0) * a.K + k0 + lane;
        if (lane < n_out)
            for (int f = 0; f < n_fr; ++f) dst[(long long)f * a.K] = hp_unkey(tile[f * pitch + lane]);
        __syncthreads();
    }
}

struct HpCentre {     // of the output frame: the input element and its frequency median
    float re, im, c;
};

template <int WC, bool CPLX>
__global__ __launch_bounds__(HP_TILE) void hpss_time_kernel(const HpArgs a) {
#pragma clang fp contract(off)
    extern __shared__ unsigned hp_lds[];
    const int lane = threadIdx.x;
    const int W = WC ? WC : a.wt, h = W >> 1;
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int tl = (int)(item % a.tiles);
        const long long rc = item / a.tiles;
        const long long c = rc % a.chunks, row = rc / a.chunks;
        const int k = tl * HP_TILE + lane;
        const bool live = k < a.K;
        const long long j0 = c * a.chunk, j1 = min(a.T, j0 + a.chunk);
        const float* src = a.in + (CPLX ? 2 : 1) * row * a.in_row_pitch;
        const float* cpl = a.cplane + row * a.T * a.K + k;
        HpWindow<WC> win(hp_lds + lane, W);
        const long long t0 = j0 - h, t1 = j1 + h;
        // the values of the first step
        float p_new = live ? hp_power<CPLX>(src, hp_refl(t0, a.T) * a.in_frame_pitch + k) : 0.f;
        float p_old = 0.f;
        HpCentre ce{0.f, 0.f, 0.f};
        for (long long t = t0; t < t1; ++t) {
            // requested before the window work of this step: what step t + 1 inserts and deletes, and the centre of this step
            const long long tn = t + 1;
            const bool del_next = tn - W >= t0;
            float n_new = 0.f, n_old = 0.f;
            if (live && tn < t1) {
                n_new = hp_power<CPLX>(src, hp_refl(tn, a.T) * a.in_frame_pitch + k);
                if (del_next) n_old = hp_power<CPLX>(src, hp_refl(tn - W, a.T) * a.in_frame_pitch + k);
            }
            const long long j = t - h;
            if (live && j >= j0) {
                if (CPLX) {
                    const hp_v2 x = reinterpret_cast<const hp_v2*>(src)[j * a.in_frame_pitch + k];
                    ce.re = x.x;
                    ce.im = x.y;
                } else {
                    ce.re = src[j * a.in_frame_pitch + k];
                }
                ce.c = cpl[j * a.K];
            }
            win.slide(t - W >= t0 ? hp_key(p_old) : HP_SENT, hp_key(p_new));
            if (live && j >= j0) {
                const float Hm = hp_unkey(win.median()), Cm = ce.c;
                const float gc = a.g_h * Cm, gh = a.g_p * Hm;
                const float dh = Hm + gc, dp = Cm + gh;
                const float mh = dh > 0.f ? __fdiv_rn(Hm, dh) : 0.f;
                const float mp = dp > 0.f ? __fdiv_rn(Cm, dp) : 0.f;
                if (a.mask_h) a.mask_h[row * a.mask_row_pitch + j * a.mask_frame_pitch + k] = mh;
                if (a.mask_p) a.mask_p[row * a.mask_row_pitch + j * a.mask_frame_pitch + k] = mp;
                const long long o = row * a.out_row_pitch + j * a.out_frame_pitch + k;
                if (CPLX) {
                    if (a.out_h) __builtin_nontemporal_store(hp_v2{mh * ce.re, mh * ce.im}, reinterpret_cast<hp_v2*>(a.out_h) + o);
                    if (a.out_p) __builtin_nontemporal_store(hp_v2{mp * ce.re, mp * ce.im}, reinterpret_cast<hp_v2*>(a.out_p) + o);
                } else {
                    if (a.out_h) a.out_h[o] = mh * ce.re;
                    if (a.out_p) a.out_p[o] = mp * ce.re;
                }
            }
            p_new = n_new;
            p_old = n_old;
        }
    }
}

}  // namespace jsg

using namespace jsg;

namespace {

struct HpCall {
    long long tiles, chunk, chunks, fblocks;
    long long scratch_bytes;
};

// the default chunk of the time pass: about 4096 work items, 32..1024 frames (a chunk re-reads the W_t - 1 frames around it).  It
// depends on the sizes of the call only, so the scratch size can be asked for without a device.
long long default_chunk(long long T, long long rows, long long tiles) {
    const i128 want = ((i128)T * rows * tiles + 4095) / 4096;
    return (long long)std::max<i128>(32, std::min<i128>(1024, want));
}

struct Span {
    i128 lo, bytes;
    const char* name;
};

int hpss_check(const jsg_hpss_args* g, const char* who, HpCall* c) {
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in) return jsg_fail_who(JSG_ERR_INVALID, who, "null input pointer");
    if (g->in_complex != 0 && g->in_complex != 1) return jsg_fail_who(JSG_ERR_INVALID, who, "in_complex must be 0 or 1");
    if (!g->out_h && !g->out_p && !g->mask_h && !g->mask_p) return jsg_fail_who(JSG_ERR_INVALID, who, "all four outputs are null");
    if (g->win_time < 1 || g->win_time > JSG_HPSS_MAX_WINDOW || !(g->win_time & 1))
        return jsg_fail_who(JSG_ERR_INVALID, who, "win_time must be odd and in 1..63");
    if (g->win_freq < 1 || g->win_freq > JSG_HPSS_MAX_WINDOW || !(g->win_freq & 1))
        return jsg_fail_who(JSG_ERR_INVALID, who, "win_freq must be odd and in 1..63");
    if (const int rc = check_rows(g->rows, who); rc != JSG_OK) return rc;
    if (g->n_bins < 1 || g->n_bins > 32769) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bins must be in 1..32769");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    if (g->chunk_frames < 0 || g->chunk_frames > 65536) return jsg_fail_who(JSG_ERR_INVALID, who, "chunk_frames must be 0 or in 1..65536");
    if (!std::isfinite(g->margin_h) || g->margin_h < 1.0f) return jsg_fail_who(JSG_ERR_INVALID, who, "margin_h must be finite and >= 1");
    if (!std::isfinite(g->margin_p) || g->margin_p < 1.0f) return jsg_fail_who(JSG_ERR_INVALID, who, "margin_p must be finite and >= 1");
    const long long K = g->n_bins, T = g->n_frames;
    const bool any_out = g->out_h || g->out_p, any_mask = g->mask_h || g->mask_p;
    if (g->in_frame_pitch < K) return jsg_fail_who(JSG_ERR_INVALID, who, "in_frame_pitch smaller than n_bins");
    if (any_out && g->out_frame_pitch < K) return jsg_fail_who(JSG_ERR_INVALID, who, "out_frame_pitch smaller than n_bins");
    if (any_mask && g->mask_frame_pitch < K) return jsg_fail_who(JSG_ERR_INVALID, who, "mask_frame_pitch smaller than n_bins");
    const i128 in_row = plane(T, g->in_frame_pitch, K), out_row = plane(T, g->out_frame_pitch, K), mask_row = plane(T, g->mask_frame_pitch, K);
    if (g->rows > 1 && g->in_row_pitch < in_row) return jsg_fail_who(JSG_ERR_INVALID, who, "in_row_pitch smaller than one row of frames");
    if (g->rows > 1 && any_out && g->out_row_pitch < out_row) return jsg_fail_who(JSG_ERR_INVALID, who, "out_row_pitch smaller than one row of frames");
    if (g->rows > 1 && any_mask && g->mask_row_pitch < mask_row) return jsg_fail_who(JSG_ERR_INVALID, who, "mask_row_pitch smaller than one row of frames");
    const int esz = g->in_complex ? 8 : 4;
    const uintptr_t amask = g->in_complex ? 7 : 3;
    if ((reinterpret_cast<uintptr_t>(g->in) & amask) || (reinterpret_cast<uintptr_t>(g->out_h) & amask) || (reinterpret_cast<uintptr_t>(g->out_p) & amask))
        return jsg_fail_who(JSG_ERR_INVALID, who, g->in_complex ? "in, out_h and out_p must be 8-byte aligned (complex float pairs)"
                                                                : "in, out_h and out_p must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(g->mask_h) & 3) || (reinterpret_cast<uintptr_t>(g->mask_p) & 3))
        return jsg_fail_who(JSG_ERR_INVALID, who, "mask_h and mask_p must be 4-byte aligned");
    // the bytes every buffer spans, first to last element; the input first
    Span s[5];
    int n = 0;
    auto add = [&](const void* p, int bytes, long long row_pitch, i128 row, const char* name) {
        if (p) s[n++] = Span{addr(p), span_bytes(g->rows, row_pitch, row, bytes), name};
    };
    add(g->in, esz, g->in_row_pitch, in_row, "in");
    add(g->out_h, esz, g->out_row_pitch, out_row, "out_h");
    add(g->out_p, esz, g->out_row_pitch, out_row, "out_p");
    add(g->mask_h, 4, g->mask_row_pitch, mask_row, "mask_h");
    add(g->mask_p, 4, g->mask_row_pitch, mask_row, "mask_p");
    for (int i = 1; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (overlap(s[i].lo, s[i].bytes, s[j].lo, s[j].bytes))
                return jsg_fail_who(JSG_ERR_INVALID, who, (std::string(s[i].name) + " overlaps " + s[j].name).c_str());
    c->tiles = (K + HP_TILE - 1) / HP_TILE;
    c->chunk = g->chunk_frames ? g->chunk_frames : default_chunk(T, g->rows, c->tiles);
    c->chunks = (T + c->chunk - 1) / c->chunk;
    c->fblocks = (T + HP_TILE - 1) / HP_TILE;
    const i128 bytes = ((i128)g->rows * T * K * 4 + 15) / 16 * 16;      // the plane of frequency medians
    if (bytes >= ((i128)1 << 62)) return jsg_fail_who(JSG_ERR_INVALID, who, "the scratch of this call would exceed 2^62 bytes");
    c->scratch_bytes = (long long)bytes;
    return JSG_OK;
}

template <bool CPLX>
hipError_t hpss_enqueue(HpArgs& k, const HpCall& c, int rows, long long max_grid, hipStream_t s) {
    // the tile of the frequency pass, and a window [W][64] per kernel unless its length is the compiled-in 31 (registers)
    const size_t lds_f = sizeof(unsigned) * (size_t)(HP_TILE * (HP_TILE + 1 + 2 * (k.wf >> 1)) + (k.wf == 31 ? 0 : HP_TILE * k.wf));
    const size_t lds_t = sizeof(unsigned) * (size_t)(k.wt == 31 ? 0 : HP_TILE * k.wt);
    k.n_items = (long long)rows * c.fblocks * c.tiles;
    dim3 grid((unsigned)std::min(k.n_items, max_grid));
    if (k.wf == 31)
        hipLaunchKernelGGL((hpss_freq_kernel<31, CPLX>), grid, dim3(HP_TILE), lds_f, s, k);
    else
        hipLaunchKernelGGL((hpss_freq_kernel<0, CPLX>), grid, dim3(HP_TILE), lds_f, s, k);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    k.n_items = (long long)rows * c.chunks * c.tiles;
    grid = dim3((unsigned)std::min(k.n_items, max_grid));
    if (k.wt == 31)
        hipLaunchKernelGGL((hpss_time_kernel<31, CPLX>), grid, dim3(HP_TILE), lds_t, s, k);
    else
        hipLaunchKernelGGL((hpss_time_kernel<0, CPLX>), grid, dim3(HP_TILE), lds_t, s, k);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int64_t jsg_hpss_scratch_bytes(const jsg_hpss_args* g) {
    HpCall c{};
    const int rc = hpss_check(g, "jsg_hpss_scratch_bytes", &c);
    return rc != JSG_OK ? rc : c.scratch_bytes;
}

int jsg_hpss_launch(const jsg_hpss_args* g, void* scratch, int64_t scratch_bytes, void* stream) {
    static const char* who = "jsg_hpss_launch";
    HpCall c{};
    int rc = hpss_check(g, who, &c);
    if (rc != JSG_OK) return rc;
    if (!scratch) return jsg_fail_who(JSG_ERR_INVALID, who, "null scratch");
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) != 0) return jsg_fail_who(JSG_ERR_INVALID, who, "scratch must be 16-byte aligned");
    if (scratch_bytes < c.scratch_bytes) return jsg_fail_who(JSG_ERR_INVALID, who, "scratch smaller than jsg_hpss_scratch_bytes");
    int dev = -1;
    rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    // every refusal is behind us
    HpArgs k{};
    const bool multi = g->rows > 1;
    k.in = g->in;
    k.in_frame_pitch = g->in_frame_pitch;
    k.in_row_pitch = multi ? g->in_row_pitch : 0;
    k.out_h = g->out_h;
    k.out_p = g->out_p;
    k.out_frame_pitch = g->out_frame_pitch;
    k.out_row_pitch = multi ? g->out_row_pitch : 0;
    k.mask_h = g->mask_h;
    k.mask_p = g->mask_p;
    k.mask_frame_pitch = g->mask_frame_pitch;
    k.mask_row_pitch = multi ? g->mask_row_pitch : 0;
    k.cplane = static_cast<float*>(scratch);
    k.T = g->n_frames;
    k.chunks = c.chunks;
    k.fblocks = c.fblocks;
    {
#pragma clang fp contract(off)
        k.g_h = g->margin_h * g->margin_h;
        k.g_p = g->margin_p * g->margin_p;
    }
    k.K = g->n_bins;
    k.tiles = (int)c.tiles;
    k.chunk = (int)c.chunk;
    k.wt = g->win_time;
    k.wf = g->win_freq;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // tests/test_gpu_hpss_edges.py reads the grid limit from the next line
    const long long max_grid = (long long)cu_count_of_device(dev) * 32;   // as many wavefronts as a compute unit holds
    const hipError_t err = g->in_complex ? hpss_enqueue<true>(k, c, g->rows, max_grid, s) : hpss_enqueue<false>(k, c, g->rows, max_grid, s);
    if (err != hipSuccess) return jsg_fail_hip(err, who);
    return JSG_OK;
}

}  // extern "C"
