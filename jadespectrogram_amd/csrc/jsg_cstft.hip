// libjsg.so, complex STFT and inverse STFT with any hop (include/jsg.h, section 2d).  A unit of its own: the dB kernels of
// jsg_stft_kernel.h are not touched and nothing of theirs is instantiated here.
//
//   cstft_fwd_kernel<N>   frames -> complex bins.  A workgroup (4 waves) takes a tile of max(N, 1024) complex points: one frame of
//                 n = 2N samples at 4096 / 8192 points, 2 or 4 frames below.  Per tile:
//                   load    lanes along the samples (coalesced, any hop, so no wider alignment), times the window, into LDS as the
//                           N-point complex sequence z[m] = x[2m] + i x[2m+1] (the float order of the frame is that sequence);
//                   FFT     radix-4 Stockham passes through LDS (one radix-2 pass last where log2 N is odd), every thread a fixed
//                           number of butterflies per pass, twiddles from an LDS copy of the plan's table;
//                   split   X_k = E_k + W_n^k O_k for k = 0..N, one lane per bin, 8-byte non-temporal stores (the bins of a frame
//                           are contiguous in the caller's frame-major buffer).
//                 The grid is at most a few workgroups per CU that walk the tiles; each loads the twiddle table once.
//   istft_c2r_kernel<N>   complex bins -> windowed frames in caller scratch: the mirror image (pre-pass Z_k from X_k and
//                 conj(X_(N-k)), inverse Stockham passes, times 1/n and the window), 16-byte stores.
//   istft_ola_kernel      windowed frames -> samples: one lane per output sample sums its covering frames in ascending order
//                 (no atomics: every sample is the same sum whatever the chunking) and multiplies by the reciprocal envelope
//                 1 / sum w^2, summed in double from the plan's w^2 table and rounded to float32 once; 0 where the envelope is at
//                 most 1e-11.
// Twiddles W_n^m (m < n/2) and w^2 are computed on the host in double and rounded once; they are uploaded with the plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "jsg_internal.h"

namespace jsg {

typedef float cs_v2 __attribute__((ext_vector_type(2)));
typedef float cs_v4 __attribute__((ext_vector_type(4)));

constexpr int CS_THREADS = 256;
constexpr int CS_LDS_PER_CU = 160 * 1024;

template <int N>
struct CsGeom {
    static constexpr int n = 2 * N;                  // real samples per frame
    static constexpr int T = N < 1024 ? 1024 : N;    // complex points per tile
    static constexpr int FPB = T / N;                // frames per tile
    static constexpr int LDS = T * 8 + N * 8 + FPB * 8;
};

struct CsFwdArgs {
    const float* in;
    long long in_pitch;
    const float* win;           // n floats
    const cs_v2* tw;            // W_n^m, m < n/2
    cs_v2* out;
    long long out_frame_pitch, out_row_pitch;   // complex elements
    int hop;
    int tiles_per_row;
    long long n_tiles;
    long long n_frames;
};

struct CsInvArgs {
    const cs_v2* in;
    long long in_frame_pitch, in_row_pitch;     // complex elements
    const float* win;
    const cs_v2* tw;
    float* scratch;             // frame (row, f) at scratch[(row * frames_per_row + f) * n]
    long long frames_per_row;   // scratch row stride in frames
    long long first_frame;      // frame index of scratch frame 0
    long long n_frames;         // frames of this chunk
    int tiles_per_row;
    long long n_tiles;
};

struct CsOlaArgs {
    const float* scratch;
    long long frames_per_row, first_frame;
    const double* w2;           // n doubles: w[m]^2
    float* out;
    long long out_pitch;
    long long t0, t1;           // output samples of this chunk
    long long n_frames;         // frames of the whole call
    int n, hop;
};

__device__ inline cs_v2 cs_mul(cs_v2 a, cs_v2 b) { return cs_v2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// W_n^m (INV: its conjugate) for 0 <= m < n from the half table tw[m] = W_n^m, m < N = n/2 (W_n^(m+N) = -W_n^m)
template <int N, bool INV>
__device__ inline cs_v2 cs_twiddle(const cs_v2* tw, int m) {
    cs_v2 w = m < N ? tw[m] : -tw[m - N];
    if (INV) w.y = -w.y;
    return w;
}

// One radix-R Stockham pass over the FPB frames of a tile (NS = length of the sub-transforms done so far): butterfly j of a frame
// reads z[j + r N/R], applies W_(R NS)^(r k) (k = j mod NS), and writes its R outputs to (j / NS) NS R + k + r NS.  All reads are in
// registers before the first write, so one buffer serves.
template <int N, int R, int NS, bool INV>
__device__ inline void cs_pass(cs_v2* buf, const cs_v2* tw, int tid) {
    constexpr int Q = N / R;                                   // butterflies per frame
    constexpr int BPT = CsGeom<N>::T / R / CS_THREADS;         // butterflies per thread
    constexpr int STEP = 2 * N / (R * NS);                     // W_(R NS) = W_n^STEP
    cs_v2 y[BPT][R];
    int dst[BPT];
#pragma unroll
    for (int b = 0; b < BPT; ++b) {
        const int g = tid + b * CS_THREADS;
        const int f = g / Q, j = g % Q, k = j % NS;
        cs_v2 a[R];
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] = buf[f * N + j + r * Q];
        if constexpr (NS > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) a[r] = cs_mul(a[r], cs_twiddle<N, INV>(tw, r * k * STEP));
        }
        if constexpr (R == 2) {
            y[b][0] = a[0] + a[1];
            y[b][1] = a[0] - a[1];
        } else {
            const cs_v2 t0 = a[0] + a[2], t1 = a[0] - a[2], t2 = a[1] + a[3], d = a[1] - a[3];
            const cs_v2 t3 = INV ? cs_v2{-d.y, d.x} : cs_v2{d.y, -d.x};   // (a1 - a3) times +i / -i
            y[b][0] = t0 + t2;
            y[b][1] = t1 + t3;
            y[b][2] = t0 - t2;
            y[b][3] = t1 - t3;
        }
        dst[b] = f * N + (j / NS) * NS * R + k;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < BPT; ++b)
#pragma unroll
        for (int r = 0; r < R; ++r) buf[dst[b] + r * NS] = y[b][r];
    __syncthreads();
}

template <int N, int NS, bool INV>
__device__ inline void cs_fft(cs_v2* buf, const cs_v2* tw, int tid) {
    if constexpr (NS * 4 <= N) {
        cs_pass<N, 4, NS, INV>(buf, tw, tid);
        cs_fft<N, NS * 4, INV>(buf, tw, tid);
    } else if constexpr (NS * 2 == N) {
        cs_pass<N, 2, NS, INV>(buf, tw, tid);
    }
}

template <int N>
__global__ __launch_bounds__(CS_THREADS) void cstft_fwd_kernel(const CsFwdArgs a) {
    using G = CsGeom<N>;
    constexpr int n = G::n, FPB = G::FPB;
    __shared__ cs_v2 s_buf[G::T];
    __shared__ cs_v2 s_tw[N];
    const int tid = threadIdx.x;
    for (int m = tid; m < N; m += CS_THREADS) s_tw[m] = a.tw[m];
    float* sf = reinterpret_cast<float*>(s_buf);
    for (long long tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long row = tile / a.tiles_per_row;
        const long long j0 = (tile - row * a.tiles_per_row) * FPB;
        const float* src = a.in + row * a.in_pitch + j0 * a.hop;
        float v[FPB * n / CS_THREADS];
#pragma unroll
        for (int i = 0; i < FPB * n / CS_THREADS; ++i) {
            const int e = tid + i * CS_THREADS, f = e / n, m = e % n;
            v[i] = (j0 + f < a.n_frames) ? src[(long long)f * a.hop + m] * a.win[m] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < FPB * n / CS_THREADS; ++i) sf[tid + i * CS_THREADS] = v[i];
        __syncthreads();
        cs_fft<N, 1, false>(s_buf, s_tw, tid);
        // real split: Z = FFT(z), E_k = (Z_k + conj Z_(N-k)) / 2, O_k = (Z_k - conj Z_(N-k)) / 2i, X_k = E_k + W_n^k O_k, k = 0..N
        for (int e = tid; e < FPB * (N + 1); e += CS_THREADS) {
            const int f = e / (N + 1), k = e - f * (N + 1);
            if (j0 + f >= a.n_frames) break;
            const cs_v2 zk = s_buf[f * N + (k & (N - 1))], zm = s_buf[f * N + ((N - k) & (N - 1))];
            const cs_v2 E = cs_v2{zk.x + zm.x, zk.y - zm.y} * 0.5f;
            const cs_v2 O = cs_v2{zk.y + zm.y, zm.x - zk.x} * 0.5f;
            const cs_v2 X = E + cs_mul(cs_twiddle<N, false>(s_tw, k), O);
            __builtin_nontemporal_store(X, a.out + row * a.out_row_pitch + (j0 + f) * a.out_frame_pitch + k);
        }
        __syncthreads();
    }
}

template <int N>
__global__ __launch_bounds__(CS_THREADS) void istft_c2r_kernel(const CsInvArgs a) {
    using G = CsGeom<N>;
    constexpr int n = G::n, FPB = G::FPB;
    __shared__ cs_v2 s_buf[G::T];
    __shared__ cs_v2 s_tw[N];
    __shared__ cs_v2 s_nyq[FPB];
    const int tid = threadIdx.x;
    for (int m = tid; m < N; m += CS_THREADS) s_tw[m] = a.tw[m];
    for (long long tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const long long row = tile / a.tiles_per_row;
        const long long j0 = (tile - row * a.tiles_per_row) * FPB;             // frame of the chunk
        const cs_v2* src = a.in + row * a.in_row_pitch + (a.first_frame + j0) * a.in_frame_pitch;
        for (int e = tid; e < FPB * (N + 1); e += CS_THREADS) {
            const int f = e / (N + 1), k = e - f * (N + 1);
            const cs_v2 x = (j0 + f < a.n_frames) ? src[(long long)f * a.in_frame_pitch + k] : cs_v2{0.f, 0.f};
            if (k < N) s_buf[f * N + k] = x;
            else s_nyq[f] = x;
        }
        __syncthreads();
        // pre-pass, pairs (k, N-k), k = 0..N/2, in place: Z_k = (X_k + conj X_(N-k)) + i (X_k - conj X_(N-k)) conj(W_n^k); the
        // imaginary parts of X_0 and X_N are not read (irfft's convention)
        for (int e = tid; e < FPB * (N / 2 + 1); e += CS_THREADS) {
            const int f = e / (N / 2 + 1), k = e - f * (N / 2 + 1);
            cs_v2 p = s_buf[f * N + k], q = k == 0 ? s_nyq[f] : s_buf[f * N + N - k];
            if (k == 0) {
                p.y = 0.f;
                q.y = 0.f;
            }
            const cs_v2 s0 = cs_v2{p.x + q.x, p.y - q.y}, d0 = cs_mul(cs_v2{p.x - q.x, p.y + q.y}, cs_twiddle<N, true>(s_tw, k));
            s_buf[f * N + k] = cs_v2{s0.x - d0.y, s0.y + d0.x};
            if (k != 0 && k != N / 2) {
                const cs_v2 s1 = cs_v2{q.x + p.x, q.y - p.y}, d1 = cs_mul(cs_v2{q.x - p.x, q.y + p.y}, cs_twiddle<N, true>(s_tw, N - k));
                s_buf[f * N + N - k] = cs_v2{s1.x - d1.y, s1.y + d1.x};
            }
        }
        __syncthreads();
        cs_fft<N, 1, true>(s_buf, s_tw, tid);
        // the frame, times 1/n (exact) and the window, into scratch: 16-byte stores
        const cs_v4* s4 = reinterpret_cast<const cs_v4*>(s_buf);
        const cs_v4* w4 = reinterpret_cast<const cs_v4*>(a.win);
        cs_v4* dst = reinterpret_cast<cs_v4*>(a.scratch + (row * a.frames_per_row + j0) * n);
        for (int e = tid; e < FPB * n / 4; e += CS_THREADS) {
            const int f = e / (n / 4), m4 = e - f * (n / 4);
            if (j0 + f >= a.n_frames) break;
            dst[e] = (s4[e] * (1.0f / n)) * w4[m4];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(CS_THREADS) void istft_ola_kernel(const CsOlaArgs a) {
#pragma clang fp contract(off)
    const long long t = a.t0 + (long long)blockIdx.x * CS_THREADS + threadIdx.x;
    if (t >= a.t1) return;
    const long long row = blockIdx.y;
    const long long lo = t - a.n + 1;
    const long long jlo = lo <= 0 ? 0 : (lo + a.hop - 1) / a.hop;
    const long long jhi = min(a.n_frames - 1, t / a.hop);
    float acc = 0.f;
    double env = 0.0;
    for (long long j = jlo; j <= jhi; ++j) {
        const long long m = t - j * a.hop;
        acc += a.scratch[(row * a.frames_per_row + j - a.first_frame) * a.n + m];
        env += a.w2[m];
    }
    a.out[row * a.out_pitch + t] = env > 1e-11 ? acc * (float)(1.0 / env) : 0.f;
}

template <int N>
int cs_blocks_per_cu() {
    return std::max(1, std::min(8, CS_LDS_PER_CU / CsGeom<N>::LDS));
}

}  // namespace jsg

using namespace jsg;

// A complex STFT plan on the device that was current at creation: window (n floats), twiddles W_n^m (m < n/2, float pairs) and w^2
// (n doubles), one allocation; the window is kept on the host for the NOLA check.
struct jsg_cstft {
    int n = 0;
    DeviceBlob blob;
    const float* d_win = nullptr;
    const cs_v2* d_tw = nullptr;
    const double* d_w2 = nullptr;
    std::vector<float> win;
};

namespace {

constexpr double kNolaEps = 1e-11;

// smallest sum_j w[rho + j hop]^2 over rho < hop, in double (the interior envelope of a long call is periodic with period hop)
double nola_min(int n, int hop, const float* w) {
#pragma clang fp contract(off)
    double mn = INFINITY;
    for (int rho = 0; rho < hop; ++rho) {
        double s = 0.0;
        for (int m = rho; m < n; m += hop) s += double(w[m]) * double(w[m]);
        mn = std::min(mn, s);
    }
    return mn;
}

int cs_check_device(const jsg_cstft* p, const char* who) {
    const DeviceBlob::Where at = p->blob.where();
    if (at == DeviceBlob::kNoDevice) return jsg_fail_who(JSG_ERR_NO_DEVICE, who, "no HIP device");
    if (at != DeviceBlob::kHere) return jsg_fail_who(JSG_ERR_INVALID, who, "the plan was created on another device");
    return JSG_OK;
}

template <int N>
hipError_t fwd_launch(const CsFwdArgs& ka, int rows, long long n_frames, int dev, hipStream_t s) {
    CsFwdArgs k = ka;
    k.tiles_per_row = (int)((n_frames + CsGeom<N>::FPB - 1) / CsGeom<N>::FPB);
    k.n_tiles = (long long)k.tiles_per_row * rows;
    hipLaunchKernelGGL(cstft_fwd_kernel<N>, dim3(resident_grid(k.n_tiles, dev, cs_blocks_per_cu<N>())), dim3(CS_THREADS), 0, s, k);      // n_tiles >= 1
    return hipGetLastError();
}

template <int N>
hipError_t c2r_launch(const CsInvArgs& ka, int rows, int dev, hipStream_t s) {
    CsInvArgs k = ka;
    k.tiles_per_row = (int)((k.n_frames + CsGeom<N>::FPB - 1) / CsGeom<N>::FPB);
    k.n_tiles = (long long)k.tiles_per_row * rows;
    hipLaunchKernelGGL(istft_c2r_kernel<N>, dim3(resident_grid(k.n_tiles, dev, cs_blocks_per_cu<N>())), dim3(CS_THREADS), 0, s, k);      // n_tiles >= 1
    return hipGetLastError();
}

hipError_t c2r_dispatch(int n, const CsInvArgs& k, int rows, int dev, hipStream_t s) {
    switch (n) {
        case 512: return c2r_launch<256>(k, rows, dev, s);
        case 1024: return c2r_launch<512>(k, rows, dev, s);
        case 2048: return c2r_launch<1024>(k, rows, dev, s);
        case 4096: return c2r_launch<2048>(k, rows, dev, s);
        default: return c2r_launch<4096>(k, rows, dev, s);
    }
}

// The chunking of an inverse call: F frames that reach the output (the last one covers sample out_samples - 1), K = the frames
// before a chunk's first new frame that still overlap its first sample, per_row = scratch frames per row.
struct IstftPlanOfCall {
    long long F, K, per_row, new_per_chunk;
};

int istft_check(const jsg_cstft* p, const jsg_istft_args* g, const char* who, IstftPlanOfCall* c) {
    if (!p || !g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    const int n = p->n, N = n / 2;
    if (!g->in || !g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null data pointer");
    if (g->hop < 1 || g->hop > n) return jsg_fail_who(JSG_ERR_INVALID, who, "hop must be in 1..n");
    if (g->rows < 1 || g->rows > 65535) return jsg_fail_who(JSG_ERR_INVALID, who, "rows must be in 1..65535");
    if (g->n_frames < 1 || g->n_frames >= (1ll << 31))
        return jsg_fail_who(JSG_ERR_INVALID, who, "n_frames must be in 1..2^31-1");
    const long long span = (g->n_frames - 1) * (long long)g->hop + n;
    if (g->out_samples < 1 || g->out_samples > span)
        return jsg_fail_who(JSG_ERR_INVALID, who, "out_samples must be in 1..(n_frames-1)*hop+n");
    if (g->in_frame_pitch < N + 1) return jsg_fail_who(JSG_ERR_INVALID, who, "in_frame_pitch smaller than n/2+1");
    if (g->rows > 1 && g->in_row_pitch < (g->n_frames - 1) * g->in_frame_pitch + N + 1)
        return jsg_fail_who(JSG_ERR_INVALID, who, "in_row_pitch smaller than one row of frames");
    if (g->rows > 1 && g->out_pitch < g->out_samples)
        return jsg_fail_who(JSG_ERR_INVALID, who, "out_pitch smaller than out_samples");
    if ((reinterpret_cast<uintptr_t>(g->in) & 7) != 0)
        return jsg_fail_who(JSG_ERR_INVALID, who, "in must be 8-byte aligned (complex float pairs)");
    if (nola_min(n, g->hop, p->win.data()) <= kNolaEps)
        return jsg_fail_who(JSG_ERR_INVALID, who, "the window fails the NOLA condition at this hop (envelope <= 1e-11)");
    c->F = std::min(g->n_frames, (g->out_samples - 1) / g->hop + 1);
    c->K = (n - 1) / g->hop;
    return JSG_OK;
}

}  // namespace

extern "C" {

int jsg_cstft_create(jsg_cstft** out, int n, const float* window) {
    if (!out || !window) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_create: null argument");
    *out = nullptr;
    if (!fft_size_supported(n)) return jsg_fail(JSG_ERR_UNSUPPORTED, "jsg_cstft_create: FFT size must be 512, 1024, 2048, 4096 or 8192");
    for (int m = 0; m < n; ++m)
        if (!std::isfinite(window[m])) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_create: the window must be finite");
    const int N = n / 2;
    // [window n floats][twiddles N float pairs][w^2 n doubles]: every part 8-byte aligned (n >= 512)
    std::vector<unsigned char> blob(size_t(n) * 4 + size_t(N) * 8 + size_t(n) * 8);
    float* w = reinterpret_cast<float*>(blob.data());
    float* tw = reinterpret_cast<float*>(blob.data() + size_t(n) * 4);
    double* w2 = reinterpret_cast<double*>(blob.data() + size_t(n) * 4 + size_t(N) * 8);
    const double pi = 3.14159265358979323846264338327950288;
    for (int m = 0; m < n; ++m) {
        w[m] = window[m];
        w2[m] = double(window[m]) * double(window[m]);   // exact in double
    }
    for (int m = 0; m < N; ++m) {
        const double ang = -2.0 * pi * double(m) / double(n);
        tw[2 * m] = float(std::cos(ang));
        tw[2 * m + 1] = float(std::sin(ang));
    }
    static const char* who = "jsg_cstft_create";
    std::unique_ptr<jsg_cstft> p(new (std::nothrow) jsg_cstft());
    if (!p) return jsg_fail_who(JSG_ERR_NOMEM, who, "out of host memory");
    p->n = n;
    const int rc = p->blob.upload(blob.data(), blob.size(), who);
    if (rc != JSG_OK) return rc;
    const unsigned char* d = static_cast<const unsigned char*>(p->blob.data());
    p->d_win = reinterpret_cast<const float*>(d);
    p->d_tw = reinterpret_cast<const cs_v2*>(d + size_t(n) * 4);
    p->d_w2 = reinterpret_cast<const double*>(d + size_t(n) * 4 + size_t(N) * 8);
    p->win.assign(window, window + n);
    (void)preload_code_object(reinterpret_cast<const void*>(&istft_ola_kernel));
    *out = p.release();
    return JSG_OK;
}

int jsg_cstft_destroy(jsg_cstft* plan) {
    delete plan;
    return JSG_OK;
}

int jsg_cstft_fft_size(const jsg_cstft* plan) { return plan ? plan->n : jsg_fail(JSG_ERR_INVALID, "jsg_cstft_fft_size: null"); }

int jsg_cstft_launch(const jsg_cstft* plan, const jsg_cstft_args* g, void* stream) {
    if (!plan || !g) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: null argument");
    const int n = plan->n, N = n / 2;
    if (!g->in || !g->out) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: null data pointer");
    if (g->hop < 1 || g->hop > n) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: hop must be in 1..n");
    if (g->rows < 1 || g->rows > 65535) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: rows must be in 1..65535");
    if (g->n_frames < 0 || g->n_frames >= (1ll << 31)) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: n_frames must be in 0..2^31-1");
    if (g->in_pitch < 0) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: negative in_pitch");
    if (g->out_frame_pitch < N + 1) return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: out_frame_pitch smaller than n/2+1");
    if (g->rows > 1 && g->n_frames > 0 && g->out_row_pitch < (g->n_frames - 1) * g->out_frame_pitch + N + 1)
        return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: out_row_pitch smaller than one row of frames");
    if (g->in_samples != 0 && g->n_frames > 0 &&
        (g->in_samples < 0 || (g->n_frames - 1) * g->hop + n > g->in_samples || (g->rows > 1 && g->in_pitch < g->in_samples)))
        return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: the last frame would read past the end of the input rows");
    if ((reinterpret_cast<uintptr_t>(g->out) & 7) != 0)
        return jsg_fail(JSG_ERR_INVALID, "jsg_cstft_launch: out must be 8-byte aligned (complex float pairs)");
    int rc = cs_check_device(plan, "jsg_cstft_launch");
    if (rc != JSG_OK) return rc;
    if (g->n_frames == 0) return JSG_OK;
    CsFwdArgs k{};
    k.in = g->in;
    k.in_pitch = g->in_pitch;
    k.win = plan->d_win;
    k.tw = plan->d_tw;
    k.out = reinterpret_cast<cs_v2*>(g->out);
    k.out_frame_pitch = g->out_frame_pitch;
    k.out_row_pitch = g->out_row_pitch;
    k.hop = g->hop;
    k.n_frames = g->n_frames;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t err;
    switch (n) {
        case 512: err = fwd_launch<256>(k, g->rows, g->n_frames, plan->blob.device(), s); break;
        case 1024: err = fwd_launch<512>(k, g->rows, g->n_frames, plan->blob.device(), s); break;
        case 2048: err = fwd_launch<1024>(k, g->rows, g->n_frames, plan->blob.device(), s); break;
        case 4096: err = fwd_launch<2048>(k, g->rows, g->n_frames, plan->blob.device(), s); break;
        default: err = fwd_launch<4096>(k, g->rows, g->n_frames, plan->blob.device(), s); break;
    }
    if (err != hipSuccess) return jsg_fail_hip(err, "jsg_cstft_launch");
    return JSG_OK;
}

int jsg_istft_nola(int n, int hop, const float* window, float* min_envelope) {
    if (!window || !min_envelope) return jsg_fail(JSG_ERR_INVALID, "jsg_istft_nola: null argument");
    if (!fft_size_supported(n)) return jsg_fail(JSG_ERR_UNSUPPORTED, "jsg_istft_nola: FFT size must be 512, 1024, 2048, 4096 or 8192");
    if (hop < 1 || hop > n) return jsg_fail(JSG_ERR_INVALID, "jsg_istft_nola: hop must be in 1..n");
    for (int m = 0; m < n; ++m)
        if (!std::isfinite(window[m])) return jsg_fail(JSG_ERR_INVALID, "jsg_istft_nola: the window must be finite");
    const double mn = nola_min(n, hop, window);
    *min_envelope = float(mn);
    if (mn <= kNolaEps) return jsg_fail(JSG_ERR_INVALID, "jsg_istft_nola: the interior envelope is <= 1e-11 (NOLA fails)");
    return JSG_OK;
}

int64_t jsg_istft_scratch_floats(const jsg_cstft* plan, const jsg_istft_args* g) {
    IstftPlanOfCall c{};
    int rc = istft_check(plan, g, "jsg_istft_scratch_floats", &c);
    if (rc != JSG_OK) return rc;
    const long long frame = (long long)g->rows * plan->n;
    const long long whole = c.F * frame, minimum = std::min(c.F, c.K + 1) * frame, cap = 16ll << 20;   // 64 MiB
    if (whole <= cap) return whole;
    return std::max(minimum, cap / frame * frame);
}

int jsg_istft_launch(const jsg_cstft* plan, const jsg_istft_args* g, float* scratch, int64_t scratch_floats, void* stream) {
    IstftPlanOfCall c{};
    int rc = istft_check(plan, g, "jsg_istft_launch", &c);
    if (rc != JSG_OK) return rc;
    if (!scratch) return jsg_fail(JSG_ERR_INVALID, "jsg_istft_launch: null scratch");
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) != 0) return jsg_fail(JSG_ERR_INVALID, "jsg_istft_launch: scratch must be 16-byte aligned");
    const int n = plan->n;
    const long long per_row = scratch_floats < 0 ? 0 : scratch_floats / ((long long)g->rows * n);
    if (per_row < std::min(c.F, c.K + 1))
        return jsg_fail(JSG_ERR_INVALID, "jsg_istft_launch: scratch smaller than rows * n * min(frames, floor((n-1)/hop) + 1) floats");
    rc = cs_check_device(plan, "jsg_istft_launch");
    if (rc != JSG_OK) return rc;
    // every refusal is behind us: chunks of new frames [a, b), each with the K frames before it that overlap its first sample
    const long long fpr = std::min(per_row, c.F);
    const long long step = per_row >= c.F ? c.F : per_row - c.K;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (long long a0 = 0; a0 < c.F; a0 += step) {
        const long long b = std::min(c.F, a0 + step), base = std::max(0LL, a0 - c.K);
        CsInvArgs k{};
        k.in = reinterpret_cast<const cs_v2*>(g->in);
        k.in_frame_pitch = g->in_frame_pitch;
        k.in_row_pitch = g->in_row_pitch;
        k.win = plan->d_win;
        k.tw = plan->d_tw;
        k.scratch = scratch;
        k.frames_per_row = fpr;
        k.first_frame = base;
        k.n_frames = b - base;
        hipError_t err = c2r_dispatch(n, k, g->rows, plan->blob.device(), s);
        if (err != hipSuccess) return jsg_fail_hip(err, "jsg_istft_launch");
        CsOlaArgs o{};
        o.scratch = scratch;
        o.frames_per_row = fpr;
        o.first_frame = base;
        o.w2 = plan->d_w2;
        o.out = g->out;
        o.out_pitch = g->out_pitch;
        o.t0 = a0 * g->hop;
        o.t1 = b == c.F ? g->out_samples : b * g->hop;
        o.n_frames = g->n_frames;
        o.n = n;
        o.hop = g->hop;
        const long long cnt = o.t1 - o.t0;
        hipLaunchKernelGGL(istft_ola_kernel, dim3((unsigned)((cnt + CS_THREADS - 1) / CS_THREADS), g->rows), dim3(CS_THREADS), 0, s, o);
        err = hipGetLastError();
        if (err != hipSuccess) return jsg_fail_hip(err, "jsg_istft_launch");
    }
    return JSG_OK;
}

}  // extern "C"
