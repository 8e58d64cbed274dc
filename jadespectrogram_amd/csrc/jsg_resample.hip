// libjsg.so, band-limited resampling by any real ratio (include/jsg.h, section 2g, and jsg_sinc_table_build of section 1).  A unit of
// its own: no kernel, launcher or table of the other units is touched.
//
// One kernel family, 1024 threads per workgroup, no scratch, no atomics, no workgroup waits on another.  A work item is (row, chunk of
// consecutive outputs); workgroups walk the items with a grid stride, so the table is loaded once per workgroup.  A chunk is worked
// off in passes of at most `sub` outputs: the input span of a pass, floor(t_first) - hw .. floor(t_last) + 1 + hw with hw =
// ceil(Z P 2^32 / S) taps per wing, goes to LDS with coalesced loads, then a lane takes one output (lanes along outputs: coalesced
// stores) and walks both wings tap by tap.  The table position of a tap is a 64-bit integer advanced by an add with carry; its upper
// half indexes the table, its lower half is the interpolation weight.  The two wings have an accumulator each and are advanced in the
// same loop iteration, so two independent chains are in flight.
//
//   resample_kernel<true, true>    "resample_lds":    the table lies in LDS beside the span (the "best" table, 131 076 B, leaves 32 KB of span)
//   resample_kernel<false, true>   "resample_l2":     the table does not fit beside the span of 256 outputs; it is read through L2 and
//                                                     the span may take the whole LDS
//   resample_kernel<true, false>   "resample_direct": not even the whole LDS holds the span of 256 outputs (a caller's table with many
//                                                     zero crossings at a large step: 2 hw reaches millions).  Nothing is staged but
//                                                     the table; the input is read through L2, lanes on neighbouring samples, and a
//                                                     chunk is one pass.
//
// Every float operation of the definition is written out (contraction is off; the two fused multiply-adds of the definition are
// explicit), and the order of the sum depends on the output index only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>

#include "jsg_internal.h"

struct jsg_resampler {
    int Z = 0, P = 0;
    jsg::DeviceBlob blob;          // win[0 .. Z P]
    const float* d_tab = nullptr;
};

namespace jsg {

constexpr int RS_THREADS = 1024;
constexpr int RS_LDS_MAX = 160 * 1024;      // a workgroup may own the whole LDS of a compute unit
constexpr int RS_MAX_SUB = 4096;            // outputs per pass, at most
constexpr int RS_DEFAULT_CHUNK = 4096;
constexpr int RS_SPAN_SLACK = 6;            // floats a span may need beyond floor((sub - 1) step) + 2 hw

struct RsArgs {
    const float* in;
    long long in_pitch;
    float* out;
    long long out_pitch;
    const float* tab;
    long long L, T, n_items, chunks;
    double step, Sd;
    unsigned long long S, lim;      // table advance per input sample; Z P 2^32
    float scale;
    int chunk, sub, hw, tab_n, span_cap;
};

template <bool TAB_LDS>
__device__ inline float rs_weight(const float* __restrict__ g_tab, const float* l_tab, unsigned long long pos) {
#pragma clang fp contract(off)
    const unsigned o = (unsigned)(pos >> 32);
    const float eta = (float)((unsigned)pos >> 8) * 0x1p-24f;
    const float w0 = TAB_LDS ? l_tab[o] : g_tab[o], w1 = TAB_LDS ? l_tab[o + 1] : g_tab[o + 1];
    return __builtin_fmaf(eta, w1 - w0, w0);
}

template <bool TAB_LDS, bool SPAN_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsArgs a) {
#pragma clang fp contract(off)
    extern __shared__ float rs_lds[];
    const int tid = threadIdx.x;
    float* xs = rs_lds;
    if (TAB_LDS) {
        for (int j = tid; j < a.tab_n; j += RS_THREADS) rs_lds[j] = a.tab[j];
        xs = rs_lds + ((a.tab_n + 3) & ~3);
    }
    for (long long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const long long row = item / a.chunks, c = item - row * a.chunks;
        const long long i0 = c * a.chunk, i1 = min(a.T, i0 + a.chunk);
        const float* src = a.in + row * a.in_pitch;
        float* dst = a.out + row * a.out_pitch;
        for (long long p0 = i0; p0 < i1; p0 += a.sub) {
            const long long p1 = min(i1, p0 + a.sub);
            long long lo = 0, hi = a.L - 1;         // SPAN_LDS = false: indices are those of the row itself
            if (SPAN_LDS) {
                const long long n_first = (long long)floor((double)p0 * a.step), n_last = (long long)floor((double)(p1 - 1) * a.step);
                lo = max(0ll, n_first - a.hw);
                hi = min(min(a.L - 1, n_last + 1 + a.hw), lo + a.span_cap - 1);      // the last bound never binds (the host sized sub)
            }
            const int top = (int)(hi - lo);
            const float* xv = SPAN_LDS ? xs : src;
            __syncthreads();        // the table is in place; the span of the pass before has been read
            if (SPAN_LDS) {
                for (int j = tid; j <= top; j += RS_THREADS) xs[j] = src[lo + j];
                __syncthreads();
            }
            for (long long i = p0 + tid; i < p1; i += RS_THREADS) {
                const double t = (double)i * a.step;
                const double fl = floor(t);
                const double f = t - fl;
                const unsigned long long F_L = (unsigned long long)__double2ll_rn(f * a.Sd);
                unsigned long long pl = F_L, pr = a.S - F_L;
                int il = (int)((long long)fl - lo), ir = il + 1;
                float acc_l = 0.f, acc_r = 0.f;
                bool live_l = pl < a.lim && il >= 0, live_r = pr < a.lim && ir <= top;
                while (live_l || live_r) {
                    if (live_l) {
                        acc_l = __builtin_fmaf(rs_weight<TAB_LDS>(a.tab, rs_lds, pl), xv[il], acc_l);
                        pl += a.S;
                        --il;
                        live_l = pl < a.lim && il >= 0;
                    }
                    if (live_r) {
                        acc_r = __builtin_fmaf(rs_weight<TAB_LDS>(a.tab, rs_lds, pr), xv[ir], acc_r);
                        pr += a.S;
                        ++ir;
                        live_r = pr < a.lim && ir <= top;
                    }
                }
                dst[i] = a.scale * (acc_l + acc_r);
            }
        }
    }
}

}  // namespace jsg

using namespace jsg;

namespace {

struct RsCall {
    long long T, chunk, chunks;
    double scale, Sd;
    unsigned long long S;
};

struct RsPath {
    bool tab_lds, span_lds;
    int hw, sub, span_cap;
    size_t lds_bytes;
};

bool step_ok(double step) { return std::isfinite(step) && step >= 1.0 / 64.0 && step <= 64.0; }

// the number of i >= 0 with (double)i * step < L, for L in 1..2^31-1 and a step in [1/64, 64]: at most 2^37
long long resample_count(long long L, double step) {
#pragma clang fp contract(off)
    long long g = (long long)std::ceil((double)L / step);
    while (g > 0 && (double)(g - 1) * step >= (double)L) --g;
    while ((double)g * step < (double)L) ++g;
    return g;
}

// everything that does not need the plan
int resample_check(const jsg_resample_args* g, const char* who, RsCall* c) {
#pragma clang fp contract(off)
    if (!g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (!g->in || !g->out) return jsg_fail_who(JSG_ERR_INVALID, who, "null data pointer");
    const uintptr_t pi = reinterpret_cast<uintptr_t>(g->in), po = reinterpret_cast<uintptr_t>(g->out);
    if ((pi & 3) != 0 || (po & 3) != 0) return jsg_fail_who(JSG_ERR_INVALID, who, "in and out must be 4-byte aligned");
    if (const int rc = check_rows(g->rows, who); rc != JSG_OK) return rc;
    if (g->in_samples < 1 || g->in_samples >= (1ll << 31)) return jsg_fail_who(JSG_ERR_INVALID, who, "in_samples must be in 1..2^31-1");
    if (!step_ok(g->step)) return jsg_fail_who(JSG_ERR_INVALID, who, "step must be finite and in 1/64..64");
    const long long L = g->in_samples, T = resample_count(L, g->step);
    if (g->out_samples != T) return jsg_fail_who(JSG_ERR_INVALID, who, "out_samples differs from jsg_resample_length(in_samples, step)");
    if (g->chunk_outputs < 0 || g->chunk_outputs > 65536) return jsg_fail_who(JSG_ERR_INVALID, who, "chunk_outputs must be 0 or in 1..65536");
    if (g->rows > 1 && g->in_pitch < L) return jsg_fail_who(JSG_ERR_INVALID, who, "in_pitch smaller than in_samples");
    if (g->rows > 1 && g->out_pitch < T) return jsg_fail_who(JSG_ERR_INVALID, who, "out_pitch smaller than out_samples");
    if (overlap(addr(g->in), span_bytes(g->rows, g->in_pitch, L, 4), addr(g->out), span_bytes(g->rows, g->out_pitch, T, 4)))
        return jsg_fail_who(JSG_ERR_INVALID, who, "out overlaps in");
    c->T = T;
    c->chunk = g->chunk_outputs ? g->chunk_outputs : RS_DEFAULT_CHUNK;
    c->chunks = (T + c->chunk - 1) / c->chunk;
    c->scale = g->step > 1.0 ? 1.0 / g->step : 1.0;
    return JSG_OK;
}

// Which kernel, and how many outputs a pass takes, for a table of Z x P.  hw = ceil(Z P 2^32 / S) taps per wing: 64 or 4097 for the
// "best" table at the ends of the step range, up to 32768 * 64 + 1 for a caller's table.  The span of k outputs is at most
// floor((k - 1) step) + 2 hw + RS_SPAN_SLACK floats.  The table goes to LDS when what it leaves holds the span of 256 outputs (or of
// the whole chunk, if that is shorter); otherwise the span may take the whole LDS; where even that does not hold 256 outputs, nothing
// is staged but the table (at most 131 088 B) and a chunk is one pass.  Every path leaves 1 <= sub and lds_bytes <= RS_LDS_MAX.
RsPath resample_path(int Z, int P, const jsg_resample_args* g, RsCall* c) {
#pragma clang fp contract(off)
    c->S = (unsigned long long)std::llrint(c->scale * (double)P * 4294967296.0);
    c->Sd = (double)c->S;
    const unsigned long long lim = (unsigned long long)Z * P << 32;
    RsPath p{};
    p.hw = (int)((lim + c->S - 1) / c->S);
    const long long want = std::min<long long>(std::min<long long>(c->chunk, c->T), RS_MAX_SUB);
    const long long fixed = 2ll * p.hw + RS_SPAN_SLACK;
    auto fit = [&](long long cap) -> long long {     // outputs whose span fits `cap` floats (0: none)
        if (cap <= fixed) return 0;
        return std::min<long long>(want, (long long)std::floor((double)(cap - fixed) / g->step) + 1);
    };
    const long long tab_floats = ((long long)Z * P + 1 + 3) & ~3ll;
    const long long enough = std::min<long long>(want, 256);
    const long long sub_lds = fit(RS_LDS_MAX / 4 - tab_floats), sub_l2 = fit(RS_LDS_MAX / 4);
    if (sub_lds >= enough) {
        p.tab_lds = p.span_lds = true;
        p.sub = (int)sub_lds;
    } else if (sub_l2 >= enough) {
        p.span_lds = true;
        p.sub = (int)sub_l2;
    } else {
        p.tab_lds = true;
        p.sub = (int)std::min<long long>(c->chunk, c->T);
    }
    p.span_cap = p.span_lds ? (int)((long long)std::floor((double)(p.sub - 1) * g->step) + fixed) : 0;
    p.lds_bytes = sizeof(float) * (size_t)((p.tab_lds ? tab_floats : 0) + p.span_cap);
    return p;
}

const char* path_name(const RsPath& p) { return !p.span_lds ? "resample_direct" : p.tab_lds ? "resample_lds" : "resample_l2"; }

// resample_check, then the path.  A pass of no outputs would never end on the device and an LDS request above the limit fails at the
// launch, so either is refused here, whatever slip in the sizing above produced it.
int resample_resolve(int Z, int P, const jsg_resample_args* g, const char* who, RsCall* c, RsPath* p) {
    const int rc = resample_check(g, who, c);
    if (rc != JSG_OK) return rc;
    *p = resample_path(Z, P, g, c);
    if (p->sub < 1 || p->lds_bytes > (size_t)RS_LDS_MAX) return jsg_fail_who(JSG_ERR_INVALID, who, "internal: no pass of this call fits the LDS");
    return JSG_OK;
}

bool table_size_ok(int Z, int P) { return Z >= 1 && P >= 1 && (long long)Z * P <= JSG_RESAMPLE_MAX_TABLE; }

double bessel_i0(double x) {
#pragma clang fp contract(off)
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 100000; ++k) {
        term = term * q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

}  // namespace

extern "C" {

int jsg_sinc_table_build(int num_zeros, int per_zero, double rolloff, double beta, float* out) {
#pragma clang fp contract(off)
    static const char* who = "jsg_sinc_table_build";
    if (!out) return jsg_fail_who(JSG_ERR_INVALID, who, "null output pointer");
    if (num_zeros < 1) return jsg_fail_who(JSG_ERR_INVALID, who, "num_zeros must be >= 1");
    if (per_zero < 1) return jsg_fail_who(JSG_ERR_INVALID, who, "per_zero must be >= 1");
    if ((long long)num_zeros * per_zero > JSG_RESAMPLE_MAX_TABLE) return jsg_fail_who(JSG_ERR_INVALID, who, "num_zeros * per_zero must be <= 32768");
    if (!(rolloff > 0.0 && rolloff <= 1.0)) return jsg_fail_who(JSG_ERR_INVALID, who, "rolloff must be in (0, 1]");
    if (!std::isfinite(beta) || beta < 0.0) return jsg_fail_who(JSG_ERR_INVALID, who, "beta must be finite and >= 0");
    const double i0b = bessel_i0(beta);
    if (!std::isfinite(i0b)) return jsg_fail_who(JSG_ERR_INVALID, who, "beta is too large: I0(beta) is not finite");
    const double pi = 3.14159265358979323846;
    const int n = num_zeros * per_zero;
    for (int j = 0; j <= n; ++j) {
        const double x = rolloff * ((double)j / (double)per_zero);
        const double sinc = j == 0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double u = (double)j / (double)n;
        const double kaiser = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
        out[j] = (float)(rolloff * sinc * kaiser);
    }
    return JSG_OK;
}

int jsg_resampler_create(jsg_resampler** out, int num_zeros, int per_zero, const float* table) {
    static const char* who = "jsg_resampler_create";
    if (!out || !table) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    *out = nullptr;
    if (num_zeros < 1) return jsg_fail_who(JSG_ERR_INVALID, who, "num_zeros must be >= 1");
    if (per_zero < 1) return jsg_fail_who(JSG_ERR_INVALID, who, "per_zero must be >= 1");
    if ((long long)num_zeros * per_zero > JSG_RESAMPLE_MAX_TABLE) return jsg_fail_who(JSG_ERR_INVALID, who, "num_zeros * per_zero must be <= 32768");
    const int n = num_zeros * per_zero + 1;
    for (int j = 0; j < n; ++j)
        if (!std::isfinite(table[j])) return jsg_fail_who(JSG_ERR_INVALID, who, "the table must be finite");
    std::unique_ptr<jsg_resampler> p(new (std::nothrow) jsg_resampler());
    if (!p) return jsg_fail_who(JSG_ERR_NOMEM, who, "out of host memory");
    p->Z = num_zeros;
    p->P = per_zero;
    int rc = p->blob.bind(who);
    if (rc != JSG_OK) return rc;
    // the kernels may ask for more than 48 KB of dynamic LDS: said once per device, here, so that a first launch may sit inside a capture
    hipError_t err = hipSuccess;
    for (const void* kernel : {reinterpret_cast<const void*>(&resample_kernel<true, true>), reinterpret_cast<const void*>(&resample_kernel<false, true>),
                               reinterpret_cast<const void*>(&resample_kernel<true, false>)})
        if (err == hipSuccess) err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_MAX);
    if (err != hipSuccess) return jsg_fail_hip(err, who);
    rc = p->blob.upload(table, sizeof(float) * (size_t)n, who);
    if (rc != JSG_OK) return rc;
    p->d_tab = static_cast<const float*>(p->blob.data());
    *out = p.release();
    return JSG_OK;
}

int jsg_resampler_destroy(jsg_resampler* rs) {
    delete rs;
    return JSG_OK;
}

int jsg_resampler_zeros(const jsg_resampler* rs) { return rs ? rs->Z : jsg_fail(JSG_ERR_INVALID, "jsg_resampler_zeros: null"); }
int jsg_resampler_per_zero(const jsg_resampler* rs) { return rs ? rs->P : jsg_fail(JSG_ERR_INVALID, "jsg_resampler_per_zero: null"); }

int64_t jsg_resample_length(int64_t in_samples, double step) {
    if (in_samples < 1 || in_samples >= (1ll << 31)) return jsg_fail(JSG_ERR_INVALID, "jsg_resample_length: in_samples must be in 1..2^31-1");
    if (!step_ok(step)) return jsg_fail(JSG_ERR_INVALID, "jsg_resample_length: step must be finite and in 1/64..64");
    return resample_count(in_samples, step);
}

int jsg_resample_launch(const jsg_resampler* rs, const jsg_resample_args* g, void* stream) {
    static const char* who = "jsg_resample_launch";
    RsCall c{};
    if (g && !rs) return jsg_fail_who(JSG_ERR_INVALID, who, "null resampler");
    int dev = -1;
    int rc = resample_check(g, who, &c);
    // every refusal of the arguments is behind us; the plan is looked at only once there is a device
    if (rc == JSG_OK) rc = current_device(&dev, who);
    if (rc != JSG_OK) return rc;
    if (rs->blob.device() != dev) return jsg_fail_who(JSG_ERR_INVALID, who, "the resampler was created on another device");
    RsPath p{};
    rc = resample_resolve(rs->Z, rs->P, g, who, &c, &p);
    if (rc != JSG_OK) return rc;
    RsArgs k{};
    k.in = g->in;
    k.in_pitch = g->rows > 1 ? g->in_pitch : 0;
    k.out = g->out;
    k.out_pitch = g->rows > 1 ? g->out_pitch : 0;
    k.tab = rs->d_tab;
    k.L = g->in_samples;
    k.T = c.T;
    k.chunks = c.chunks;
    k.n_items = (long long)g->rows * c.chunks;
    k.step = g->step;
    k.Sd = c.Sd;
    k.S = c.S;
    k.lim = (unsigned long long)rs->Z * rs->P << 32;
    k.scale = (float)c.scale;
    k.chunk = (int)c.chunk;
    k.sub = p.sub;
    k.hw = p.hw;
    k.tab_n = rs->Z * rs->P + 1;
    k.span_cap = p.span_cap;
    const dim3 grid(resident_grid(k.n_items, dev, per_cu_by_lds(RS_LDS_MAX, (long long)p.lds_bytes, 2)));   // 2048 threads per compute unit
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!p.span_lds)
        hipLaunchKernelGGL((resample_kernel<true, false>), grid, dim3(RS_THREADS), p.lds_bytes, s, k);
    else if (p.tab_lds)
        hipLaunchKernelGGL((resample_kernel<true, true>), grid, dim3(RS_THREADS), p.lds_bytes, s, k);
    else
        hipLaunchKernelGGL((resample_kernel<false, true>), grid, dim3(RS_THREADS), p.lds_bytes, s, k);
    return finish_launch(who);
}

int jsg_resample_plan(int num_zeros, int per_zero, const jsg_resample_args* g, char* name, int name_len, int32_t* pass_outputs, int32_t* lds_bytes) {
    static const char* who = "jsg_resample_plan";
    if (const int rn = check_name_buffer(who, name, name_len, false); rn != JSG_OK) return rn;
    if (!table_size_ok(num_zeros, per_zero)) return jsg_fail_who(JSG_ERR_INVALID, who, "num_zeros and per_zero must be >= 1, their product <= 32768");
    RsCall c{};
    RsPath p{};
    const int rc = resample_resolve(num_zeros, per_zero, g, who, &c, &p);
    if (rc != JSG_OK) return rc;
    put_path_name(name, name_len, path_name(p));
    if (pass_outputs) *pass_outputs = p.sub;
    if (lds_bytes) *lds_bytes = (int32_t)p.lds_bytes;
    return JSG_OK;
}

int jsg_resample_kernel_name(const jsg_resampler* rs, const jsg_resample_args* g, char* out, int out_len) {
    static const char* who = "jsg_resample_kernel_name";
    if (const int rn = check_name_buffer(who, out, out_len, true); rn != JSG_OK) return rn;
    if (g && !rs) return jsg_fail_who(JSG_ERR_INVALID, who, "null resampler");
    RsCall c{};
    RsPath p{};
    int rc = resample_check(g, who, &c);         // before the plan is read
    if (rc == JSG_OK) rc = resample_resolve(rs->Z, rs->P, g, who, &c, &p);
    if (rc != JSG_OK) return rc;
    put_path_name(out, out_len, path_name(p));
    return JSG_OK;
}

}  // extern "C"
