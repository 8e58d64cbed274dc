// libjsg.so, filterbank spectrograms: the band kernel and the launcher of jsg_stft_fb_launch(_strided) (include/jsg.h, section 2b).
//
//   launcher     resolves the STFT plan ONCE for the whole call (strided_call_variant, the rule of jsg_stft_db_launch_strided) and pins
//                every chunk to it; runs the existing STFT kernels with linear_out = 1 into the caller's scratch, a chunk of columns at a
//                time, and the band kernel after every chunk -- all on one stream, enqueue only.
//   fb_band_kernel  power columns -> band columns.  A persistent grid of 256-thread workgroups over tiles of T power columns: the tile
//                is read once with coalesced 16-byte loads into LDS; the bank (band descriptors + weights) is staged into LDS once per
//                workgroup where it fits (else read through the caches, once per tile of T columns); lanes run over the bands, every
//                lane sums its band's bins for the T columns of the tile (each weight read once, used T times), and the band values of
//                one column go out as one coalesced row.
//
// Band sum: ascending bins from +0.0f, every product and every sum rounded on its own -- no contraction into fma (the pragma in the
// kernel; __fmul_rn / __fadd_rn would not do: they are plain operators in HIP, contracted after inlining), no reordering: a float32 loop on a CPU reproduces it bit for bit.
#include "jsg_stft_kernel.h"

namespace jsg {

struct FbKArgs {
    const float* pw;              // scratch: power columns of pw_pitch floats, column q = (batch * rows + row) * cols + j
    long long pw_pitch;
    int cols;                     // columns per row in this chunk
    int rows;                     // rows per batch (channels in per-channel mode, else 1)
    int n_cols;                   // columns of the chunk (batches x rows x cols)
    int height;                   // n/2 + 1
    float* out;
    long long out_pitch, out_cpitch, out_bstride;
    int ring_w, ring_pos;         // ring column of j = 0 (ring_pos + first frame of the chunk, modulo ring_w)
    const int* desc;              // first_bin[B], n_bins[B], offset[B]
    const float* w;
    int n_bands;
    int nnz;
    int mode;                     // 0 band power, 1 dB (hardware log), 2 dB (jsg_exact_db)
};

typedef float fb_v4f __attribute__((ext_vector_type(4)));
constexpr int kFbThreads = 256;
constexpr int kFbBankBytes = 28 * 1024;     // bank staged in LDS up to this size (128 Slaney mels: 1.5 KB of descriptors + 2..33 KB)

template <int T, bool BANK_LDS>
__global__ __launch_bounds__(kFbThreads) void fb_band_kernel(const FbKArgs a) {
#pragma clang fp contract(off)
    extern __shared__ fb_v4f s_mem4[];
    float* s_pw = reinterpret_cast<float*>(s_mem4);
    const int P = int(a.pw_pitch), B = a.n_bands, tid = threadIdx.x;
    const int* first = a.desc;
    const int* count = a.desc + B;
    const int* offset = a.desc + 2 * B;
    const float* w = a.w;
    if constexpr (BANK_LDS) {
        int* s_bank = reinterpret_cast<int*>(s_pw + T * P);
        const int words = 3 * B + a.nnz;   // descriptors and weights are one contiguous allocation
        for (int i = tid; i < words; i += kFbThreads) s_bank[i] = a.desc[i];
        first = s_bank;
        count = s_bank + B;
        offset = s_bank + 2 * B;
        w = reinterpret_cast<const float*>(s_bank + 3 * B);
    }
    const int P4 = P / 4, H4 = (a.height + 3) / 4;
    const fb_v4f* pw4 = reinterpret_cast<const fb_v4f*>(a.pw);
    const int n_tiles = (a.n_cols + T - 1) / T;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int q0 = tile * T;
        if (tile != (int)blockIdx.x) __syncthreads();   // the previous tile's bands are done with the LDS columns
        for (int i = tid; i < T * H4; i += kFbThreads) {
            const int t = i / H4, k4 = i - t * H4;
            if (q0 + t < a.n_cols) s_mem4[t * P4 + k4] = pw4[(long long)(q0 + t) * P4 + k4];
        }
        // where every column of the tile goes (wave-uniform)
        long long obase[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int q = q0 + t;
            const int row = q / a.cols, j = q - row * a.cols;
            const int batch = row / a.rows, r = row - batch * a.rows;
            int col = a.ring_pos + j;
            if (col >= a.ring_w) col -= a.ring_w;
            obase[t] = (long long)batch * a.out_bstride + (long long)r * a.out_cpitch + (long long)col * a.out_pitch;
        }
        __syncthreads();
        for (int b = tid; b < B; b += kFbThreads) {
            const int f = first[b], nb = count[b], o = offset[b];
            float acc[T];
#pragma unroll
            for (int t = 0; t < T; ++t) acc[t] = 0.0f;
            for (int k = 0; k < nb; ++k) {
                const float wk = w[o + k];
#pragma unroll
                for (int t = 0; t < T; ++t) {   // written out here: the pragma above applies to the operations of this function only
                    const float prod = wk * s_pw[t * P + f + k];
                    acc[t] = acc[t] + prod;
                }
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                if (q0 + t >= a.n_cols) break;
                float v = acc[t];
                if (a.mode == 1) v = to_db(v);
                else if (a.mode == 2) v = jsg_exact_db(v);
                a.out[obase[t] + b] = v;
            }
        }
    }
}

// The numbers of one band launch, in one place: jsg_fb_band_plan reports them, the launcher launches them.
//   tile_cols  columns per tile: at most 34 KB of whole power columns in LDS (8 columns at <= 2048 points, 4 at 4096, 2 at 8192)
//   pw_pitch   floats per power column in scratch: whole 128-byte lines
//   grid       as many resident workgroups per CU as its 160 KB of LDS holds (up to 8): tiles of the other workgroups are loading while one sums
struct FbBandPlan {
    int tile_cols = 0;
    bool bank_lds = false;
    long long pw_pitch = 0;
    size_t lds = 0;
    int grid = 0;
};

static int fb_tile_cols(int n) { return n <= 2048 ? 8 : n == 4096 ? 4 : 2; }
static long long fb_pw_pitch(int n) { return ((long long)(n / 2 + 1) + 31) / 32 * 32; }

static FbBandPlan fb_band_plan(int n, int n_bands, long long nnz, long long n_cols, int n_cu) {
    FbBandPlan p;
    p.tile_cols = fb_tile_cols(n);
    p.pw_pitch = fb_pw_pitch(n);
    const long long bank_words = 3ll * n_bands + nnz;
    p.bank_lds = bank_words * 4 <= kFbBankBytes;
    p.lds = size_t(p.tile_cols) * size_t(p.pw_pitch) * 4 + (p.bank_lds ? size_t(bank_words) * 4 : 0);
    const long long n_tiles = (n_cols + p.tile_cols - 1) / p.tile_cols;
    const int per_cu = std::max(1, std::min(8, int((160u * 1024u) / std::max<size_t>(p.lds, 1))));
    p.grid = int(std::max(1ll, std::min(n_tiles, (long long)n_cu * per_cu)));
    return p;
}

template <int T>
static hipError_t launch_band(const FbKArgs& a, const FbBandPlan& p, hipStream_t s) {
    if (p.bank_lds) hipLaunchKernelGGL((fb_band_kernel<T, true>), dim3(p.grid), dim3(kFbThreads), p.lds, s, a);
    else hipLaunchKernelGGL((fb_band_kernel<T, false>), dim3(p.grid), dim3(kFbThreads), p.lds, s, a);
    return hipGetLastError();
}

static hipError_t launch_band_kernel(int n, const FbKArgs& a, int n_cu, hipStream_t s) {
    const FbBandPlan p = fb_band_plan(n, a.n_bands, a.nnz, a.n_cols, n_cu);
    switch (p.tile_cols) {
        case 8: return launch_band<8>(a, p, s);
        case 4: return launch_band<4>(a, p, s);
        default: return launch_band<2>(a, p, s);
    }
}

}  // namespace jsg

using namespace jsg;

namespace {

struct FbCall {
    const VariantRow* stft = nullptr;   // the STFT variant of every chunk: its plan_select pins them, its workgroup step is the minimum chunk
    long long rows = 1;                 // rows per batch
    long long pitch = 0;                // floats per power column in scratch
};

int fb_resolve(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* g, int n_batches, FbCall& c, const char* who) {
    if (!plan || !fb || !g) return jsg_fail_who(JSG_ERR_INVALID, who, "null argument");
    if (n_batches < 1) return jsg_fail_who(JSG_ERR_INVALID, who, "n_batches must be >= 1");
    const int n = jsg_plan_fft_size(plan);
    if (fb->n != n) return jsg_fail_who(JSG_ERR_INVALID, who, "the filterbank was built for another FFT size than the plan's");
    int dev = -1;
    const DeviceBlob::Where at = fb->blob.where(&dev);
    if (at == DeviceBlob::kNoDevice) return jsg_fail_who(JSG_ERR_NO_DEVICE, who, "no device");
    if (at != DeviceBlob::kHere || dev != plan_device(plan))
        return jsg_fail_who(JSG_ERR_INVALID, who, "the plan or the filterbank was created on another device");
    if (g->channels <= 0 || g->n_frames < 0) return jsg_fail_who(JSG_ERR_INVALID, who, "bad geometry");
    c.stft = &strided_call_variant(plan, g, n_batches, cu_count_of_device(dev));
    c.rows = g->mix_mode == JSG_MIX_PER_CHANNEL ? g->channels : 1;
    c.pitch = fb_pw_pitch(n);
    return JSG_OK;
}

}  // namespace

extern "C" {

int jsg_stft_fb_launch_strided(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* g, int n_batches, int64_t in_batch_stride,
                               int64_t out_batch_stride, float* scratch, int64_t scratch_floats, void* stream) {
    static const char* who = "jsg_stft_fb_launch";
    FbCall c;
    int rc = fb_resolve(plan, fb, g, n_batches, c, who);
    if (rc != JSG_OK) return rc;
    const int n = jsg_plan_fft_size(plan), H = n / 2 + 1;
    if (!g->in || !g->out_db || !scratch) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: null pointer");
    if (g->out_tail) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: out_tail must be NULL (band columns have no tail plane)");
    if (g->out_pitch < fb->n_bands) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: out_pitch < n_bands");
    if (g->ring_width <= 0 || g->ring_pos < 0 || g->ring_pos >= g->ring_width || g->n_frames > g->ring_width || g->first_frame < 0)
        return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: bad ring geometry (n_frames > ring_width, or ring_pos outside the ring)");
    if (in_batch_stride < 0 || out_batch_stride < 0) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: negative stride");
    if (n_batches > 1) {
        const long long extent = (c.rows - 1) * g->out_channel_pitch + (long long)(g->ring_width - 1) * g->out_pitch + fb->n_bands;
        if (out_batch_stride < extent) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: the rings of consecutive batches would overlap");
    }
    if ((reinterpret_cast<uintptr_t>(scratch) & 15) != 0) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: scratch must be 16-byte aligned");
    // columns per row the scratch holds (at most 2^28 columns per chunk: the band kernel counts them in 32 bits)
    const long long step = c.stft->step;
    const long long cap = scratch_floats > 0 ? std::min(scratch_floats / (c.rows * c.pitch), (1ll << 28) / c.rows) : 0;
    if (cap < step) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_launch: scratch holds less than one workgroup step of columns");
    if (g->n_frames == 0) return JSG_OK;
    // Every refusal the STFT launcher could raise for one of the chunks (the per-launch ones: check_stft_args; every batch reads in +
    // b * in_batch_stride), decided here for the WHOLE call before the first chunk is enqueued: a refused call enqueues nothing
    rc = check_stft_args(n, g, who);
    if (rc != JSG_OK) return rc;
    int dev = -1;
    (void)hipGetDevice(&dev);
    const int n_cu = cu_count_of_device(dev);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);

    jsg_stft_args st = *g;                   // the STFT chunks: linear power into scratch, pinned to the plan of the whole call
    if (c.stft->plan_select) st.plan_select = c.stft->plan_select;
    st.linear_out = 1;
    st.exact_log = 0;
    st.out_db = scratch;
    st.out_pitch = c.pitch;
    st.ring_pos = 0;
    st.out_tail = nullptr;
    FbKArgs ka{};
    ka.pw = scratch;
    ka.pw_pitch = c.pitch;
    ka.rows = int(c.rows);
    ka.height = H;
    ka.out_pitch = g->out_pitch;
    ka.out_cpitch = g->out_channel_pitch;
    ka.out_bstride = out_batch_stride;
    ka.ring_w = g->ring_width;
    ka.desc = fb->d_desc;
    ka.w = fb->d_w;
    ka.n_bands = fb->n_bands;
    ka.nnz = int(fb->nnz);
    ka.mode = g->linear_out ? 0 : g->exact_log ? 2 : 1;

    auto chunk = [&](long long b0, int nb, long long f0, long long m) -> int {
        st.in = g->in + b0 * in_batch_stride;
        st.first_frame = g->first_frame + f0;
        st.n_frames = m;
        st.ring_width = int(m);
        st.out_channel_pitch = m * c.pitch;
        int r = jsg_stft_db_launch_strided(plan, &st, nb, in_batch_stride, c.rows * m * c.pitch, stream);
        if (r != JSG_OK) return r;
        ka.cols = int(m);
        ka.n_cols = int(nb * c.rows * m);
        ka.out = g->out_db + b0 * out_batch_stride;
        ka.ring_pos = int((g->ring_pos + f0) % g->ring_width);
        const hipError_t err = launch_band_kernel(n, ka, n_cu, s);
        return err == hipSuccess ? JSG_OK : jsg_fail_hip(err, "jsg_stft_fb_launch: band kernel");
    };
    if (g->n_frames <= cap) {   // whole batches per chunk
        const long long per = std::max(1ll, std::min<long long>(n_batches, cap / g->n_frames));
        for (long long b0 = 0; b0 < n_batches; b0 += per) {
            rc = chunk(b0, int(std::min<long long>(per, n_batches - b0)), 0, g->n_frames);
            if (rc != JSG_OK) return rc;
        }
        return JSG_OK;
    }
    const long long m = cap / step * step;   // chunks of whole workgroup steps of one batch
    for (long long b = 0; b < n_batches; ++b)
        for (long long f0 = 0; f0 < g->n_frames; f0 += m) {
            rc = chunk(b, 1, f0, std::min(m, g->n_frames - f0));
            if (rc != JSG_OK) return rc;
        }
    return JSG_OK;
}

int jsg_stft_fb_launch(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* args, float* scratch, int64_t scratch_floats, void* stream) {
    return jsg_stft_fb_launch_strided(plan, fb, args, 1, 0, 0, scratch, scratch_floats, stream);
}

int64_t jsg_stft_fb_scratch_floats(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* g, int n_batches) {
    FbCall c;
    const int rc = fb_resolve(plan, fb, g, n_batches, c, "jsg_stft_fb_scratch_floats");
    if (rc != JSG_OK) return rc;
    const long long per_col = c.rows * c.pitch;
    const long long budget = (64ll << 20) / 4;
    const long long whole = std::max<long long>(1, g->n_frames) * n_batches * per_col;
    const long long step = c.stft->step;
    if (whole <= budget) return std::max(whole, step * per_col);
    return std::max(1ll, budget / (step * per_col)) * step * per_col;
}

int jsg_stft_fb_kernel_name(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* g, int n_batches, char* out, int out_len) {
    if (!out || out_len < 24) return jsg_fail(JSG_ERR_INVALID, "jsg_stft_fb_kernel_name: bad argument");
    FbCall c;
    const int rc = fb_resolve(plan, fb, g, n_batches, c, "jsg_stft_fb_kernel_name");
    if (rc != JSG_OK) return rc;
    std::snprintf(out, size_t(out_len), "%s", c.stft->name);
    return JSG_OK;
}

int jsg_fb_band_plan(int n, int n_bands, int64_t nnz, int64_t n_cols, int n_cu, int32_t* tile_cols, int32_t* bank_in_lds, int32_t* pw_pitch,
                     int32_t* lds_bytes, int32_t* grid) {
    static const char* who = "jsg_fb_band_plan";
    if (n != 512 && n != 1024 && n != 2048 && n != 4096 && n != 8192) return jsg_fail_who(JSG_ERR_INVALID, who, "n must be a power of two in 512..8192");
    if (n_bands < 1 || n_bands > JSG_FB_MAX_BANDS) return jsg_fail_who(JSG_ERR_INVALID, who, "n_bands outside 1..JSG_FB_MAX_BANDS");
    if (nnz < 0 || nnz > 0x7fffffffll) return jsg_fail_who(JSG_ERR_INVALID, who, "nnz outside 0..2^31-1");
    if (n_cols < 1 || n_cols > (1ll << 28)) return jsg_fail_who(JSG_ERR_INVALID, who, "n_cols outside 1..2^28 (the columns of one chunk)");
    if (n_cu < 1) return jsg_fail_who(JSG_ERR_INVALID, who, "n_cu must be >= 1");
    const FbBandPlan p = fb_band_plan(n, n_bands, nnz, n_cols, n_cu);
    if (tile_cols) *tile_cols = p.tile_cols;
    if (bank_in_lds) *bank_in_lds = p.bank_lds ? 1 : 0;
    if (pw_pitch) *pw_pitch = int32_t(p.pw_pitch);
    if (lds_bytes) *lds_bytes = int32_t(p.lds);
    if (grid) *grid = p.grid;
    return JSG_OK;
}

}  // extern "C"
