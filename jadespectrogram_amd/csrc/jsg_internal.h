// Internal helpers shared by the translation units of libjsg.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/jsg.h"
#include "jsg_launch.h"      // OncePerDevice, launch_large_lds
#include "jsg_spans.h"

namespace jsg {

// last error text of the calling thread (jsg_last_error(NULL)); engines keep their own copy too
std::string& tls_error();
int jsg_fail(int code, const char* what);
int jsg_fail_hip(hipError_t err, const char* where);
// jsg_fail with the text "<who>: <what>" (checks that several entry points share)
inline int jsg_fail_who(int code, const char* who, const char* what) { return jsg_fail(code, (std::string(who) + ": " + what).c_str()); }

// the transform sizes of every plan and table object: 512, 1024, 2048, 4096, 8192
inline bool fft_size_supported(int n) { return n >= 512 && n <= 8192 && (n & (n - 1)) == 0; }

// Loads the code object that holds `kernel` onto the current device now, on the thread that configures, not inside the first launch
// (the runtime loads lazily; querying any kernel of a translation unit loads all of them).
inline hipError_t preload_code_object(const void* kernel) {
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, kernel);
}

// A table built on the host, uploaded once to the device that is current at creation and used by launches on that device: what
// jsg_plan, jsg_filterbank, jsg_freq_axis and jsg_cstft own.  The objects keep typed pointers into data().
struct DeviceBlob {
    enum Where { kHere, kNoDevice, kElsewhere };

    DeviceBlob() = default;
    DeviceBlob(const DeviceBlob&) = delete;
    DeviceBlob& operator=(const DeviceBlob&) = delete;
    ~DeviceBlob() {
        if (d_) (void)hipFree(d_);
    }

    // records the current device; upload() does it itself unless the caller has (jsg_plan_create: device, kernel attributes, then tables)
    int bind(const char* who) {
        if (hipGetDevice(&device_) == hipSuccess) return JSG_OK;
        return jsg_fail_who(JSG_ERR_NO_DEVICE, who, "no HIP device (the engine has no CPU fallback)");
    }
    int upload(const void* host, size_t bytes, const char* who) {
        if (device_ < 0) {
            const int rc = bind(who);
            if (rc != JSG_OK) return rc;
        }
        hipError_t err = hipMalloc(&d_, bytes);
        if (err == hipSuccess) err = hipMemcpy(d_, host, bytes, hipMemcpyHostToDevice);
        return err == hipSuccess ? JSG_OK : jsg_fail_hip(err, who);
    }
    void* data() const { return d_; }
    int device() const { return device_; }
    // launch time: is the current device (stored to *current where the caller goes on to use it) the blob's?
    Where where(int* current = nullptr) const {
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return kNoDevice;
        if (current) *current = dev;
        return dev == device_ ? kHere : kElsewhere;
    }

private:
    void* d_ = nullptr;
    int device_ = -1;
};

// jsg_kernels.hip: compute units of a device (read once per device), the device a plan was created on
int cu_count_of_device(int dev);
int plan_device(const jsg_plan* plan);
// jsg_kernels.hip: the refusals of jsg_stft_args that the STFT launcher and the filterbank launcher share (message prefix `who`)
int check_stft_args(int n, const jsg_stft_args* g, const char* who);
// jsg_display_axis.hip: preload_code_object of the axis kernel (jsg_freq_axis_create)
void touch_axis_module();

// ---- what the feature units (jsg_cstft.hip and every unit after it) share; the spans of their overlap refusals are in jsg_spans.h ----

// the refusals that every unit words alike; JSG_OK where the call passes.  A unit calls them at its own place in the header's order
inline int check_rows(long long rows, const char* who) {
    return rows >= 1 && rows <= 65535 ? JSG_OK : jsg_fail_who(JSG_ERR_INVALID, who, "rows must be in 1..65535");
}
template <class... P>
int check_aligned4(const char* who, const P*... p) {
    return aligned4(p...) ? JSG_OK : jsg_fail_who(JSG_ERR_INVALID, who, "pointers must be 4-byte aligned");
}

// The two ends of a ..._plan or ..._kernel_name call: the refusal of a name buffer below 24 bytes, before any other (a plan call may
// pass no buffer, a kernel_name call must pass one), and the path's name into the buffer once the call has passed.
inline int check_name_buffer(const char* who, const char* buf, int len, bool required) {
    return (required ? !buf || len < 24 : buf && len < 24) ? jsg_fail_who(JSG_ERR_INVALID, who, "bad argument") : JSG_OK;
}
inline void put_path_name(char* buf, int len, const char* path) {
    if (buf) std::strncpy(buf, path, len);
}

// the device a launch goes to
inline int current_device(int* dev, const char* who) {
    return hipGetDevice(dev) == hipSuccess ? JSG_OK : jsg_fail_who(JSG_ERR_NO_DEVICE, who, "no HIP device");
}
// The grid of a kernel whose workgroups walk n_items with a grid stride: what the device holds at a time at per_cu workgroups per
// compute unit, or the items where they are fewer.  per_cu_by_lds: as many as `limit` bytes of LDS hold at `lds` bytes each, 1..cap.
inline unsigned resident_grid(long long n_items, int dev, long long per_cu) {
    return (unsigned)std::min<long long>(n_items, (long long)cu_count_of_device(dev) * per_cu);
}
inline long long per_cu_by_lds(long long limit, long long lds, long long cap) { return std::max<long long>(1, std::min<long long>(cap, limit / lds)); }
// after the last launch of a call: what the launches left, as the call's return code
inline int finish_launch(const char* who) {
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? JSG_OK : jsg_fail_hip(err, who);
}

// jsg_yin_host.cpp: the refusals of jsg_yin_args and how a call that passes is served (jsg_yin.hip launches by it).  A work item is a
// row and F consecutive frames; its LDS holds the frames' span ((F - 1) S + w + tau_max floats, S = min(hop, w + tau_max) between
// the frames), kYinPad floats that lanes past tau_max may read, and F rows of tau_max + 1 floats for d'.
constexpr int kYinThreads = 256;
constexpr int kYinPad = 1024;
constexpr int kYinLdsFour = 10240;          // 40 KiB: four workgroups per compute unit, where a frame fits
constexpr int kYinLdsTwo = 20480;           // 80 KiB: two
constexpr int kYinLdsOne = 40960;           // 160 KiB
constexpr int kYinFrames = 16;              // frames per item where the caller does not say
struct YinPlan {
    int NL;                    // lags a lane accumulates at a time: 1, 2, 4 or 8
    int F, S;
    long long chunks;          // ceil(T / F)
    int lds_floats;
};
int yin_check(const jsg_yin_args* g, const char* who);
void yin_resolve(const jsg_yin_args* g, YinPlan* p);
const char* yin_path_name(const YinPlan& p);

// jsg_rhythm_host.cpp: the refusals of section 2j and how a tempogram call that passes is served (jsg_rhythm.hip launches by it).  A
// work item is a row and F consecutive frames; its LDS holds F rows of windowed samples y (Wn rounded up to 4 floats each), F rows of
// Lg sums, kTgPad floats (a 16-byte read may end one float past the last row), the window table and the span of the frames
// ((F - 1) S + Wn floats, S = min(hop, Wn)).
constexpr int kTgThreads = 256;
constexpr int kTgPad = 64;
constexpr int kTgLdsFour = 10240;           // 40 KiB: four workgroups per compute unit, where a frame fits
constexpr int kTgLdsTwo = 20480;            // 80 KiB: two
constexpr int kTgLdsOne = 40960;            // 160 KiB
constexpr int kTgFrames = 16;               // frames per item where the caller does not say
struct TgPlan {
    int NL;                    // lags a lane accumulates at a time: 1, 2, 4 or 8
    int F, S;
    long long chunks;          // ceil(n_frames / F)
    int lds_floats;
};
int onset_check(const jsg_onset_args* g, const char* who);
int tempogram_check(const jsg_tempogram_args* g, const char* who);
void tempogram_resolve(const jsg_tempogram_args* g, TgPlan* p);
const char* tempogram_path_name(const TgPlan& p);
int tempo_check(const jsg_tempo_args* g, const char* who);

// jsg_cepstral_host.cpp: the refusals of section 2k and how a projection that passes is served (jsg_cepstral.hip launches by it).  A
// work item is a row and F consecutive frames.  Its LDS holds the table (M rows of B floats, staged once per workgroup), the tile (F
// rows of P = B | 1 floats: lane-per-frame reads fall into different banks) and the staged outputs (F rows of M | 1 floats).  A lane
// owns a frame, so F <= 64; a wave takes blocks of MB coefficients of all F frames; MB is 4, 5, 8, 10 or 16 by M alone.
constexpr int kMfccThreads = 256;
constexpr int kMfccLdsOne = 40960;          // 160 KiB
constexpr int kMfccFrames = 64;             // frames per item: one per lane of a wave
struct MfccPlan {
    int MB;                    // coefficients a lane accumulates at a time
    int F;
    long long chunks;          // ceil(n_frames / F)
    int lds_floats;
};
int mfcc_check(const jsg_mfcc_args* g, const char* who);
void mfcc_resolve(const jsg_mfcc_args* g, MfccPlan* p);
const char* mfcc_path_name(const MfccPlan& p);
int delta_check(const jsg_delta_args* g, const char* who);

// jsg_spectral_host.cpp: the refusals of section 2l and how a call that passes is served (jsg_spectral.hip launches by it).  A group
// of W lanes owns a frame and has FK frames in flight; a workgroup takes FK * 256 / W consecutive frames of a row per step.  NC > 0:
// the register path whose lanes hold up to NC values of a frame (K <= 64 NC); NC == 0: the streaming path.  By K alone.
constexpr int kSpThreads = 256;
constexpr int kSpMaxRegs = 65;              // values of a frame a lane keeps at most: the 4097 bins of an 8192-point transform
struct SpectralPlan {
    int NC, FK, W;
    long long groups;          // ceil(T / (FK * 256 / W)) work items per row
};
int spectral_check(const jsg_spectral_args* g, const char* who);
void spectral_resolve(const jsg_spectral_args* g, SpectralPlan* p);
const char* spectral_path_name(const SpectralPlan& p);

// Slaney's mel scale (librosa.filters.mel, htk = False): linear below 1 kHz (200/3 Hz per mel), logarithmic above (27 mels per
// factor 6.4).  Shared by the MEL_SLANEY filterbank and the MEL display axis.
inline double slaney_logstep() { return std::log(6.4) / 27.0; }
inline double slaney_hz_to_mel(double f) { return f < 1000.0 ? f / (200.0 / 3.0) : 15.0 + std::log(f / 1000.0) / slaney_logstep(); }
inline double slaney_mel_to_hz(double m) { return m < 15.0 ? (200.0 / 3.0) * m : 1000.0 * std::exp(slaney_logstep() * (m - 15.0)); }

}  // namespace jsg

// A filterbank on the device (jsg_filterbank_host.cpp creates it, jsg_filterbank.hip applies it): the CSR of jsg_filterbank_build,
// band descriptors as three int arrays of n_bands entries (first bin, bin count, weight offset) followed by the weights, one allocation
struct jsg_filterbank {
    int n = 0;
    int n_bands = 0;
    long long nnz = 0;
    jsg::DeviceBlob blob;       // first_bin[n_bands], n_bins[n_bands], offset[n_bands], then nnz floats of weights
    const int* d_desc = nullptr;
    const float* d_w = nullptr;
    std::vector<int> first, count, offset;   // host copy (jsg_filterbank_weights)
    std::vector<float> w;
};

// A display frequency axis on the device (jsg_display_axis_host.cpp creates it, jsg_display_axis.hip launches over it): the row table of
// jsg_freq_axis_build and the row tiles of the launch, one allocation.  A tile is (first row, rows, first bin, bins): at most
// kAxisTileRows consecutive rows whose bins -- those of a reduced row, k and k+1 of an interpolated one -- lie in [first bin,
// first bin + bins).  A tile spans at most kAxisSpan bins unless it is one reduced row (the kernel then walks its span in steps).
constexpr int kAxisTileRows = 64;
constexpr int kAxisSpan = 128;
struct jsg_freq_axis {
    int n = 0;
    int height = 0;
    int n_tiles = 0;
    jsg::DeviceBlob blob;         // first_bin[height], n_bins[height], interp_t[height] (float bits), then tiles[4 * n_tiles]
    const int* d_rows = nullptr;
    const int* d_tiles = nullptr;
    std::vector<float> centre_hz; // host copy (jsg_display_axis_centres)
};
