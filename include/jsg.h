/*
 * jsg.h -- C-ABI of the MI355X-native (gfx950) STFT spectrogram engine.
 *
 * This is the drop-in boundary for the hot path of JoergBitzer/JadeSpectrogram
 * (sliding-window FFT -> |X|^2 -> channel mix -> 10*log10 -> colour-map LUT -> ARGB).
 * Host code (C++/JUCE: jadespectrogram_amd/host/Spectrogram.h, or any FFI) calls HIP
 * only through these entry points: plain pointers and sizes, no C++/torch types.
 *
 * Every entry point cites the reference interface it replaces (paths are relative to the
 * reference tree, i.e. JadeSpectrogram/<file>:<line>).
 *
 * Conventions
 *   - return value: JSG_OK (0) or a negative jsg_status, except where the reference returns a
 *     count (jsg_get_mem: number of new columns, -1 on size mismatch, like Spectrogram.cpp:297-298).
 *   - nothing throws across this boundary; jsg_last_error() gives the text of the last failure.
 *   - an engine is bound to the HIP device that is current when it is created; one engine per GPU,
 *     one process per GPU for multi-GPU use (channels/streams are sharded, no collective needed).
 *   - threading: one producer thread (jsg_process_block) and one consumer thread (get_mem / display_* / setters).
 *     jsg_process_block is wait-free (a lock-free ring of page-locked memory; a worker thread of the engine makes the HIP
 *     calls); readers take their snapshot of the ring on a second HIP stream and hold the state lock only while they
 *     enqueue; what follows them waits on the GPU.  Setters quiesce the engine (the reference's m_protect around
 *     setFFTSize, Spectrogram.cpp:162).
 *   - there is NO CPU fallback: every compute entry point fails with JSG_ERR_HIP / JSG_ERR_NO_DEVICE
 *     when no gfx950 device is usable.
 */
#ifndef JSG_H_
#define JSG_H_

#include <stddef.h>
#include <stdint.h>

/* libjsg.so is built with -fvisibility=hidden: only the entry points declared here are exported. */
#if defined(__GNUC__)
#define JSG_API __attribute__((visibility("default")))
#else
#define JSG_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define JSG_ABI_VERSION 6   /* 3: + kernel-name query, launch pool, image scratch query, sharded set; 4: + strided image batches (round 3);
                               5: + strided dB batches, exact-log mode, producer ring statistics (round 4);
                               6: + lossless producer call, all-or-nothing sharded push, exact-log display path, tail plane, pair plan (round 5);
                                  additions to 6: filterbank spectrograms (jsg_filterbank_*, jsg_stft_fb_*; section 2b),
                                  display frequency axes (jsg_freq_axis_*, jsg_colormap_axis_launch, jsg_display_set_freq_axis,
                                  jsg_display_height, jsg_display_axis_centres; section 2c),
                                  complex STFT and inverse STFT with any hop (jsg_cstft_*, jsg_istft_*; section 2d); additive since: the
                                 phase vocoder (jsg_pvoc_*; section 2e), harmonic-percussive separation (jsg_hpss_*; section 2f),
                                 band-limited resampling (jsg_sinc_table_build, jsg_resampler_*, jsg_resample_*; section 2g),
                                 constant-Q and variable-Q spectrograms by direct evaluation (jsg_cqt_*; section 2h),
                                 the band launch query (jsg_fb_band_plan; section 2b),
                                 YIN fundamental-frequency tracking (jsg_yin_*; section 2i),
                                 onset strength, autocorrelation tempogram and tempo (jsg_onset_*, jsg_tempogram_*, jsg_tempo_*; section 2j),
                                 cepstral coefficients and delta features (jsg_mfcc_*, jsg_delta_*; section 2k),
                                 spectral shape descriptors (jsg_spectral_shape_*; section 2l) */

typedef enum jsg_status {
    JSG_OK = 0,
    JSG_ERR_SIZE_MISMATCH = -1, /* the reference's "-1" (Spectrogram.cpp:297-298) */
    JSG_ERR_INVALID = -2,       /* bad argument */
    JSG_ERR_UNSUPPORTED = -3,   /* e.g. FFT size outside 512..8192 or not a power of two */
    JSG_ERR_HIP = -4,           /* a HIP call failed; see jsg_last_error */
    JSG_ERR_NO_DEVICE = -5,
    JSG_ERR_NOMEM = -6
} jsg_status;

/* Spectrogram::ChannelMixMode, Spectrogram.h:84-91 (same order). PER_CHANNEL is an extension:
 * no mix, one spectrogram per channel (what channel-sharded multi-GPU runs produce). */
typedef enum jsg_mix_mode {
    JSG_MIX_ABSMEAN = 0, JSG_MIX_MAX = 1, JSG_MIX_MIN = 2, JSG_MIX_LEFT = 3, JSG_MIX_RIGHT = 4,
    JSG_MIX_PER_CHANNEL = 100,
    JSG_MIX_SUM = 101           /* extension: plain sum over the local channels, no divide (partial of a
                                   cross-GPU AbsMean; finished by jsg_db_from_power_launch after the reduce) */
} jsg_mix_mode;

/* Spectrogram::Windows, Spectrogram.h:92-100 (same order; the GUI casts combo indices to it,
 * Spectrogram.cpp:409). */
typedef enum jsg_window {
    JSG_WIN_RECT = 0, JSG_WIN_HANN = 1, JSG_WIN_HAMMING = 2, JSG_WIN_BLACKMANHARRIS = 3,
    JSG_WIN_FLATTOP = 4, JSG_WIN_HANNPOISSON = 5
} jsg_window;

/* Spectrogram::FeedPercentage, Spectrogram.h:101-107. */
typedef enum jsg_feed { JSG_FEED_100 = 0, JSG_FEED_50 = 1, JSG_FEED_25 = 2, JSG_FEED_10 = 3 } jsg_feed;

/* CColorPalette scheme ids, CColorpalette.h:9-18. */
typedef enum jsg_colorscheme {
    JSG_CM_MONO = 0, JSG_CM_BW = 1, JSG_CM_HOT = 2, JSG_CM_RAINBOW = 3, JSG_CM_VIRIDIS = 4,
    JSG_CM_PLASMA = 5, JSG_CM_JADE = 6
} jsg_colorscheme;

JSG_API int jsg_abi_version(void);
/* Number of usable gfx950 devices (0 when there is none; never initialises a context). */
JSG_API int jsg_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * 1. Host-side precompute that feeds the kernels (pure integer / double arithmetic, no GPU).
 * ------------------------------------------------------------------------------------------------ */

/* m_feed_samples = int(m_feed_percent*0.01*m_fftsize+0.5)           -- Spectrogram.cpp:216 */
JSG_API int jsg_feed_samples(float feed_percent, int fftsize);
/* m_memsize_blocks = int(m_memsize_s*m_fs/m_feed_samples + 0.5)     -- Spectrogram.cpp:217 */
JSG_API int jsg_memsize_blocks(float memsize_s, float fs, int feed_samples);
/* Spectrogram::getnextpowerof2                                       -- Spectrogram.cpp:171-176 */
JSG_API int jsg_next_power_of_2(float fftsize_ms, float fs);
/* Spectrogram::setWindowFkt: n RMS-normalised window samples        -- Spectrogram.cpp:239-293 */
JSG_API int jsg_window_build(int window, int n, float* out);
/* CColorPalette::ComputeColors: n_colors ints 0x00RRGGBB             -- CColorpalette.cpp:106-339 */
JSG_API int jsg_colormap_build(int n_colors, int scheme, int32_t* lut_out);
/* CColorPalette::setValueRange: resolves (lo,hi) -> m_Min, m_Max, m_AccessMult -- CColorpalette.cpp:39-54 */
JSG_API int jsg_colormap_range(int n_colors, float lo, float hi, float* vmin, float* vmax, float* access_mult);
/* The windowed-sinc table of section 2g, num_zeros * per_zero + 1 floats: with Z = num_zeros, P = per_zero,
 *     out[j] = rolloff * sinc(rolloff * j / P) * I0(beta * sqrt(1 - (j / (Z P))^2)) / I0(beta),   sinc(x) = sin(pi x) / (pi x),
 * evaluated in double (I0 by its power series) and rounded to float once; out[0] == (float)rolloff.  Kaiser designs in the style of
 * resampy: "best" = (64, 512, 0.9475937167399596, 14.769656459379492), "fast" = (16, 512, 0.85, 8.555504641634386).
 * Refused (JSG_ERR_INVALID): a null pointer, Z < 1, P < 1, Z * P > JSG_RESAMPLE_MAX_TABLE, a rolloff outside (0, 1], a beta that is
 * negative or not finite. */
#define JSG_RESAMPLE_MAX_TABLE 32768
JSG_API int jsg_sinc_table_build(int num_zeros, int per_zero, double rolloff, double beta, float* out);

/* ------------------------------------------------------------------------------------------------
 * 2. Stateless device operations.  Every data pointer is a DEVICE pointer on the current device;
 *    `stream` is a hipStream_t (NULL = default stream).  Asynchronous: they only enqueue.
 * ------------------------------------------------------------------------------------------------ */

/* FFT plan: twiddle / window tables resident in HBM for one (fft size, window).  Replaces the
 * `spectrum m_fft` member + m_window (Spectrogram.h:157-159; Spectrogram.cpp:215, :239-293).
 * `window` = n host floats; it is multiplied by sqrt(power_scale) when the tables are built. */
typedef struct jsg_plan jsg_plan;
JSG_API int jsg_plan_create(jsg_plan** out, int n, const float* window, float power_scale);
JSG_API int jsg_plan_destroy(jsg_plan* plan);
JSG_API int jsg_plan_fft_size(const jsg_plan* plan);

/* One launch of the fused kernel: framing + window + real FFT + |X|^2 + channel mix + 10*log10
 * + ring store.  Replaces the body of Spectrogram::processSynchronBlock's frame loop
 * (Spectrogram.cpp:50-119) incl. computePowerSpectrum (:137-145) and spectrum::power (:144).
 *
 * Frame j (j = first_frame .. first_frame+n_frames-1) of channel c reads n samples starting at
 *     in[c*in_pitch + (j / feedblocks)*n + (j % feedblocks)*hop]
 * (for a regular hop this is j*hop; the split reproduces the reference's irregular `perc10` hop).
 * The caller provides the stream WITH the reference's n leading zeros if it wants the reference's
 * time line; the engine API below does that itself.
 * Column i of this launch is written to ring column (ring_pos + i) % ring_width:
 *     out_db[col*out_pitch + bin],  bin = 0..n/2          (per-channel mode: + c*out_channel_pitch)
 */
typedef struct jsg_stft_args {
    const float* in;
    int64_t in_pitch;        /* floats between channel rows */
    int32_t channels;
    int32_t hop;
    int32_t feedblocks;
    int32_t mix_mode;        /* jsg_mix_mode */
    int64_t first_frame;
    int64_t n_frames;
    float* out_db;
    int64_t out_pitch;       /* floats between ring columns (>= n/2+1) */
    int64_t out_channel_pitch;
    int32_t ring_width;
    int32_t ring_pos;
    int32_t linear_out;      /* 0: dB = 10*log10(p + 1e-11f) (the reference's column); 1: mixed linear power p */
    int32_t blocks_per_cu;   /* 0: default (up to 8 workgroups per CU -- 16 or 32 in strided multi-batch launches of the small-workgroup plans --
                                the rest of the frames is looped over); smaller values make
                                fewer, longer-lived workgroups that prefetch their next frame -- better when several
                                launches run concurrently, worse for one launch alone */
    int64_t in_samples;      /* floats of every channel row that may be read; the launch is refused (JSG_ERR_INVALID) when
                                its last frame would read past them.  0: unknown, not checked */
    int32_t plan_select;     /* 1024 points (round 6): 0 automatic -- the two-stage kernel "Cfg1024B" (split-radix 16 x 32, four frames
                                per wavefront, one 8-wave workgroup of 32 columns per CU) where >= 4 channels are mixed into one column
                                (AbsMean / Sum) and the launch fills its rounds, the three-stage kernel "Cfg1024" otherwise; 1: always
                                "Cfg1024" (the engine pins this); 2: "Cfg1024B" wherever it exists (float columns, not Max / Min, not the
                                display launches).  The two agree inside the float32 bound, not bit for bit.
                                2048 / 4096 points have two kernels each.  0: automatic -- the large-workgroup "B" kernel (one 8-wave
                                workgroup of 16 / 8 columns per CU; faster when it can fill the GPU) for launches that fill their
                                rounds of <CU count> workgroups to at least 87 % (e.g. 3584..4096 columns of 2048 points or
                                1784..2048 of 4096 points on 256 CUs, or any launch of 7 rounds and more) AND, at 2048 points, mix
                                >= 2 channels per column (at 4096 points "B" is ahead at every channel count); the small-workgroup
                                kernel otherwise.  1: always the small-workgroup kernel, 2: always "B".  The two round differently in
                                the last bits (both inside the parity bound): callers that cut one stream into launches of
                                very different sizes and need bit-identical columns pin one of them (the engine pins 1).
                                jsg_stft_kernel_name() tells which one a launch takes.  3 (2048 points, round 5): the PAIR plan "Cfg2048P"
                                where it applies -- AbsMean / Sum over an even channel count, dB / power launches: two channels as one
                                complex transform z = x_c + i x_(c+1), sum |X_c|^2 = (|Z[k]|^2 + |Z[N-k]|^2) / 2 (a reassociation of the
                                mix of Spectrogram.cpp:64-76 inside the parity bound); as 0 where it does not.  Never chosen
                                automatically: on an MI355X it is slower than "B" (DESIGN.md section 6).  Other sizes: ignored */
    int32_t exact_log;       /* 0: 10*log10 on the hardware log unit (1 ulp, not specified bit for bit); 1: by the library's own float32
                                routine (jadespectrogram_amd/csrc/jsg_exact_math.h: exponent + degree-9 polynomial, within 2 ulp of the
                                reference's double log10): every dB value -- and so every palette index and ARGB pixel -- is then
                                reproducible bit for bit on a CPU (oracle/jsg_mirror.c does).  A separate instantiation of the kernel
                                whose epilogue calls the routine (16 instead of 3 vector instructions per value): every launch form takes
                                it -- jsg_stft_db_launch, _strided, _batches, jsg_stft_image_launch(_strided) in both of its forms, the
                                engine via jsg_set_exact_log.  (round 4: a second elementwise pass, dB launches only) */
    int32_t reserved0;       /* 0 */
    float* out_tail;         /* NULL: the reference's column layout, bin n/2 at out_db[col*out_pitch + n/2].  Otherwise: a dense plane of
                                one float per ring column; bin n/2 of ring column col is written to out_tail[r*ring_width + col] (r = 0, or
                                the channel in per-channel mode, or batch * planes + channel in a strided launch: rows x ring_width floats)
                                and NOT into the column, whose pitch may then be n/2 floats (>= n/2): a column is exactly n/2 * 4 bytes of
                                whole 128-byte lines and the 4-byte piece that opened one more line per column is gone (N = 1024: 16
                                lines instead of 16 + 1/32).  Values are bit-identical to the reference layout.  dB launches only
                                (jsg_stft_db_launch, _strided, _batches); must be NULL for the image launches */
} jsg_stft_args;
JSG_API int jsg_stft_db_launch(const jsg_plan* plan, const jsg_stft_args* args, void* stream);
/* The kernel configuration jsg_stft_db_launch picks for these arguments on the current device, as text ("Cfg1024", "Cfg2048",
 * "Cfg2048B", "Cfg4096B", ...; out_len >= 24): lets a benchmark or a test name -- and pin -- the kernel it times or checks. */
JSG_API int jsg_stft_kernel_name(const jsg_plan* plan, const jsg_stft_args* args, char* out, int out_len);

/* `count` independent launches issued from one call, launch i on streams[i % n_streams] (hipStream_t handles; NULL or
 * n_streams == 0: the default stream).  For batches that do not depend on each other (distinct input and output
 * buffers): takes the per-launch FFI cost out of the caller's loop and, with more than one stream, lets the tail of
 * one launch overlap the ramp-up of the next.  Ordering between the streams is the caller's business. */
JSG_API int jsg_stft_db_launch_many(const jsg_plan* plan, const jsg_stft_args* args, int count, void* const* streams, int n_streams);
/* The same issued by n_threads host threads (stream k belongs to thread k % n_threads, so the order inside a stream
 * is kept): for callers whose single issuing thread (~3.5 us per launch) is slower than the GPU. */
JSG_API int jsg_stft_db_launch_many_threads(const jsg_plan* plan, const jsg_stft_args* args, int count, void* const* streams,
                                    int n_streams, int n_threads);

/* Independent launches that CANNOT be laid out at a stride (otherwise: jsg_stft_db_launch_strided below, one kernel launch for all of
 * them): `count` launches (no two of them write the same ring columns), stream-ordered with respect to `stream` like one launch -- they
 * start after everything that was enqueued on `stream` before the call, and work enqueued on `stream` after the call sees all their
 * results -- but spread over FOUR working streams: the caller's own plus three that the library owns (created once per device, in
 * jsg_plan_create), issued by two host threads, so that the ramp-up and drain of consecutive launches overlap.  Two working streams for
 * the one-workgroup-per-CU kernels of 2048 / 4096 points.  The caller neither creates streams nor knows the good stream count; it must
 * not enqueue on `stream` from another thread during the call.
 * Hardware queues: the GPU's compute front end serves four hardware queues at a time.  A FIFTH busy queue makes the command processor
 * time-slice them (measured at C2: 1.08e9 frames/s with four busy queues, 0.35e9 with five) -- which is why the caller's stream is one of
 * the four working streams and not a fifth beside them -- and two busy streams that the HIP runtime maps onto ONE hardware queue
 * serialise.  The runtime multiplexes all streams of the process onto GPU_MAX_HW_QUEUES queues (default 4) in creation order (measured
 * with nine streams in the process: 0.79 / 0.41 / 0.84 / 1.08 / 1.08e9 frames/s at 4 / 6 / 8 / 12 / 16 queues): a host that wants this
 * entry point at its full rate exports GPU_MAX_HW_QUEUES=16 itself before its first HIP call.  The library does not touch the
 * environment (rounds 2-3 set the variable from a constructor: not thread-safe inside a multi-threaded host, and it changed every
 * other HIP user of the process).  Calls for one device are serialised on the host.  Inside a stream capture (hipGraph) the launches are
 * issued by the calling thread and become parallel branches of the graph; every forked stream is joined even when a launch fails. */
JSG_API int jsg_stft_db_launch_batches(const jsg_plan* plan, const jsg_stft_args* args, int count, void* stream);

/* `n_batches` independent batches of ONE geometry in ONE kernel launch on ONE stream (the frame loop of
 * Spectrogram::processSynchronBlock, Spectrogram.cpp:50-119, over K streams' worth of blocks): `args` describes batch 0; batch b reads
 * args->in + b * in_batch_stride (floats; 0 = the same input) and writes its own ring at args->out_db + b * out_batch_stride (floats,
 * at least one ring: the rings must not overlap).  Everything else in `args` (frame count, hop, ring_pos, mix, in_samples -- which then
 * holds for the rows of EVERY batch) is the same for all batches.  The workgroups of the one launch walk through the columns of all
 * batches: lane tables loaded once per workgroup instead of once per step of four to sixteen frames, no ramp-up and drain per batch, the next columns in
 * flight while the current ones are transformed -- the rate of back-to-back launches without extra streams, hardware queues or issuing
 * threads (bench.py's default C2 step).  args->blocks_per_cu: workgroups per CU of the grid (0 = the library's choice).
 *   1024 / 2048 / 4096 points: the plan rule of plan_select looks at the frames of the WHOLE call and decides once for all of it;
 *   columns are those of single launches with plan_select pinned to that plan.  512 / 8192 points: bit-identical to single launches.
 * Max / Min mixes have no strided kernel: they are launched batch by batch in stream order, and the plan rule looks at the frames of
 * ONE batch (each launch keeps the faster kernel for its real size).  More than 2^20 workgroup steps go out as several launches, all
 * pinned to the plan of the whole call.  jsg_stft_db_strided_kernel_name tells the kernel every launch of the call takes. */
JSG_API int jsg_stft_db_launch_strided(const jsg_plan* plan, const jsg_stft_args* args, int n_batches, int64_t in_batch_stride,
                               int64_t out_batch_stride, void* stream);
JSG_API int jsg_stft_db_strided_kernel_name(const jsg_plan* plan, const jsg_stft_args* args, int n_batches, int64_t in_batch_stride, char* out,
                                    int out_len);

/* out[i] = 10*log10(power[i]/divisor + 1e-11f), i < count: the tail of the mix (reference Spectrogram.cpp:74,107)
 * for partial sums that were reduced across GPUs (JSG_MIX_SUM).  In place (out == power) is allowed. */
JSG_API int jsg_db_from_power_launch(const float* power, float* out, int64_t count, float divisor, void* stream);
/* ... with the logarithm of jsg_stft_args.exact_log (1) instead of the hardware unit (0) */
JSG_API int jsg_db_from_power_launch_ex(const float* power, float* out, int64_t count, float divisor, int exact_log, void* stream);

/* The reference's dense column shape out of the tail-plane layout (jsg_stft_args.out_tail): dst[col*dst_pitch + bin] for bin < height - 1 from
 * db[col*db_pitch + bin], and dst[col*dst_pitch + height - 1] from tail[col], col < n_columns (one ring / one row of the plane; height = n/2 + 1).
 * What Spectrogram::getMem hands out (m_mem[col][bin], Spectrogram.h:144, Spectrogram.cpp:295-331) for callers that computed in whole-line
 * columns.  Device pointers; db_pitch >= height - 1, dst_pitch >= height. */
JSG_API int jsg_columns_from_tail_layout_launch(const float* db, int64_t db_pitch, const float* tail, int n_columns, int height, float* dst,
                                        int64_t dst_pitch, void* stream);

/* Roofline calibration (no reference counterpart): a tuned float4 streaming copy of `bytes` bytes (multiple of 16, 16-byte aligned
 * device pointers), non-temporal loads and stores, one thread per 16 bytes.  bench.py times it on buffers that rotate over > 1 GB to
 * report what the HBM of THIS box gives a balanced read + write stream (`peak_copy_GBps`), the yardstick beside the 8 TB/s spec. */
JSG_API int jsg_calib_copy_launch(const void* src, void* dst, int64_t bytes, void* stream);

/* Colour loop: dB ring columns -> ARGB pixels (and/or 8-bit palette indices).
 * Replaces the pixel loops of SpectrogramComponent::timerCallback (Spectrogram.cpp:632-648,
 * :673-680, :693-700) with CColorPalette::getRGBColor inlined (CColorpalette.h:32-47):
 *     pixel(x, height-1-bin) = lut[index(db[col][bin])] | 0xFF000000
 * for i in [0,n_cols): col = (col_first+i) % ring_width, x = (x_first+i) % x_wrap.
 * Image layout is row-major [height][img_pitch] (what juce::Image::BitmapData exposes). */
typedef struct jsg_colormap_args {
    const float* db;
    int64_t db_pitch;
    int32_t ring_width;
    int32_t height;          /* bins = n/2+1 */
    int32_t col_first;
    int32_t n_cols;
    int32_t x_first;
    int32_t x_wrap;          /* image width */
    const int32_t* lut;      /* device, n_colors entries 0x00RRGGBB */
    int32_t n_colors;
    float vmin, vmax, access_mult;   /* from jsg_colormap_range */
    uint32_t* argb_out;      /* may be NULL */
    int64_t argb_pitch;      /* pixels between image rows */
    uint8_t* index_out;      /* may be NULL; requires n_colors <= 256 */
    int64_t index_pitch;
} jsg_colormap_args;
JSG_API int jsg_colormap_launch(const jsg_colormap_args* args, void* stream);

/* Fused display path: STFT -> palette index -> ARGB without the dB column ever going to memory (reference
 * Spectrogram.cpp:632-648: the colour loop consumes the column the engine has just produced).  The image is bit-identical to
 * jsg_stft_db_launch (same plan_select) followed by jsg_colormap_launch -- except at 1024 points, where the display launches always
 * take the three-stage arithmetic ("Cfg1024"), whatever plan_select says: the image is that of jsg_stft_db_launch with plan_select = 1.
 *   ONE kernel where a workgroup of the plan holds eight whole columns -- 1024 points, and 4096 points when the launch takes the
 *   one-wavefront-per-frame kernel (automatic rule of jsg_stft_args.plan_select, or plan_select = 2; e.g. a 10-second stereo image
 *   at 96 kHz = 1875 columns): the workgroup parks the palette indices (CColorPalette::getRGBColor's index, CColorpalette.h:34-45)
 *   of its columns in LDS and writes the ARGB rows itself; only the input is read, only the image is written, `index_scratch`
 *   is not touched and may be NULL.  Needs colour.argb_out, no colour.index_out, n_colors <= 256, n_cols <= x_wrap.
 *   TWO kernels otherwise: the STFT kernel writes 1 byte per bin into `index_scratch`, the colour kernel reads those bytes.
 * jsg_stft_image_needs_scratch() tells which (1: index_scratch is required, 0: it is not used).
 * stft.out_db may be NULL (it is not written); colour.db is ignored; colour must cover exactly the columns of the launch
 * (n_cols == n_frames, col_first == ring_pos, ring_width equal, height n/2+1); n_colors <= 256; mixes: AbsMean / Sum / Left / Right. */
typedef struct jsg_stft_image_args {
    jsg_stft_args stft;
    jsg_colormap_args colour;
    uint8_t* index_scratch;        /* device: ring_width columns of index_scratch_pitch bytes each (two-kernel form only) */
    int64_t index_scratch_pitch;   /* >= n/2+1; a multiple of 64 keeps the columns line-aligned */
} jsg_stft_image_args;
JSG_API int jsg_stft_image_launch(const jsg_plan* plan, const jsg_stft_image_args* args, void* stream);
JSG_API int jsg_stft_image_needs_scratch(const jsg_plan* plan, const jsg_stft_image_args* args);
/* `n_images` images of ONE geometry from one call (a batch of independent streams, or the pages of a long recording): `args`
 * describes one image; image i reads args->stft.in + i * in_image_stride (floats, >= 0) and writes args->colour.argb_out +
 * i * argb_image_stride (pixels, >= height * argb_pitch).  Where the single-kernel form applies to a launch of the TOTAL size
 * (1024 points; 4096 points when all images together fill the one-workgroup-per-CU kernel's rounds, or plan_select = 2) the images
 * share ONE kernel launch whose workgroups walk through the columns of all of them: tables loaded once, the next columns in flight
 * while the current ones are transformed, no idle workgroup slots at the end of every image (C5, 1875 columns = 235 groups of
 * eight on 256 CUs: see DESIGN.md 4.4 for the measured gain).  Pixels: those of n_images jsg_stft_image_launch calls with plan_select pinned to the
 * plan the whole launch takes (the plan rule looks at the total column count; 1024 points: the three-stage arithmetic, as a single
 * launch).  Otherwise: n_images launches in stream order, which need `index_scratch` like a single one
 * (jsg_stft_image_strided_needs_scratch tells).  colour.index_out must be NULL. */
JSG_API int jsg_stft_image_launch_strided(const jsg_plan* plan, const jsg_stft_image_args* args, int n_images, int64_t in_image_stride,
                                  int64_t argb_image_stride, void* stream);
JSG_API int jsg_stft_image_strided_needs_scratch(const jsg_plan* plan, const jsg_stft_image_args* args, int n_images);

/* ------------------------------------------------------------------------------------------------
 * 2b. Filterbank spectrograms: mel and log-frequency rows (no reference counterpart; the reference stores its
 *     MinFreq / MaxFreq as log(Hz), Spectrogram.h:24-39, and stretches a linear bin range, Spectrogram.cpp:441-463).
 *
 *     A bank is sparse and banded: band b has the weights w[b][k] of the bins k = first_bin[b] .. first_bin[b]+n_bins[b]-1,
 *     stored at weights[offset[b] ..] (CSR).  Band power and value of one column (power P_k = the mixed linear power of
 *     jsg_stft_args.linear_out = 1, bit for bit):
 *         acc = +0.0f;  for k ascending over the band:  acc = acc + w[b][k] * P_k
 *     in float32, every product and every sum rounded separately (no fused multiply-add, no reordering), and
 *         value = acc (linear_out = 1),  10*log10(acc + 1e-11f) on the hardware unit (exact_log = 0, the STFT epilogue's
 *         logarithm), or jsg_exact_db of acc (exact_log = 1; jadespectrogram_amd/csrc/jsg_exact_math.h: bit-reproducible on a CPU).
 *     An empty band (n_bins = 0) has power 0 and reads 10*log10(1e-11f), about -110 dB.
 * ------------------------------------------------------------------------------------------------ */
typedef enum jsg_fb_scale { JSG_FB_MEL_SLANEY = 0, JSG_FB_MEL_HTK = 1, JSG_FB_LOG = 2, JSG_FB_LINEAR = 3 } jsg_fb_scale;
typedef enum jsg_fb_norm { JSG_FB_NORM_NONE = 0, JSG_FB_NORM_SLANEY = 1, JSG_FB_NORM_UNIT_SUM = 2 } jsg_fb_norm;
#define JSG_FB_MAX_BANDS 8192
typedef struct jsg_fb_spec {
    int32_t n;          /* FFT size: a power of two in 512..8192 */
    float fs;           /* sample rate, Hz (> 0) */
    int32_t n_bands;    /* 1..JSG_FB_MAX_BANDS (LOG / LINEAR: >= 2) */
    float fmin, fmax;   /* Hz: 0 <= fmin < fmax <= fs/2 (LOG: fmin > 0) */
    int32_t scale;      /* jsg_fb_scale */
    int32_t norm;       /* jsg_fb_norm */
} jsg_fb_spec;
/* The bank of a spec, on the host (no GPU).  All arithmetic in double, every weight rounded to float32 once.  Positions are fractional
 * bins, x = f * n / fs (bin k sits at x = k).  A triangle (lo, c, hi) gives bin k the weight max(0, min((k-lo)/(c-lo), (hi-k)/(hi-c)));
 * zero weights at either end of a band are trimmed (a band may be empty: n_bins 0, first_bin 0).
 *   MEL_SLANEY / MEL_HTK (librosa.filters.mel, htk = False / True): B+2 points equally spaced in mel between mel(fmin) and mel(fmax);
 *       band b = the triangle (p_b, p_b+1, p_b+2).  Slaney: mel = f / (200/3) below 1 kHz, 15 + ln(f/1000) / (ln(6.4)/27) above;
 *       HTK: mel = 2595 log10(1 + f/700).  centre_hz[b] = p_b+1.
 *   LOG (display rows): centres c_b = fmin r^b, r = (fmax/fmin)^(1/(B-1)), c_-1 and c_B extend the progression;
 *       lo_b = min(x(c_b-1), x(c_b) - 1), hi_b = max(x(c_b+1), x(c_b) + 1): a row narrower than a bin is the linear interpolation
 *       between its two neighbouring bins.  centre_hz[b] = c_b.
 *   LINEAR: as LOG with c_b = fmin + b (fmax - fmin)/(B-1) (the reference's min / max-frequency zoom, any pixel height).
 *   NORM_SLANEY: band b times 2 / (hi - lo) in Hz.  NORM_UNIT_SUM: band b divided by its weight sum (a flat spectrum keeps its
 *       level; the natural choice for LOG / LINEAR).
 * Outputs: first_bin, n_bins, offset, centre_hz of n_bands entries each, weights of *nnz floats (weights_cap >= *nnz, else
 * JSG_ERR_SIZE_MISMATCH with *nnz set).  weights == NULL: only *nnz is computed (the other arrays may then be NULL as well).
 * JSG_ERR_INVALID for a spec outside the ranges above. */
JSG_API int jsg_filterbank_build(const jsg_fb_spec* s, int32_t* first_bin, int32_t* n_bins, int32_t* offset, float* centre_hz,
                                 float* weights, int64_t weights_cap, int64_t* nnz);

/* A bank resident on the device that is current at creation (uploaded once, like jsg_plan_create). */
typedef struct jsg_filterbank jsg_filterbank;
JSG_API int jsg_filterbank_create(jsg_filterbank** out, const jsg_fb_spec* s);
/* A caller's dense bank w[n_bands][n/2+1] (host floats); each row keeps the span from its first to its last nonzero weight
 * (interior zeros are kept).  n: a power of two in 512..8192, 1 <= n_bands <= JSG_FB_MAX_BANDS, finite weights. */
JSG_API int jsg_filterbank_create_matrix(jsg_filterbank** out, int n, int n_bands, const float* w);
JSG_API int jsg_filterbank_destroy(jsg_filterbank* fb);
JSG_API int jsg_filterbank_bands(const jsg_filterbank* fb);
JSG_API int jsg_filterbank_fft_size(const jsg_filterbank* fb);
/* The weights as a dense host matrix [n_bands][n/2+1] (zeros outside every band's span). */
JSG_API int jsg_filterbank_weights(const jsg_filterbank* fb, float* dense);

/* STFT + filterbank: the columns of jsg_stft_db_launch(_strided) with the bank applied.  `args` keeps its meaning, except:
 *   out_db is a ring of BAND columns: out_db[col*out_pitch + b], b < n_bands, out_pitch >= n_bands (per-channel mode: + c*out_channel_pitch);
 *   linear_out = 1 writes band power instead of dB; exact_log selects the logarithm (see above); out_tail must be NULL.
 * Every mix, per-channel included.  The launcher runs the STFT kernel (linear power) into the caller's `scratch` (device floats,
 * 16-byte aligned; the layout is private to the library) in chunks of as many columns as scratch_floats holds, and after each chunk the
 * band kernel on it -- all on `stream`, enqueue only (no allocation, no synchronisation; hipGraph capture works).  The STFT plan is
 * resolved ONCE for the whole call, by the rule of jsg_stft_db_launch_strided (the frames of all rows of the call decide), and every
 * chunk is pinned to it: the result does not depend on scratch_floats, and jsg_stft_fb_kernel_name reports that plan.  Refused
 * (JSG_ERR_INVALID): scratch smaller than one workgroup step of the plan (rows x step columns), a bank of another FFT size, a bank or plan
 * of another device, null pointers, n_frames > ring_width -- and every argument jsg_stft_db_launch(_strided) refuses.  All refusals are
 * decided for the whole call before its first chunk is enqueued: a refused call enqueues nothing.  A single call is the strided call with
 * n_batches = 1. */
JSG_API int jsg_stft_fb_launch(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* args, float* scratch, int64_t scratch_floats,
                               void* stream);
JSG_API int jsg_stft_fb_launch_strided(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* args, int n_batches, int64_t in_batch_stride,
                                       int64_t out_batch_stride, float* scratch, int64_t scratch_floats, void* stream);
/* A recommended scratch size (floats) for such a call: the whole call where it fits 64 MiB (one STFT launch and one band launch),
 * otherwise 64 MiB worth of whole workgroup steps (chunks that stay inside the GPU's 256 MiB Infinity Cache).  < 0: error. */
JSG_API int64_t jsg_stft_fb_scratch_floats(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* args, int n_batches);
/* The STFT kernel every chunk of such a call takes ("Cfg1024", "Cfg2048B", ...; out_len >= 24). */
JSG_API int jsg_stft_fb_kernel_name(const jsg_plan* plan, const jsg_filterbank* fb, const jsg_stft_args* args, int n_batches, char* out, int out_len);
/* How the band kernel of one chunk is launched (host arithmetic only: no device, no objects; the launcher takes its numbers from the
 * same routine).  A chunk of n_cols power columns (batches x rows x frames) of an n-point plan, a bank of n_bands bands and nnz weights,
 * a device of n_cu compute units:
 *   tile_cols    power columns per LDS tile: 8 (n <= 2048), 4 (4096), 2 (8192)
 *   bank_in_lds  1 where descriptors and weights, 3 n_bands + nnz words, fit 28 KB and are staged in LDS; 0: read through the caches
 *   pw_pitch     floats per power column in scratch: n/2 + 1 rounded up to whole 128-byte lines
 *   lds_bytes    4 tile_cols pw_pitch, plus 4 (3 n_bands + nnz) where the bank is in LDS
 *   grid         workgroups: max(1, min(ceil(n_cols / tile_cols), n_cu min(8, 163840 / lds_bytes))); a workgroup takes the tiles
 *                blockIdx, blockIdx + grid, ...
 * Any output pointer may be NULL.  JSG_ERR_INVALID: n not a power of two in 512..8192, n_bands outside 1..JSG_FB_MAX_BANDS, nnz outside
 * 0..2^31-1, n_cols outside 1..2^28, n_cu < 1. */
JSG_API int jsg_fb_band_plan(int n, int n_bands, int64_t nnz, int64_t n_cols, int n_cu, int32_t* tile_cols, int32_t* bank_in_lds,
                             int32_t* pw_pitch, int32_t* lds_bytes, int32_t* grid);

/* ------------------------------------------------------------------------------------------------
 * 2c. Frequency axis of the colour loop: `height` image rows on a linear, log or mel axis, drawn from the dB columns the ring
 *     already holds (the reference draws one row per bin and zooms by blitting a sub-rectangle, Spectrogram.cpp:441-459).
 *
 *     Row table (jsg_freq_axis_build, host, double arithmetic; row r = 0 is the BOTTOM row, H = height):
 *         w(f) = f (LINEAR), ln f (LOG), Slaney mel (MEL: the formula of the MEL_SLANEY filterbank), du = (w(fmax) - w(fmin)) / (H-1)
 *         centre_hz[r] = w^-1(w(fmin) + r du)
 *         b_j = w^-1(w(fmin) + (j - 1/2) du) * n / fs,  j = 0..H  (each bound computed once: row r = [b_r, b_r+1), the rows
 *               partition the bin axis)
 *         the bins of row r are the integers k in [0, n/2] with b_r <= k < b_r+1:
 *           at least one: first_bin[r] = the first of them, n_bins[r] = their count (interp_t[r] = 0);
 *           none:         n_bins[r] = 0, x = centre_hz[r] n / fs (double centre), k = min(floor(x), n/2-1),
 *                         first_bin[r] = k, interp_t[r] = (float)(x - k).
 *     LINEAR over [0, fs/2] with H = n/2+1 is the identity: row r holds exactly bin r.
 *
 *     Pixel of dB column c, row r (float32, bit for bit):
 *         n_bins >= 1: v = max(db[c][first .. first+n_bins-1]); NaN if any of those values is NaN
 *         n_bins == 0: a = db[c][k], b = db[c][k+1], v = a + t (b - a), the subtraction, the product and the sum rounded
 *                      separately (no fused multiply-add)
 *         pixel(x, H-1-r) = lut[index(v)] | 0xFF000000 and index_out = index(v), index() as in jsg_colormap_launch (NaN: index 0).
 *     The maximum keeps a narrow tone visible in a row that spans many bins (a mean of dB would hide it).
 * ------------------------------------------------------------------------------------------------ */
typedef enum jsg_axis_scale { JSG_AXIS_BINS = 0, JSG_AXIS_LINEAR = 1, JSG_AXIS_LOG = 2, JSG_AXIS_MEL = 3 } jsg_axis_scale;
#define JSG_AXIS_MAX_HEIGHT 16384
typedef struct jsg_axis_spec {
    int32_t n;          /* FFT size: a power of two in 512..8192 */
    float fs;           /* sample rate, Hz (> 0) */
    int32_t scale;      /* LINEAR / LOG / MEL (BINS is the engine's default and is refused here) */
    int32_t height;     /* image rows, 2..JSG_AXIS_MAX_HEIGHT */
    float fmin, fmax;   /* Hz: 0 <= fmin < fmax <= fs/2 (LOG: fmin > 0) */
} jsg_axis_spec;
/* The row table of a spec, on the host (no GPU): first_bin, n_bins, interp_t, centre_hz of `height` entries each.
 * JSG_ERR_INVALID for a spec outside the ranges above. */
JSG_API int jsg_freq_axis_build(const jsg_axis_spec* s, int32_t* first_bin, int32_t* n_bins, float* interp_t, float* centre_hz);

/* The row table resident on the device that is current at creation (uploaded once, with the row tiles the kernel is launched over). */
typedef struct jsg_freq_axis jsg_freq_axis;
JSG_API int jsg_freq_axis_create(jsg_freq_axis** out, const jsg_axis_spec* s);
JSG_API int jsg_freq_axis_destroy(jsg_freq_axis* ax);
JSG_API int jsg_freq_axis_height(const jsg_freq_axis* ax);
/* jsg_colormap_launch with the rows of `ax`: args->height must be n/2+1 of the axis's FFT size (the bins of a dB column); the image
 * has jsg_freq_axis_height(ax) rows.  Every other argument keeps its meaning (ring wrap, x_first / x_wrap, argb_out and / or
 * index_out, any n_colors).  Enqueue only (hipGraph capture works).  Refused: everything jsg_colormap_launch refuses, an axis of
 * another device or of another FFT size. */
JSG_API int jsg_colormap_axis_launch(const jsg_colormap_args* args, const jsg_freq_axis* ax, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2d. Complex STFT and inverse STFT with any hop (no reference counterpart: the reference keeps only power).
 *
 *     Forward: frame j of row r reads n samples at in[r*in_pitch + j*hop + m], m < n, any hop in 1..n, and writes the n/2+1 bins
 *         X[r][j][k] = sum_{m<n} w[m] x[r][j*hop+m] exp(-2 pi i k m / n)        (numpy.fft.rfft(w * frame); no scaling)
 *     as interleaved float pairs (re, im) at out[2 * (r*out_row_pitch + j*out_frame_pitch + k)] (pitches in complex elements).
 *     Inverse (torch.istft's definition, frames at j*hop, no centring):
 *         y[r][t] = (sum_j w[t - j*hop] irfft(X[r][j])[t - j*hop]) / (sum_j w[t - j*hop]^2),   t < (n_frames-1)*hop + n,
 *     irfft dividing by n and ignoring the imaginary parts of bins 0 and n/2.  Each sample sums its frames in ascending j (no atomics,
 *     bit for bit the same whatever the chunking); the envelope is summed in double from w^2 (computed on the host, uploaded with the
 *     plan) and its reciprocal rounded to float32 once; y = 0 where the envelope is <= 1e-11 (only at the edges of a call that passes
 *     the NOLA check).
 * ------------------------------------------------------------------------------------------------ */
/* A plan: window, twiddle tables (double on the host, rounded to float once) and w^2, resident on the device that is current at
 * creation.  n: a power of two in 512..8192 (else JSG_ERR_UNSUPPORTED); a non-finite window is refused (JSG_ERR_INVALID). */
typedef struct jsg_cstft jsg_cstft;
JSG_API int jsg_cstft_create(jsg_cstft** out, int n, const float* window);
JSG_API int jsg_cstft_destroy(jsg_cstft* plan);
JSG_API int jsg_cstft_fft_size(const jsg_cstft* plan);

typedef struct jsg_cstft_args {
    const float* in;            /* device floats, rows of samples */
    int64_t in_pitch;           /* floats between rows (>= 0) */
    int32_t rows;               /* 1..65535, independent (no channel mix); all in one launch */
    int32_t hop;                /* 1..n */
    int64_t n_frames;           /* frames per row (0: nothing is enqueued) */
    int64_t in_samples;         /* floats of every row that may be read: a launch whose last frame would read past them is refused
                                   (and rows > 1 need in_pitch >= in_samples).  0: not checked */
    float* out;                 /* device complex bins, 8-byte aligned */
    int64_t out_frame_pitch;    /* complex elements between frames (>= n/2+1) */
    int64_t out_row_pitch;      /* complex elements between rows (rows > 1: >= (n_frames-1)*out_frame_pitch + n/2+1) */
} jsg_cstft_args;
/* Enqueue only: no allocation, no synchronisation; hipGraph capture works.  Refused (JSG_ERR_INVALID, nothing enqueued, jsg_last_error
 * set): null pointers, a plan of another device, hop outside 1..n, pitches smaller than above, a read past in_samples. */
JSG_API int jsg_cstft_launch(const jsg_cstft* plan, const jsg_cstft_args* args, void* stream);

/* NOLA on the host: *min_envelope = the smallest interior envelope, min over rho < hop of sum_{m = rho mod hop} w[m]^2 (double, then
 * rounded to float).  JSG_ERR_INVALID when it is <= 1e-11 (*min_envelope is still set); jsg_istft_launch refuses such a hop. */
JSG_API int jsg_istft_nola(int n, int hop, const float* window, float* min_envelope);

typedef struct jsg_istft_args {
    const float* in;            /* device complex bins (float pairs), 8-byte aligned */
    int64_t in_frame_pitch;     /* complex elements between frames (>= n/2+1) */
    int64_t in_row_pitch;       /* complex elements between rows (rows > 1: >= (n_frames-1)*in_frame_pitch + n/2+1) */
    int32_t rows;               /* 1..65535 */
    int32_t hop;                /* 1..n, passing jsg_istft_nola */
    int64_t n_frames;           /* 1..2^31-1 */
    float* out;                 /* device floats: y[r][t] at out[r*out_pitch + t], t < out_samples */
    int64_t out_pitch;          /* rows > 1: >= out_samples */
    int64_t out_samples;        /* 1..(n_frames-1)*hop + n */
} jsg_istft_args;
/* `scratch`: device floats, 16-byte aligned, layout private to the library.  The call runs in chunks of as many frames as scratch
 * holds; a chunk recomputes the floor((n-1)/hop) frames before it that overlap its first sample, so the output is bit-identical for
 * every accepted scratch size.  Refused (JSG_ERR_INVALID): everything jsg_cstft_launch refuses for its arguments, a hop that fails
 * NOLA, out_samples outside the range above, scratch smaller than rows * n * min(F, floor((n-1)/hop) + 1) floats (F = the frames
 * that reach out_samples).  All refusals are decided before anything is enqueued.  Enqueue only; hipGraph capture works. */
JSG_API int jsg_istft_launch(const jsg_cstft* plan, const jsg_istft_args* args, float* scratch, int64_t scratch_floats, void* stream);
/* A recommended scratch size (floats): the whole call where it fits 64 MiB, otherwise 64 MiB worth of frames (at least the minimum
 * above).  < 0: the call would be refused. */
JSG_API int64_t jsg_istft_scratch_floats(const jsg_cstft* plan, const jsg_istft_args* args);

/* ------------------------------------------------------------------------------------------------
 * 2e. Phase vocoder (time stretch between jsg_cstft_launch and jsg_istft_launch; torchaudio.functional.phase_vocoder's formula).
 *
 *     Input X[r][j][k], complex64, frame-major with the pitches of section 2d: T frames of K = n/2+1 bins, taken with hop `hop` and
 *     FFT size n.  Output frame i sits at time t_i = (double)i * rate (one IEEE multiply); there are T_out = #{i >= 0 : t_i < T} of
 *     them (jsg_pvoc_frames).  With j = floor(t_i), alpha = (float)(t_i - j), a0 = X[j], a1 = X[j+1] (frames at index >= T are zero):
 *         mag_i = alpha |a1| + (1 - alpha) |a0|                                   (float32)
 *         d_i   = wrap(arg a1 - arg a0 - A_k) + A_k,  A_k = 2 pi hop k / n,  wrap(x) = x - 2 pi round(x / 2 pi)
 *         phi_0 = arg X[0],  phi_i = phi_(i-1) + d_(i-1)
 *         Y[r][i][k] = mag_i (cos phi_i, sin phi_i)
 *     The phase arithmetic is exact by construction.  Only phi mod 2 pi matters, so the library works in turns: the advance is
 *     frac(hop k / n), taken from the integer (hop k) mod n in double; (arg a1 - arg a0) is a float32 difference times the float32
 *     1 / (2 pi), widened to double; the advance is subtracted, round() of the result is subtracted, the advance is added back; the
 *     increment becomes fixed point with llrint(u * 2^32) and is accumulated in uint32_t with its natural wrap-around (2^32 units are
 *     one turn); phi_0 is converted the same way.  sincosf receives (float)(int32_t)acc * (2 pi / 2^32).  Integer addition is
 *     associative, so every chunk length, grid, row count and pitch gives the same bits, and a large hop * k causes no drift
 *     however long the input.  atan2f and sincosf are the device library's, so there is no bit-exact CPU mirror: the contract is a
 *     tolerance against a float64 evaluation of the formulas above.
 * ------------------------------------------------------------------------------------------------ */
/* T_out for T = n_frames_in (1..2^31-1) and a finite rate > 0.  JSG_ERR_INVALID for other arguments or a T_out above 2^31-1. */
JSG_API int64_t jsg_pvoc_frames(int64_t n_frames_in, double rate);

typedef struct jsg_pvoc_args {
    const float* in;            /* device complex bins (float pairs), 8-byte aligned */
    int64_t in_frame_pitch;     /* complex elements between frames (>= n/2+1) */
    int64_t in_row_pitch;       /* complex elements between rows (rows > 1: >= (n_frames_in-1)*in_frame_pitch + n/2+1) */
    int32_t rows;               /* 1..65535 */
    int32_t n;                  /* FFT size of the frames: any even number in 2..65536 (no transform is done here) */
    int32_t hop;                /* analysis hop, 1..n */
    int64_t n_frames_in;        /* T, 1..2^31-1 */
    double rate;                /* finite, > 0; > 1 shortens */
    float* out;                 /* device complex bins, 8-byte aligned, not overlapping `in` */
    int64_t out_frame_pitch;    /* >= n/2+1; elements between the bins of two frames are not written */
    int64_t out_row_pitch;      /* rows > 1: >= (n_frames_out-1)*out_frame_pitch + n/2+1 */
    int64_t n_frames_out;       /* must equal jsg_pvoc_frames(n_frames_in, rate) */
    int32_t chunk_frames;       /* output frames per chunk: 0 = the library's choice, else 1..65536; the result does not depend on it */
} jsg_pvoc_args;
/* Bytes of scratch the call needs (4 bytes per row, chunk and bin, rounded up to 16).  < 0: the call would be refused.  Needs no device. */
JSG_API int64_t jsg_pvoc_scratch_bytes(const jsg_pvoc_args* args);
/* Enqueue only (three kernels: chunk sums, their prefixes, the output): no allocation, no synchronisation; hipGraph capture works.
 * `scratch`: device memory, 16-byte aligned, layout private to the library.  Refused (JSG_ERR_INVALID, nothing enqueued,
 * jsg_last_error set): null pointers, in or out not 8-byte aligned, n, hop, rows, n_frames_in or chunk_frames outside their ranges,
 * a rate that is not finite or <= 0, a T_out above 2^31-1, n_frames_out != T_out, pitches smaller than above, out overlapping in,
 * scratch that is null, not 16-byte aligned or smaller than jsg_pvoc_scratch_bytes.  JSG_ERR_NO_DEVICE without a HIP device. */
JSG_API int jsg_pvoc_launch(const jsg_pvoc_args* args, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2f. Harmonic-percussive separation by median filtering (on the frames of jsg_cstft_launch, or on a power plane such as the
 *     ring of linear_out = 1).  This is librosa.decompose.hpss(|X|, kernel_size=(W_f, W_t), power=2, margin=(margin_h, margin_p),
 *     mask=True) and the masked input: the median commutes with squaring, so the whole operation is stated on float32 power.
 *
 *     Input in[r][j][k], frame-major, complex64 (in_complex = 1) or real power (in_complex = 0); T frames of K bins.  All values
 *     are float32, every operation is rounded separately, there is no fused multiply-add:
 *         P[j][k]  = re*re + im*im                      (real input: P = in)
 *         refl(i,L): m = i mod 2L (non-negative);  m < L ? m : 2L-1-m        (scipy's "reflect", any distance past the edge)
 *         H[j][k]  = the (h_t+1)-th smallest of P[refl(j+d,T)][k], d = -h_t..h_t,   h_t = (W_t-1)/2
 *         C[j][k]  = the (h_f+1)-th smallest of P[j][refl(k+d,K)], d = -h_f..h_f,   h_f = (W_f-1)/2
 *         g_h = margin_h*margin_h,  g_p = margin_p*margin_p
 *         D_h = H + g_h*C;   M_h = D_h > 0 ? H / D_h : 0     (IEEE correctly rounded division)
 *         D_p = C + g_p*H;   M_p = D_p > 0 ? C / D_p : 0
 *         out_h = (M_h*re, M_h*im)   (real input: M_h*P);   out_p likewise;   mask_h = M_h, mask_p = M_p
 *     A numpy restatement therefore agrees bit for bit.  Covered: inputs whose powers and products are zero or normal floats
 *     (subnormal intermediates are outside the contract).  A NaN, an Inf or, for real input, a negative value at (j0, k0) is
 *     contained: it may change only outputs whose time window in column k0 or frequency window in frame j0 holds it; every other
 *     output keeps its bits, and nothing faults.  The bits do not depend on chunk_frames, the grid, the row count, the pitches or on
 *     which outputs are requested.  Elements between n_bins and a pitch are not written.
 * ------------------------------------------------------------------------------------------------ */
#define JSG_HPSS_MAX_WINDOW 63
typedef struct jsg_hpss_args {
    const float* in;             /* device; in_complex = 1: float pairs (re, im), 8-byte aligned; 0: real power values >= 0 */
    int32_t in_complex;
    int64_t in_frame_pitch;      /* elements (complex elements or floats) between frames, >= n_bins */
    int64_t in_row_pitch;        /* rows > 1: >= (n_frames-1)*in_frame_pitch + n_bins */
    int32_t rows;                /* 1..65535, independent */
    int32_t n_bins;              /* K, 1..32769 */
    int64_t n_frames;            /* T, 1..2^31-1 */
    int32_t win_time, win_freq;  /* odd, 1..JSG_HPSS_MAX_WINDOW: W_t filters along frames (harmonic), W_f along bins (percussive) */
    float margin_h, margin_p;    /* finite, >= 1 (librosa's margin) */
    float* out_h; float* out_p;  /* masked input, same kind as `in`; either may be NULL */
    int64_t out_frame_pitch, out_row_pitch;   /* as the input's; looked at only where out_h or out_p is given */
    float* mask_h; float* mask_p;/* float planes; either may be NULL.  At least one of the four outputs is non-NULL */
    int64_t mask_frame_pitch, mask_row_pitch; /* floats; looked at only where mask_h or mask_p is given */
    int32_t chunk_frames;        /* frames per work item along time: 0 = the library's choice, else 1..65536; never changes the result */
} jsg_hpss_args;
/* Bytes of scratch the call needs (one float per row, frame and bin: the frequency medians; rounded up to 16).  < 0: the call would
 * be refused.  Needs no device. */
JSG_API int64_t jsg_hpss_scratch_bytes(const jsg_hpss_args* args);
/* Enqueue only (two kernels: the medians along the bins to scratch, then the medians along the frames, the masks and the outputs):
 * no allocation, no synchronisation; hipGraph capture on one stream works.  `scratch`: device memory, 16-byte aligned, layout
 * private to the library.  Refused (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set, decided before any device call): null
 * args or input, all four outputs NULL, a window that is even or out of range, rows, n_bins, n_frames or chunk_frames out of range,
 * a margin that is not finite or below 1, a pitch below its minimum, a misaligned pointer, an output that overlaps the input or
 * another output, scratch that is null, not 16-byte aligned or smaller than jsg_hpss_scratch_bytes.  JSG_ERR_NO_DEVICE without a
 * HIP device, after these checks. */
JSG_API int jsg_hpss_launch(const jsg_hpss_args* args, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2g. Band-limited resampling by any real ratio (a windowed-sinc table read with linear interpolation; one table serves every ratio).
 *
 *     Table win[0..Z P], float32: Z zero crossings per wing, P entries per zero crossing (Z >= 1, P >= 1, Z P <= 32768), supplied by
 *     the caller (jsg_sinc_table_build makes the usual one).  delta[o] = win[o+1] - win[o], a float32 subtraction of the float32
 *     entries.  Rows x[r][0..L); step = input samples per output sample (sr_in / sr_out), finite, in [1/64, 64].  Output i sits at
 *     t_i = (double)i * step (one IEEE multiply); there are T = #{i >= 0 : t_i < L} outputs (jsg_resample_length; ceil(L new / orig)
 *     for a rational step).  The tap positions are fixed point, 2^32 units per table entry:
 *         scale = step > 1 ? 1 / step : 1                    (double, one division)
 *         S     = llrint(scale * P * 2^32)                   (int64: the table advance per input sample)
 *         n = floor(t_i),  f = t_i - n,  F_L = llrint(f * (double)S),  F_R = S - F_L
 *         left wing,  a = 0, 1, ...:  m = n - a,      pos = F_L + a S
 *         right wing, b = 0, 1, ...:  m = n + 1 + b,  pos = F_R + b S
 *         a tap is live iff  pos < (Z P) 2^32  and  0 <= m < L
 *         o = pos >> 32,  eta = (float)((pos & 0xffffffff) >> 8) * 2^-24         (exact in float32)
 *         w = fmaf(eta, delta[o], win[o])
 *         y[r][i] = (float)scale * sum over the live taps of w * x[r][m]
 *     The positions are integers, so every tap's weight is defined to the bit.  The library sums each wing in ascending a (b) with
 *     fmaf into an accumulator of its own, adds the two once and scales once; the order depends on i only, so the bits do not
 *     depend on chunk_outputs, the grid, the row count, the pitches or the alignment of the pointers.  The contract is a tolerance
 *     against a float64 evaluation of the formulas above.  Taps that are not live contribute nothing (they are not multiplied by
 *     zero): a NaN or an Inf at x[r][m0] changes exactly the outputs of row r that have a live tap at m0.
 * ------------------------------------------------------------------------------------------------ */
typedef struct jsg_resampler jsg_resampler;
/* Uploads `table` (num_zeros * per_zero + 1 host floats) to the current device.  Refused (JSG_ERR_INVALID): null pointers, Z or P out
 * of range, a table entry that is not finite.  JSG_ERR_NO_DEVICE without a HIP device, after these checks. */
JSG_API int jsg_resampler_create(jsg_resampler** out, int num_zeros, int per_zero, const float* table);
JSG_API int jsg_resampler_destroy(jsg_resampler* rs);
JSG_API int jsg_resampler_zeros(const jsg_resampler* rs);
JSG_API int jsg_resampler_per_zero(const jsg_resampler* rs);
/* T for L = in_samples (1..2^31-1) and a finite step in [1/64, 64].  JSG_ERR_INVALID for other arguments.  Needs no device. */
JSG_API int64_t jsg_resample_length(int64_t in_samples, double step);

typedef struct jsg_resample_args {
    const float* in;            /* device floats: x[r][m] at in[r*in_pitch + m] */
    int64_t in_pitch;           /* rows > 1: >= in_samples */
    int32_t rows;               /* 1..65535, independent */
    int64_t in_samples;         /* L, 1..2^31-1 */
    double step;                /* finite, in [1/64, 64]; > 1 lowers the sample rate */
    float* out;                 /* device floats: y[r][i] at out[r*out_pitch + i]; elements from out_samples to the pitch are not written */
    int64_t out_pitch;          /* rows > 1: >= out_samples */
    int64_t out_samples;        /* must equal jsg_resample_length(in_samples, step) */
    int32_t chunk_outputs;      /* consecutive outputs per work item: 0 = the library's choice, else 1..65536; never changes the result */
} jsg_resample_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works.  Refused (JSG_ERR_INVALID, nothing
 * enqueued, jsg_last_error set, decided before any device call): null pointers, in or out not 4-byte aligned, a step that is not
 * finite or outside [1/64, 64], rows, in_samples or chunk_outputs out of range, out_samples != jsg_resample_length, a pitch below
 * in_samples / out_samples when rows > 1, out overlapping in.  Then JSG_ERR_NO_DEVICE without a HIP device, and JSG_ERR_INVALID for
 * a plan of another device (asking for the current device is the first device call).  Every table and step that pass these checks
 * are served: see the paths of jsg_resample_plan. */
JSG_API int jsg_resample_launch(const jsg_resampler* rs, const jsg_resample_args* args, void* stream);
/* What the launch would do for a table of num_zeros x per_zero and these arguments, without a plan and without a device: the path
 * as text (name may be NULL, else name_len >= 24), the outputs a pass takes and the bytes of LDS a workgroup asks for (either may be
 * NULL).  The paths: "resample_lds" (table and input span in LDS), "resample_l2" (the table does not fit beside the span of 256
 * outputs and is read through L2), "resample_direct" (not even the whole LDS holds that span: a table with many zero crossings at a
 * large step; only the table is staged, the input is read through L2).  Every accepted call has pass_outputs >= 1 and lds_bytes <=
 * 163840.  Refused: what the launch refuses for `args`, and table sizes jsg_resampler_create refuses. */
JSG_API int jsg_resample_plan(int num_zeros, int per_zero, const jsg_resample_args* args, char* name, int name_len, int32_t* pass_outputs,
                              int32_t* lds_bytes);
/* The path of jsg_resample_plan for the sizes of `rs` (out_len >= 24).  The argument refusals of the launch; then only the sizes of
 * the plan are read: no device is needed and the plan's device is not looked at. */
JSG_API int jsg_resample_kernel_name(const jsg_resampler* rs, const jsg_resample_args* args, char* out, int out_len);

/* ------------------------------------------------------------------------------------------------
 * 2h. Constant-Q and variable-Q spectrograms by direct evaluation in the time domain (one inner product per bin and frame; any
 *     fmin, any hop; no FFT, no resampling chain).
 *
 *     A basis is K bins.  Bin k has a half length h_k >= 0 and N_k = 2 h_k + 1 complex float32 taps c_k[m], m = -h_k..h_k, stored
 *     contiguously (re, im) from complex element offset[k] = sum of N_j over j < k (CSR as in section 2b).  For rows x[r][0..L),
 *     hop >= 1 and frames t = 0..T-1 centred on sample t * hop (int64 arithmetic):
 *         C[r][t][k] = sum over the live taps of  x[r][t*hop + m] * c_k[m]
 *         a tap is live iff  0 <= t*hop + m < L
 *     a real-by-complex product per tap, accumulated in float32 for re and im separately.  Taps that are not live are never
 *     touched (they are not multiplied by zero): a NaN or an Inf at x[r][m0] changes exactly the (t, k) of row r with
 *     |m0 - t*hop| <= h_k.  Frames past the signal are sums of no taps: +0.
 *
 *     The order of the float32 sum depends on k and on the tap index i = m + h_k alone.  With W_k = 64 where N_k > 32, else the
 *     smallest power of two >= N_k: lane l of W_k takes the live taps i = l, l + W_k, l + 2 W_k, ... in ascending order,
 *         acc_l = fmaf(x, c.re, acc_l)  (and the same for im),  acc_l = +0 at the start,
 *     then a fixed halving tree: for s = W_k/2, W_k/4, ..., 1: acc_l = acc_l + acc_(l+s) for l < s; the result is acc_0.  The bits
 *     therefore do not depend on t, r, L, chunk_frames, the grid, the row count, the pitches or the alignment of the pointers, and
 *     an interior frame of a signal delayed by one hop has the bits of the previous frame of the undelayed signal.  The contract
 *     is a tolerance against the float64 evaluation of the formula above on the float32 taps.
 *
 *     Output is frame-major: out_power = 0 writes float pairs (re, im) at out[(r*out_row_pitch + t*out_frame_pitch + k)] (pitches in
 *     complex elements); out_power = 1 writes re*re + im*im (both products and the sum rounded separately, no fused multiply-add;
 *     pitches in floats), the plane that jsg_db_from_power_launch, jsg_colormap_launch (height = K) and jsg_hpss_launch
 *     (in_complex = 0) take.  Elements between K and the frame pitch are not written.
 *
 *     The standard basis (jsg_cqt_basis_build; all arithmetic in double, each tap component rounded to float32 once):
 *         r = 2^(1/B),  alpha = (r^2 - 1) / (r^2 + 1),  Q = filter_scale / alpha,  f_k = fmin * 2^(k/B)
 *         l_k = Q * fs / (f_k + gamma / alpha)          (gamma = 0: constant-Q; gamma > 0: variable-Q)
 *         h_k = floor(l_k / 2)
 *         g[m] = 1/2 + 1/2 cos(pi m / (h_k + 1)),  normalised to sum g = 1,  times sqrt(l_k) if scale is set
 *         c_k[m] = g[m] * (cos phi, -sin phi),  phi = 2 pi frac(f_k * m / fs),  frac(u) = u - floor(u)
 *     the shape of librosa's wavelet / cqt / vqt (the same alpha, Q and lengths, an L1-normalised Hann, the sqrt-length scale) on a
 *     symmetric support of odd length; agreement with librosa has not been measured.
 * ------------------------------------------------------------------------------------------------ */
#define JSG_CQT_MAX_BINS 4096
#define JSG_CQT_MAX_HALF_LEN 131072
#define JSG_CQT_MAX_TAPS 16777216       /* sum of N_k */
#define JSG_CQT_MAX_CLASSES 20
typedef struct jsg_cqt_spec {
    double fs;                  /* sample rate, finite, > 0 */
    double fmin;                /* centre of bin 0, finite, > 0 */
    int32_t n_bins;             /* K, 1..JSG_CQT_MAX_BINS */
    int32_t bins_per_octave;    /* B, 1..1200 */
    double filter_scale;        /* finite, > 0 */
    double gamma;               /* finite, >= 0 */
    int32_t scale;              /* != 0: taps times sqrt(l_k) */
} jsg_cqt_spec;
/* The standard basis on the host (no device): half_len[K], offset[K] (complex elements), centre_hz[K] (any of the three may be NULL),
 * taps[2 * n_taps] floats (re, im).  taps == NULL only counts: *n_taps = sum of N_k.  Refused (JSG_ERR_INVALID): a null spec or
 * n_taps, fs, fmin, filter_scale or gamma out of range, n_bins or bins_per_octave out of range, f_(K-1) * (1 + alpha / 2) > fs / 2,
 * an h_k above JSG_CQT_MAX_HALF_LEN, sum N_k above JSG_CQT_MAX_TAPS, taps_cap (complex elements) below sum N_k. */
JSG_API int jsg_cqt_basis_build(const jsg_cqt_spec* spec, int32_t* half_len, int64_t* offset, float* centre_hz, float* taps,
                                int64_t taps_cap, int64_t* n_taps);

typedef struct jsg_cqt jsg_cqt;
/* Builds the standard basis and uploads it to the current device; the kernel's dynamic LDS limit is set here, so that a first
 * launch may sit inside a graph capture.  Refused: what jsg_cqt_basis_build refuses.  Then JSG_ERR_NO_DEVICE without a HIP device. */
JSG_API int jsg_cqt_create(jsg_cqt** out, const jsg_cqt_spec* spec);
/* The same for a caller's basis: n_bins half lengths and sum N_k complex taps (host memory).  Refused: null pointers, n_bins outside
 * 1..JSG_CQT_MAX_BINS, an h_k outside 0..JSG_CQT_MAX_HALF_LEN, sum N_k above JSG_CQT_MAX_TAPS.  Then JSG_ERR_NO_DEVICE. */
JSG_API int jsg_cqt_create_tables(jsg_cqt** out, int n_bins, const int32_t* half_len, const float* taps);
JSG_API int jsg_cqt_destroy(jsg_cqt* cq);
JSG_API int jsg_cqt_bins(const jsg_cqt* cq);
JSG_API int jsg_cqt_half_len(const jsg_cqt* cq, int32_t* out);     /* n_bins entries */
JSG_API int64_t jsg_cqt_total_taps(const jsg_cqt* cq);
/* 1 + floor(L / hop) for L in 1..2^31-1 and hop in 1..2^20 (JSG_ERR_INVALID otherwise): the frames whose centre lies in 0..L.  The
 * launch takes any T >= 1. */
JSG_API int64_t jsg_cqt_frames(int64_t in_samples, int64_t hop);

typedef struct jsg_cqt_args {
    const float* in;            /* device floats: x[r][m] at in[r*in_pitch + m] */
    int64_t in_pitch;           /* rows > 1: >= in_samples */
    int32_t rows;               /* 1..65535, independent */
    int64_t in_samples;         /* L, 1..2^31-1 */
    int64_t hop;                /* 1..2^20 */
    int64_t n_frames;           /* T, 1..2^31-1 */
    void* out;                  /* device; out_power = 0: float pairs, 8-byte aligned; 1: floats, 4-byte aligned */
    int64_t out_frame_pitch;    /* elements (complex elements or floats) between frames, >= K */
    int64_t out_row_pitch;      /* rows > 1: >= (T-1)*out_frame_pitch + K */
    int32_t out_power;          /* 0 or 1 */
    int32_t chunk_frames;       /* upper bound on the frames per work item: 0 = the library's choice, else 1..65536; never changes the result */
} jsg_cqt_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused
 * (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set), in this order and before any device call: a null basis, null args, a null
 * data pointer, out_power other than 0 or 1, a misaligned pointer, rows outside 1..65535, in_samples outside 1..2^31-1, hop outside
 * 1..2^20, n_frames outside 1..2^31-1, chunk_frames outside 0 or 1..65536, in_pitch below in_samples (rows > 1).  Then
 * JSG_ERR_NO_DEVICE without a HIP device (asking for the current device is the first device call; the basis is read only after it).
 * Then, still with nothing enqueued: out_frame_pitch below K, out_row_pitch below (T-1)*out_frame_pitch + K (rows > 1), out
 * overlapping in, a basis of another device.  jsg_cqt_plan and jsg_cqt_kernel_name decide all of these without a device.  Every basis
 * and call that pass are served: see the paths of jsg_cqt_plan. */
JSG_API int jsg_cqt_launch(const jsg_cqt* cq, const jsg_cqt_args* args, void* stream);
/* What the launch would do for a basis of these half lengths, without a basis object and without a device.  Bins are served in
 * classes by length: class c holds the bins with 2^(c-1) < N_k <= 2^c (class 0: N_k = 1); the classes that hold bins are reported
 * longest first: *n_classes of them (<= JSG_CQT_MAX_CLASSES) in the arrays class_max_taps (the largest N_k of the class),
 * frames_per_item (frames a work item of the class takes: one staging of the input into LDS), taps_per_pass (taps of a bin that are
 * staged at a time: < class_max_taps only on the "cqt_passes" path) and lds_bytes (of the class; a workgroup asks for the largest).
 * Any output pointer may be NULL (name: else name_len >= 24).  The paths: "cqt_span" (every bin's taps are staged in one pass) and
 * "cqt_passes" (a class with N_k > 12288 walks its taps in passes of 12288, the lane accumulators kept across the passes, so the
 * order of the sum is the same).  Every accepted call has frames_per_item >= 1, taps_per_pass >= 1 and lds_bytes <= 163840.
 * Refused: what the launch refuses for `args`, and what jsg_cqt_create_tables refuses for n_bins and half_len. */
JSG_API int jsg_cqt_plan(int n_bins, const int32_t* half_len, const jsg_cqt_args* args, char* name, int name_len, int32_t* n_classes,
                         int32_t* class_max_taps, int32_t* frames_per_item, int32_t* taps_per_pass, int32_t* lds_bytes);
/* The path of jsg_cqt_plan for the basis `cq` (out_len >= 24).  The argument refusals of the launch; no device is needed. */
JSG_API int jsg_cqt_kernel_name(const jsg_cqt* cq, const jsg_cqt_args* args, char* out, int out_len);

/* ------------------------------------------------------------------------------------------------
 * 2i. YIN fundamental-frequency tracking (de Cheveigne and Kawahara 2002), the difference function evaluated directly in the time
 *     domain (their eq. 6: a sum of non-negative terms, no autocorrelation by FFT, so nothing cancels where a voiced frame dips).
 *
 *     Rows x[r][0..L), a window w, lags tau_min <= tau_max, hop >= 1.  Frame t covers x[t*hop .. t*hop + w + tau_max); there are
 *     jsg_yin_frames(L, w, tau_max, hop) = 1 + (L - w - tau_max) / hop of them for L >= w + tau_max, else 0: no frame reaches outside
 *     its row, and a launch reads nothing outside the spans of its frames.  Per frame, with x[j] = x[r][t*hop + j], all in float32:
 *
 *     1. d[0] = 0;  d[tau] = sum over j = 0..w-1 of (x[j] - x[j+tau])^2  for tau = 1..tau_max.  The order of the sum depends on w and
 *        j alone: one accumulator per lag, acc = +0, and for jb = 0, 512, 1024, ...: for j0 = 0..63: for jj = 0..7:
 *            j = jb + j0 + 64 jj;  if j < w:  e = x[j] - x[j+tau];  acc = fmaf(e, e, acc)
 *        (j ascends by 64 inside a block of 512, the blocks and the j0 ascend outside; for w <= 64 this is j = 0, 1, ..., w-1).
 *     2. S[tau] = the running sum of d[1..tau], in groups of 64 lags: with tau = 1 + 64 c + l, l = 0..63 (d = +0 past tau_max), the
 *        group is scanned in place by v_l = v_l + v_(l-s) for l >= s, for s = 1, 2, 4, 8, 16, 32 in turn (all l at once per s), then
 *        S[tau] = carry + v_l with carry = +0 for c = 0 and carry = S[64 c] (the last S of the group before) otherwise.
 *        d'[0] = 1;  d'[tau] = (d[tau] * (float)tau) / S[tau], the product rounded, the divide correctly rounded;  d'[tau] = 1 where
 *        S[tau] == 0.
 *     3. tau = the smallest lag in tau_min..tau_max with d'[tau] < threshold (strict); from there tau += 1 while tau + 1 <= tau_max and
 *        d'[tau+1] < d'[tau].  If no lag is below the threshold: the lag of the minimum of d' over tau_min..tau_max, the lowest on ties.
 *     4. If tau + 1 <= tau_max: a, b, c = d'[tau-1], d'[tau], d'[tau+1];  den = (a - b) + (c - b);  if den > 0:
 *        s = (0.5f * (a - c)) / den, kept if |s| <= 1, else 0.  In every other case s = 0.  period = (float)tau + s.
 *     5. f0[r][t] = sample_rate / period at f0[r*out_pitch + t], aper[r][t] = d'[tau] at aper[r*out_pitch + t],
 *        cmnd[r][t][0..tau_max] = d' at cmnd[r*cmnd_row_pitch + t*cmnd_frame_pitch + tau] (a [frames][lags] plane as in section 2h: what
 *        jsg_db_from_power_launch and jsg_colormap_launch (height = tau_max + 1) take).  Any of the three may be NULL, not all.  Elements
 *        between tau_max + 1 and the frame pitch are not written.  Voicing is the caller's aper < threshold.
 *     6. If any d'[tau], tau in tau_min..tau_max, is NaN, f0 and aper of that frame are NaN (a NaN sample does this to exactly the
 *        frames whose span holds it; no other frame is touched).  A silent frame has d' = 1 everywhere: tau = tau_min, s = 0,
 *        f0 = sample_rate / (float)tau_min, aper = 1.
 *
 *     The bits do not depend on t, r, L, the hop, chunk_frames, the grid, the row count, the pitches or which outputs are NULL.  The
 *     contract for d' is a relative tolerance against the float64 evaluation: (2w + tau + 12) 2^-24 d'[tau].  librosa.yin integrates
 *     over a window of frame_length - tau_max samples too but takes the difference function from an FFT autocorrelation
 *     (r(0) + r_tau(0) - 2 r(tau)) and has other details of its own; agreement with it has not been measured.
 * ------------------------------------------------------------------------------------------------ */
#define JSG_YIN_MAX_WINDOW 8192
#define JSG_YIN_MAX_LAG 8192
/* 1 + (L - w - tau_max) / hop for L >= w + tau_max, else 0.  JSG_ERR_INVALID: in_samples outside 1..2^31-1, window outside
 * 1..JSG_YIN_MAX_WINDOW, tau_max outside 1..JSG_YIN_MAX_LAG, hop outside 1..2^20. */
JSG_API int64_t jsg_yin_frames(int64_t in_samples, int32_t window, int32_t tau_max, int64_t hop);

typedef struct jsg_yin_args {
    const float* in;            /* device floats: x[r][m] at in[r*in_pitch + m] */
    int64_t in_pitch;           /* rows > 1: >= in_samples */
    int32_t rows;               /* 1..65535, independent */
    int32_t window;             /* w, 1..JSG_YIN_MAX_WINDOW */
    int64_t in_samples;         /* L, 1..2^31-1 */
    int32_t tau_min;            /* 1..tau_max */
    int32_t tau_max;            /* 1..JSG_YIN_MAX_LAG */
    int64_t hop;                /* 1..2^20 */
    int64_t n_frames;           /* T, 1..jsg_yin_frames(in_samples, window, tau_max, hop) */
    float threshold;            /* finite, > 0 */
    float sample_rate;          /* finite, > 0 */
    float* f0;                  /* device floats or NULL */
    float* aper;                /* device floats or NULL */
    int64_t out_pitch;          /* of f0 and aper, rows > 1: >= n_frames */
    float* cmnd;                /* device floats or NULL */
    int64_t cmnd_frame_pitch;   /* floats between frames, >= tau_max + 1 */
    int64_t cmnd_row_pitch;     /* rows > 1: >= (T-1)*cmnd_frame_pitch + tau_max + 1 */
    int32_t chunk_frames;       /* upper bound on the frames per work item: 0 = the library's choice, else 1..65536; never changes the result */
} jsg_yin_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused
 * (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set), in this order and before any device call: null args, a null in, f0, aper
 * and cmnd all null, a pointer that is not 4-byte aligned, rows outside 1..65535, in_samples outside 1..2^31-1, window outside
 * 1..8192, tau_max outside 1..8192, tau_min outside 1..tau_max, hop outside 1..2^20, n_frames outside
 * 1..jsg_yin_frames(in_samples, window, tau_max, hop), chunk_frames outside 0 or 1..65536, a threshold that is not finite and > 0, a
 * sample_rate that is not finite and > 0, in_pitch below in_samples (rows > 1), out_pitch below n_frames (rows > 1, f0 or aper given),
 * cmnd_frame_pitch below tau_max + 1 (cmnd given), cmnd_row_pitch below (T-1)*cmnd_frame_pitch + tau_max + 1 (rows > 1, cmnd given),
 * an output overlapping in.  Then JSG_ERR_NO_DEVICE without a HIP device.  Every call that passes is served. */
JSG_API int jsg_yin_launch(const jsg_yin_args* args, void* stream);
/* What the launch would do, without a device: the path ("yin_lags1", "yin_lags2", "yin_lags4" or "yin_lags8": the lags a lane
 * accumulates at a time, by tau_max alone), the frames a work item takes (one staging of their span into LDS) and the bytes of LDS a
 * workgroup asks for (<= 163840).  Any output pointer may be NULL (name: else name_len >= 24).  Refused: what the launch refuses. */
JSG_API int jsg_yin_plan(const jsg_yin_args* args, char* name, int name_len, int32_t* frames_per_item, int32_t* lds_bytes);
/* The path of jsg_yin_plan (out_len >= 24).  The refusals of the launch; no device is needed. */
JSG_API int jsg_yin_kernel_name(const jsg_yin_args* args, char* out, int out_len);

/* ------------------------------------------------------------------------------------------------
 * 2j. Onset strength, autocorrelation tempogram and tempo: spectral flux of a [frames][bands] plane (what jsg_stft_fb_launch and
 *     the dB conversion write), the local autocorrelation of that envelope evaluated directly (no FFT), and the lag of the best
 *     tempo under a log-normal prior.  All arithmetic is float32; no sum depends on the row, the frame index, the number of rows or
 *     frames, the pitches, chunk_frames, the grid or which outputs are NULL.
 *
 *     Onset strength.  Rows S[r][t][b] at in[r*row_pitch + t*frame_pitch + b], t = 0..T-1, b = 0..B-1, a lag and a filter size m:
 *         ref[t][b] = the maximum of S[t][b'] over b' in [b - m/2, b + (m-1)/2] (integer division) clipped to [0, B), taken with
 *                     b' ascending by  mx = S[t][first b'];  then  mx = v  where  v > mx  or  v is NaN  (a NaN stays)
 *         e = S[t][b] - ref[t-lag][b];   p(b) = e where e > 0 or e is NaN, else +0       (fmaxf would drop the NaN)
 *         o[r][t] = (sum over b of p(b)) / (float)B  for t >= lag,  o[r][t] = +0 for t < lag (written too), at out[r*out_pitch + t]
 *     The order of the sum depends on B alone.  With W = 64 where B > 32, else the smallest power of two >= B: lane l of W adds
 *     b = l, l + W, l + 2W, ... ascending with plain adds from +0, then a halving tree: for s = W/2, W/4, ..., 1:
 *     acc_l = acc_l + acc_(l+s) for l < s; the sum is acc_0.  o[t] is NaN exactly when S[t] or S[t-lag] holds a NaN (for finite
 *     input otherwise); no other frame is touched, and nothing outside the T x B elements of a row is read.
 *
 *     Tempogram.  Rows o[r][t] at in[r*in_pitch + t], t = 0..T-1, a window table w[0..Wn), Lg lags, hop >= 1.  There are
 *     jsg_tempogram_frames(T, hop) = 1 + (T-1)/hop frames; frame i is centred on c = i*hop:
 *         y[j] = fl(o[c - Wn/2 + j] * w[j])  where 0 <= c - Wn/2 + j < T,  else +0  (nothing outside the row is read or multiplied)
 *         A[tau] = sum over j = 0..Wn-1-tau of y[j] * y[j+tau],  tau = 0..Lg-1
 *     one accumulator per lag, acc = +0, and for j = 0, 1, 2, ..., Wn-1-tau in this order:  acc = fmaf(y[j], y[j+tau], acc).
 *     Pairs past the window are left out, not multiplied by zero.
 *         normalise = 0:  TG[tau] = A[tau]
 *         normalise = 1:  TG[tau] = A[tau] / A[0], the divide correctly rounded;  +0 for every tau where A[0] == 0
 *     TG[r][i][tau] goes to out[r*row_pitch + i*frame_pitch + tau], a [frames][lags] plane as in sections 2h and 2i (what
 *     jsg_db_from_power_launch and jsg_colormap_launch with height = Lg take).  Elements between Lg and the frame pitch are not
 *     written.  A NaN at y[j0] makes, with normalise = 0, exactly the lags NaN whose sum pairs it (tau <= max(j0, Wn-1-j0)); with
 *     normalise = 1 the whole frame.  An all-zero window gives +0 everywhere.
 *     Against the same sums in float64 on the float32 products y, with u = 2^-24 and M[tau] = sum |y[j]| |y[j+tau]|:
 *         normalise = 0:  |TG - TG64| <= (Wn - tau + 4) u M[tau]            (one rounding per fmaf, Wn - tau of them; second order in the 4)
 *         normalise = 1:  |TG - TG64| <= ((Wn - tau + 4) M[tau] / A64[0] + (Wn + 8) |TG64|) u     (A[0] is a sum of non-negative terms:
 *                         its relative error is at most (Wn + 4) u; then the divide and the second-order terms)
 *
 *     Tempo.  A plane TG[r][i][tau], i = 0..N-1, tau = 0..Lg-1 (Lg >= 2), and a prior table of Lg floats:
 *         g[tau] = (sum over i of TG[i][tau]) / (float)N, the sum in blocks of 64 frames: P_k = the sum of the frames 64k .. 64k+63
 *                  below N, i ascending, plain adds from +0;  total = +0, then total = total + P_k for k ascending
 *         s[tau] = fl(fmaf(1e6f, g[tau], 1.0f) * prior[tau])
 *         tau* = the tau in 1..Lg-1 with the largest s, the lowest on ties (a NaN s never wins; tau* = 1 where none does)
 *         bpm[r] = fl(60.0f * frame_rate) / (float)tau*,  lag[r] = tau*,  profile[r][0..Lg) = g at profile[r*profile_pitch + tau]
 *     If any g[tau], tau >= 1, is NaN: bpm = NaN and lag = -1.  In exact arithmetic tau* is the argmax of log1p(1e6 g) + log prior,
 *     the rule of librosa.feature.tempo, so no logarithm runs on the device.  The standard prior (jsg_tempo_prior_build, in double,
 *     rounded to float32 once): prior[0] = 0;  prior[tau] = exp(-0.5 ((log2(60 frame_rate / tau) - log2(start_bpm)) / std_bpm)^2);
 *     prior[tau] = 0 where 60 frame_rate / tau > max_bpm (max_bpm <= 0: no limit).
 *
 *     These definitions differ from librosa.onset.onset_strength / librosa.feature.tempogram / librosa.feature.tempo on purpose: the
 *     envelope is not shifted by n_fft / (2 hop) frames for centring; the maximum filter is clipped at the band edges, not
 *     reflected; the envelope is taken as zero outside the row, where librosa pads with a linear ramp to zero; the autocorrelation
 *     is summed directly, not taken from an FFT of the padded frame.  Agreement with librosa has not been measured.
 * ------------------------------------------------------------------------------------------------ */
#define JSG_ONSET_MAX_BANDS 65536
#define JSG_ONSET_MAX_LAG 4096
#define JSG_ONSET_MAX_SIZE 255
#define JSG_TEMPOGRAM_MAX_WINDOW 4096
typedef struct jsg_onset_args {
    const float* in;            /* device floats: S[r][t][b] at in[r*row_pitch + t*frame_pitch + b] */
    int64_t frame_pitch;        /* floats between frames, >= n_bands */
    int64_t row_pitch;          /* rows > 1: >= (T-1)*frame_pitch + n_bands */
    int32_t rows;               /* 1..65535, independent */
    int32_t n_bands;            /* B, 1..JSG_ONSET_MAX_BANDS */
    int64_t n_frames;           /* T, 1..2^31-1 */
    int32_t lag;                /* 1..JSG_ONSET_MAX_LAG */
    int32_t max_size;           /* m, 1..JSG_ONSET_MAX_SIZE */
    float* out;                 /* device floats: o[r][t] at out[r*out_pitch + t] */
    int64_t out_pitch;          /* rows > 1: >= n_frames */
} jsg_onset_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused
 * (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set), in this order and before any device call: null args, a null in, a null
 * out, a pointer that is not 4-byte aligned, rows outside 1..65535, n_bands outside 1..65536, n_frames outside 1..2^31-1, lag
 * outside 1..4096, max_size outside 1..255, frame_pitch below n_bands, row_pitch below (T-1)*frame_pitch + n_bands (rows > 1),
 * out_pitch below n_frames (rows > 1), out overlapping in.  Then JSG_ERR_NO_DEVICE without a HIP device.  Every call that passes is
 * served. */
JSG_API int jsg_onset_strength_launch(const jsg_onset_args* args, void* stream);

/* 1 + (n_in - 1) / hop.  JSG_ERR_INVALID: n_in outside 1..2^31-1, hop outside 1..2^20. */
JSG_API int64_t jsg_tempogram_frames(int64_t n_in, int64_t hop);
typedef struct jsg_tempogram_args {
    const float* in;            /* device floats: o[r][t] at in[r*in_pitch + t] */
    int64_t in_pitch;           /* rows > 1: >= n_in */
    int32_t rows;               /* 1..65535, independent */
    int32_t win_length;         /* Wn, 2..JSG_TEMPOGRAM_MAX_WINDOW */
    int64_t n_in;               /* T, 1..2^31-1 */
    int64_t hop;                /* 1..2^20 */
    int64_t n_frames;           /* 1..jsg_tempogram_frames(n_in, hop) */
    int32_t lags;               /* Lg, 1..win_length */
    int32_t normalise;          /* 0 or 1 */
    const float* window;        /* device floats: w[0..Wn) */
    float* out;                 /* device floats: TG[r][i][tau] at out[r*row_pitch + i*frame_pitch + tau] */
    int64_t frame_pitch;        /* floats between frames, >= lags */
    int64_t row_pitch;          /* rows > 1: >= (n_frames-1)*frame_pitch + lags */
    int32_t chunk_frames;       /* upper bound on the frames per work item: 0 = the library's choice, else 1..65536; never changes the result */
} jsg_tempogram_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused
 * (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set), in this order and before any device call: null args, a null in, a null
 * window, a null out, a pointer that is not 4-byte aligned, rows outside 1..65535, n_in outside 1..2^31-1, win_length outside
 * 2..4096, lags outside 1..win_length, hop outside 1..2^20, n_frames outside 1..jsg_tempogram_frames(n_in, hop), normalise other than
 * 0 or 1, chunk_frames outside 0 or 1..65536, in_pitch below n_in (rows > 1), frame_pitch below lags, row_pitch below
 * (n_frames-1)*frame_pitch + lags (rows > 1), out overlapping in or window.  Then JSG_ERR_NO_DEVICE without a HIP device.  Every
 * call that passes is served. */
JSG_API int jsg_tempogram_launch(const jsg_tempogram_args* args, void* stream);
/* What the launch would do, without a device: the path ("tempogram_lags1", "tempogram_lags2", "tempogram_lags4" or
 * "tempogram_lags8": the lags a lane accumulates at a time, by `lags` alone), the frames a work item takes (one staging of their span
 * of the envelope and of the window into LDS) and the bytes of LDS a workgroup asks for (<= 163840).  Any output pointer may be NULL
 * (name: else name_len >= 24).  Refused: what the launch refuses. */
JSG_API int jsg_tempogram_plan(const jsg_tempogram_args* args, char* name, int name_len, int32_t* frames_per_item, int32_t* lds_bytes);
/* The path of jsg_tempogram_plan (out_len >= 24).  The refusals of the launch; no device is needed. */
JSG_API int jsg_tempogram_kernel_name(const jsg_tempogram_args* args, char* out, int out_len);

/* The standard prior on the host (no device): out[0..lags).  JSG_ERR_INVALID: a null out, lags outside 1..JSG_TEMPOGRAM_MAX_WINDOW,
 * frame_rate, start_bpm or std_bpm not finite and > 0, max_bpm not finite. */
JSG_API int jsg_tempo_prior_build(int32_t lags, double frame_rate, double start_bpm, double std_bpm, double max_bpm, float* out);
typedef struct jsg_tempo_args {
    const float* in;            /* device floats: TG[r][i][tau] at in[r*row_pitch + i*frame_pitch + tau] */
    int64_t frame_pitch;        /* floats between frames, >= lags */
    int64_t row_pitch;          /* rows > 1: >= (N-1)*frame_pitch + lags */
    int32_t rows;               /* 1..65535, independent */
    int32_t lags;               /* Lg, 2..JSG_TEMPOGRAM_MAX_WINDOW */
    int64_t n_frames;           /* N, 1..2^31-1 */
    float frame_rate;           /* frames of the envelope per second, finite, > 0 */
    const float* prior;         /* device floats: prior[0..Lg) */
    float* bpm;                 /* device floats [rows] or NULL */
    int32_t* lag;               /* device int32 [rows] or NULL */
    float* profile;             /* device floats or NULL: g[r][tau] at profile[r*profile_pitch + tau] */
    int64_t profile_pitch;      /* rows > 1: >= lags */
} jsg_tempo_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused
 * (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set), in this order and before any device call: null args, a null in, a null
 * prior, bpm, lag and profile all null, a pointer that is not 4-byte aligned, rows outside 1..65535, lags outside 2..4096, n_frames
 * outside 1..2^31-1, a frame_rate that is not finite and > 0, frame_pitch below lags, row_pitch below (N-1)*frame_pitch + lags
 * (rows > 1), profile_pitch below lags (rows > 1, profile given), an output overlapping in or prior.  Then JSG_ERR_NO_DEVICE without
 * a HIP device.  Every call that passes is served. */
JSG_API int jsg_tempo_launch(const jsg_tempo_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2k. Cepstral coefficients and delta features: a [frames][bands] plane (what jsg_stft_fb_launch and the dB conversion write)
 *     projected through a dense table (the DCT-II of MFCCs, its zero-padded inverse, or any table of yours), and the
 *     Savitzky-Golay derivative of a plane along its frames.  All device arithmetic is float32 (denormals kept, NaN and infinity as
 *     the fmaf chains give them, as in section 2j); no sum depends on the row, the frame index, the number of rows or frames, the
 *     pitches, chunk_frames, the grid or the path jsg_mfcc_plan names.
 *
 *     Projection.  Rows S[r][t][b] at in[r*row_pitch + t*frame_pitch + b], t = 0..T-1, b = 0..B-1 (B = n_in), and a table D[m][b]
 *     at table[m*B + b], m = 0..M-1 (M = n_out):
 *         C[r][t][m] = acc after  acc = +0;  for b = 0, 1, ..., B-1 in this order:  acc = fmaf(D[m][b], S[t][b], acc)
 *     at out[r*out_row_pitch + t*out_frame_pitch + m].  Elements between M and the frame pitch are not written.  A NaN or an
 *     infinity at S[t0][b0] reaches exactly the outputs of frame t0 of that row, as the chain gives them (a zero in the table does
 *     not stop a NaN); no other frame is touched, and nothing outside the T x B elements of a row is read.  Against the same sum in
 *     float64 of the exact products of the float32 operands, with u = 2^-24:
 *         |C - C64| <= (B + 2) u * sum over b of |D[m][b]| |S[t][b]|           (one rounding per fmaf; second order in the 2)
 *
 *     Tables (jsg_mfcc_table_build, on the host in double, rounded to float32 once).  k = m*(2b+1) mod 4B in integers,
 *     c = cos(pi*k / (2B)):
 *         forward, M x B, the DCT-II of scipy.fft.dct(type=2):  D[m][b] = 2c * s[m] * L[m]
 *             s[m] = 1 (JSG_DCT_NORM_NONE);  sqrt(1/(4B)) for m = 0, sqrt(1/(2B)) otherwise (JSG_DCT_NORM_ORTHO)
 *             L[m] = 1 + (lifter/2) * sin(pi*(m+1)/lifter),  1 for lifter 0      (the lifter of librosa.feature.mfcc, in the table)
 *         inverse, B x M in the layout of a launch with n_in = M, n_out = B: the zero-padded inverse of scipy.fft.idct(type=2, n=B)
 *             ortho:  I[b][m] = 2c * s[m] / L[m];     none:  I[b][m] = (m == 0 ? 1 : 2c) / (2B) / L[m]
 *
 *     Delta.  Rows X[r][t][m] with the pitches of a plane, M = n_coeffs values per frame, weights w[0..Wd), Wd odd, h = Wd/2:
 *         JSG_DELTA_EDGE_INTERP  (T >= Wd):  s = min(max(t - h, 0), T - Wd);  window j is frame s + j
 *         JSG_DELTA_EDGE_NEAREST (T >= 1):   window j is frame min(max(t - h + j, 0), T - 1)
 *         Y[r][t][m] = acc after  acc = +0;  for j = 0..Wd-1 in this order:  acc = fmaf(w[j], X[frame j][m], acc)
 *     With a polynomial order equal to the derivative order (what librosa.feature.delta passes to scipy.signal.savgol_filter) the
 *     derivative of the fit is constant over the window, so mode = 'interp' is the interior weights on the first or last Wd frames.
 *     A NaN at X[t0][m0] reaches exactly the frames whose window holds t0, in coefficient m0 only.
 *         |Y - Y64| <= (Wd + 2) u * sum over j of |w[j]| |X[frame j][m]|
 *     jsg_delta_weights_build: w = order! * row `order` of the pseudo-inverse of the Vandermonde matrix of j - h, in double, rounded
 *     once; the centre weight of an odd order is exactly 0; width 9, order 1 gives (j - 4) / 60.
 *
 *     Differences from librosa.feature.mfcc / delta / inverse.mfcc_to_mel, on purpose: the frames lie along axis -2 and the
 *     coefficients along the last axis; the mel dB plane of the Python layer is 10 log10(power + 1e-11) without top_db clipping or
 *     centring; the lifter is folded into the table before its one rounding.  Agreement with librosa has not been measured.
 * ------------------------------------------------------------------------------------------------ */
#define JSG_MFCC_MAX_BANDS 4096
#define JSG_MFCC_MAX_COEFFS 4096
#define JSG_MFCC_MAX_TABLE 32768        /* n_in * n_out floats (128 KB): the whole table sits in LDS next to the staged tile */
#define JSG_DCT_NORM_NONE 0
#define JSG_DCT_NORM_ORTHO 1
#define JSG_DELTA_MAX_WIDTH 255
#define JSG_DELTA_MAX_ORDER 4
#define JSG_DELTA_MAX_COEFFS 65536
#define JSG_DELTA_EDGE_INTERP 0
#define JSG_DELTA_EDGE_NEAREST 1
typedef struct jsg_mfcc_args {
    const float* in;            /* device floats: S[r][t][b] at in[r*row_pitch + t*frame_pitch + b] */
    int64_t frame_pitch;        /* floats between frames, >= n_in */
    int64_t row_pitch;          /* rows > 1: >= (T-1)*frame_pitch + n_in */
    int32_t rows;               /* 1..65535, independent */
    int32_t n_in;               /* B, 1..JSG_MFCC_MAX_BANDS */
    int64_t n_frames;           /* T, 1..2^31-1 */
    const float* table;         /* device floats: D[m][b] at table[m*n_in + b]; n_in*n_out <= JSG_MFCC_MAX_TABLE */
    int32_t n_out;              /* M, 1..JSG_MFCC_MAX_COEFFS */
    float* out;                 /* device floats: C[r][t][m] at out[r*out_row_pitch + t*out_frame_pitch + m] */
    int64_t out_frame_pitch;    /* floats between frames, >= n_out */
    int64_t out_row_pitch;      /* rows > 1: >= (T-1)*out_frame_pitch + n_out */
    int32_t chunk_frames;       /* upper bound on the frames per work item: 0 = the library's choice, else 1..65536; never changes the result */
} jsg_mfcc_args;
/* Applies any dense table (the inverse runs through it with the roles of B and M exchanged).  Enqueue only (one kernel, no scratch):
 * no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused (JSG_ERR_INVALID, nothing enqueued,
 * jsg_last_error set), in this order and before any device call: null args, a null in, a null table, a null out, a pointer that is
 * not 4-byte aligned, rows outside 1..65535, n_in outside 1..4096, n_out outside 1..4096, n_in*n_out above 32768, n_frames outside
 * 1..2^31-1, chunk_frames outside 0 or 1..65536, frame_pitch below n_in, row_pitch below (T-1)*frame_pitch + n_in (rows > 1),
 * out_frame_pitch below n_out, out_row_pitch below (T-1)*out_frame_pitch + n_out (rows > 1), out overlapping in or table.  Then
 * JSG_ERR_NO_DEVICE without a HIP device.  Every call that passes is served. */
JSG_API int jsg_mfcc_launch(const jsg_mfcc_args* args, void* stream);
/* What the launch would do, without a device: the path ("mfcc_block4", "mfcc_block5", "mfcc_block8", "mfcc_block10" or
 * "mfcc_block16": the coefficients a lane accumulates at a time, by n_out alone), the frames a work item takes (at most 64, one per
 * lane; fewer where chunk_frames, n_frames or the LDS next to a large table say so) and the bytes of LDS a workgroup asks for
 * (<= 163840: the table, the tile and the staged outputs).  Any output pointer may be NULL
 * (name: else name_len >= 24).  Refused: what the launch refuses. */
JSG_API int jsg_mfcc_plan(const jsg_mfcc_args* args, char* name, int name_len, int32_t* frames_per_item, int32_t* lds_bytes);
/* The path of jsg_mfcc_plan (out_len >= 24).  The refusals of the launch; no device is needed. */
JSG_API int jsg_mfcc_kernel_name(const jsg_mfcc_args* args, char* out, int out_len);
/* A DCT table on the host (no device): forward, out[n_coeffs][n_bands]; inverse, out[n_bands][n_coeffs].  JSG_ERR_INVALID, in this
 * order: a null out, n_bands outside 1..4096, n_coeffs outside 1..4096, n_coeffs above n_bands, n_bands*n_coeffs above 32768, norm
 * other than JSG_DCT_NORM_NONE or JSG_DCT_NORM_ORTHO, inverse other than 0 or 1, a lifter that is negative or not finite, an inverse
 * whose L[m] is zero for some m. */
JSG_API int jsg_mfcc_table_build(int32_t n_bands, int32_t n_coeffs, int32_t norm, double lifter, int32_t inverse, float* out);

/* The Savitzky-Golay derivative weights on the host (no device): out[0..width).  JSG_ERR_INVALID, in this order: a null out, a width
 * that is even or outside 3..255, an order outside 1..4 or not below width. */
JSG_API int jsg_delta_weights_build(int32_t width, int32_t order, float* out);
typedef struct jsg_delta_args {
    const float* in;            /* device floats: X[r][t][m] at in[r*row_pitch + t*frame_pitch + m] */
    int64_t frame_pitch;        /* floats between frames, >= n_coeffs */
    int64_t row_pitch;          /* rows > 1: >= (T-1)*frame_pitch + n_coeffs */
    int32_t rows;               /* 1..65535, independent */
    int32_t n_coeffs;           /* M, 1..JSG_DELTA_MAX_COEFFS */
    int64_t n_frames;           /* T, 1..2^31-1 */
    const float* weights;       /* device floats: w[0..width) */
    int32_t width;              /* Wd, odd, 3..JSG_DELTA_MAX_WIDTH */
    int32_t mode;               /* JSG_DELTA_EDGE_INTERP or JSG_DELTA_EDGE_NEAREST */
    float* out;                 /* device floats: Y[r][t][m] at out[r*out_row_pitch + t*out_frame_pitch + m] */
    int64_t out_frame_pitch;    /* floats between frames, >= n_coeffs */
    int64_t out_row_pitch;      /* rows > 1: >= (T-1)*out_frame_pitch + n_coeffs */
} jsg_delta_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused
 * (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set), in this order and before any device call: null args, a null in, a null
 * weights, a null out, a pointer that is not 4-byte aligned, rows outside 1..65535, n_coeffs outside 1..65536, n_frames outside
 * 1..2^31-1, a width that is even or outside 3..255, a mode other than the two, n_frames below width under JSG_DELTA_EDGE_INTERP,
 * frame_pitch below n_coeffs, row_pitch below (T-1)*frame_pitch + n_coeffs (rows > 1), out_frame_pitch below n_coeffs, out_row_pitch
 * below (T-1)*out_frame_pitch + n_coeffs (rows > 1), out overlapping in or weights.  Then JSG_ERR_NO_DEVICE without a HIP device.
 * Every call that passes is served. */
JSG_API int jsg_delta_launch(const jsg_delta_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 2l. Spectral shape descriptors: energy, centroid, spread, rolloff, flatness and crest of every frame of a [frames][bins] plane
 *     (the power plane of jsg_stft_db_launch with linear_out, a mel plane of jsg_stft_fb_launch, a power plane of jsg_cqt_launch),
 *     one kernel that reads the plane once and writes a few floats per frame.  All arithmetic is float32, denormals are kept; no
 *     result depends on the row, the frame index, the number of rows or frames, the pitches, the grid, the path
 *     jsg_spectral_shape_plan names or which outputs are NULL.
 *
 *     Input.  Rows S[r][t][k] at in[r*row_pitch + t*frame_pitch + k], t = 0..T-1, k = 0..K-1 (K = n_bins), and a table f[0..K) of
 *     frequencies (the Hz of FFT bins, mel or CQT centres, anything), the same for every row; roll_percent p in (0, 1].  S is
 *     non-negative; negative values are outside the contract, but even then nothing outside the T x K elements of a row and the K
 *     of the table is read, and no index leaves [0, K).
 *
 *     The lane sum (the rule of section 2j).  W = 64 where K > 32, else the smallest power of two >= K.  Lane l of W takes
 *     k = l, l + W, l + 2W, ... ascending, from acc_l = +0; then a halving tree: for s = W/2, W/4, ..., 1:
 *     acc_l = acc_l + acc_(l+s) for l < s; the sum is acc_0.  Per frame:
 *         E  = lane sum with  acc = acc + S[k]
 *         N1 = lane sum with  acc = fmaf(f[k], S[k], acc)
 *         mx = +0;  then  mx = v  where  v > mx  or  v is NaN  (a NaN stays; for non-NaN values the largest S[k], in any order)
 *         L  = lane sum with  acc = acc + dB(S[k])          (dB(p) = 10 log10(p + 1e-11f) by the shared routine jsg_exact_db of
 *                                                              csrc/jsg_exact_math.h: bit-reproducible on a CPU)
 *         centroid = N1 / E, the divide correctly rounded
 *         M2 = lane sum with  d = f[k] - centroid;  acc = fmaf(fl(d*d), S[k], acc)
 *         spread = sqrt(M2 / E), the divide and the square root correctly rounded      (librosa's spectral_bandwidth with p = 2)
 *         crest = mx / (E / (float)K)
 *         flatness_db = L / (float)K - dB(E / (float)K)     (10 log10 of geometric over arithmetic mean, the floor
 *                       1e-11f inside each logarithm; no exponential runs on the device, the linear value is 10^(flatness_db/10))
 *     Where E == 0: centroid, spread and crest are +0; flatness_db is what its chain gives.
 *
 *     Rolloff.  A prefix sum in a stated order, so that "the first bin" is defined.  Chunk j holds the W bins jW .. jW+W-1, bins
 *     past K count as +0.  Within a chunk, an inclusive scan: x_l = S[jW + l];  for s = 1, 2, 4, ..., W/2: every lane l >= s does
 *     x_l = x_l + x_(l-s), reading the values of the step before.  cum[jW + l] = base_j + x_l;  base_0 = +0,
 *     base_(j+1) = base_j + x_(W-1) of chunk j.
 *         thr = fl(p * cum[K-1]);   k* = the lowest k in [0, K) with cum[k] >= thr
 *         rolloff = f[k*],  rolloff_bin = k*
 *     k* is the first in ascending k: cum is not assumed to be monotone, and the bin is searched, not the frequency (f need not
 *     ascend).  For finite non-negative input k* exists, since thr <= cum[K-1]; where no k qualifies (possible only outside the
 *     contract) k* = K-1.  An all-zero frame gives k* = 0.
 *
 *     NaN and infinity.  A NaN at S[t0][k0] makes every float output of frame t0 of that row NaN and rolloff_bin -1, and touches
 *     no other frame: the sums carry it, mx keeps it by the rule above (a plain > would drop it), and for the rolloff: where thr
 *     is NaN (cum[K-1] carries every bin), rolloff = NaN and rolloff_bin = -1 (every comparison with a NaN is false).  A +inf
 *     gives what the chains give (energy +inf, centroid NaN from inf/inf, k* at the first infinite cum).
 *
 *     Outputs, each optional, each [rows][T] at out[r*out_pitch + t] with one shared out_pitch: energy (E), centroid, spread,
 *     rolloff, rolloff_bin (int32), flatness_db, crest.  A NULL output does not cost its separable work: without rolloff and
 *     rolloff_bin no scan runs, without flatness_db no logarithm, without spread no second pass, without centroid and spread no N1.
 *
 *     Against the same sums in float64 on the float32 inputs, with u = 2^-24, n = ceil(K/W) + log2 W (every term non-negative, so
 *     the bounds are relative; one rounding per add or fmaf, the first of a lane exact; products that do not underflow):
 *         |E - E64| <= (n + 1) u E64          |N1 - N164| <= (n + 1) u N164   (f >= 0)
 *         |centroid - centroid64| <= (2n + 4) u centroid64   (f >= 0: both sums and the divide)
 *     The spread is ill-conditioned where the spectrum is narrow (d = f - centroid cancels): no bound is given; its measured error
 *     is in profiles/spectral_accuracy.md.
 *
 *     Differences from librosa.feature.spectral_centroid / spectral_bandwidth / spectral_rolloff / spectral_flatness, on purpose:
 *     the plane is taken as it is (the Python layer's default is power, librosa's magnitude); the frames lie along axis -2; the
 *     floor inside the logarithms is 1e-11 (librosa: amin = 1e-10); no centring of frames.  Agreement with librosa has not been
 *     measured.
 * ------------------------------------------------------------------------------------------------ */
#define JSG_SPECTRAL_MAX_BINS 65536
typedef struct jsg_spectral_args {
    const float* in;            /* device floats: S[r][t][k] at in[r*row_pitch + t*frame_pitch + k] */
    int64_t frame_pitch;        /* floats between frames, >= n_bins */
    int64_t row_pitch;          /* rows > 1: >= (T-1)*frame_pitch + n_bins */
    int32_t rows;               /* 1..65535, independent */
    int32_t n_bins;             /* K, 1..JSG_SPECTRAL_MAX_BINS */
    int64_t n_frames;           /* T, 1..2^31-1 */
    const float* freqs;         /* device floats: f[0..K) */
    float roll_percent;         /* p, in (0, 1] */
    int32_t reserved0;          /* ignored */
    float* energy;              /* each output: device floats [rows][T] at out[r*out_pitch + t], or NULL */
    float* centroid;
    float* spread;
    float* rolloff;
    int32_t* rolloff_bin;       /* device int32, same layout, or NULL */
    float* flatness_db;
    float* crest;
    int64_t out_pitch;          /* rows > 1: >= n_frames; shared by all outputs */
} jsg_spectral_args;
/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; hipGraph capture works, a first launch included.  Refused
 * (JSG_ERR_INVALID, nothing enqueued, jsg_last_error set), in this order and before any device call: null args, a null in, a null
 * freqs, all outputs null, a pointer that is not 4-byte aligned, rows outside 1..65535, n_bins outside 1..65536, n_frames outside
 * 1..2^31-1, a roll_percent that is not in (0, 1] (NaN included), frame_pitch below n_bins, row_pitch below
 * (T-1)*frame_pitch + n_bins (rows > 1), out_pitch below n_frames (rows > 1), an output overlapping in or freqs.  Then
 * JSG_ERR_NO_DEVICE without a HIP device.  Every call that passes is served. */
JSG_API int jsg_spectral_shape_launch(const jsg_spectral_args* args, void* stream);
/* What the launch would do, without a device: the path, by n_bins alone -- "spectral_regs1", "spectral_regs2", "spectral_regs4",
 * "spectral_regs9", "spectral_regs17", "spectral_regs33" or "spectral_regs65": a lane keeps its ceil(K/W) values of a frame (at most
 * the number in the name: K <= 64 times it) in registers between the passes, so the plane crosses memory once; "spectral_stream"
 * (K > 4160): the second pass re-reads the frame through the caches -- the lanes that own a frame (W) and the frames a group of W
 * lanes has in flight at a time (a workgroup of 256 threads takes 256/W times as many consecutive frames per step of its grid
 * stride), and the bytes of LDS a workgroup asks for (0: the frequency table of the register paths sits in registers, loaded once
 * per workgroup).  Any output pointer may be NULL (name: else name_len >= 24).  Refused: what the launch refuses. */
JSG_API int jsg_spectral_shape_plan(const jsg_spectral_args* args, char* name, int name_len, int32_t* lanes_per_frame, int32_t* frames_per_group,
                                    int32_t* lds_bytes);
/* The path of jsg_spectral_shape_plan (out_len >= 24).  The refusals of the launch; no device is needed. */
JSG_API int jsg_spectral_shape_kernel_name(const jsg_spectral_args* args, char* out, int out_len);

/* ------------------------------------------------------------------------------------------------
 * 3. Engine: the state of class Spectrogram (Spectrogram.h:81-169) living on the GPU.
 * ------------------------------------------------------------------------------------------------ */
typedef struct jsg_engine jsg_engine;

/* Spectrogram::Spectrogram() defaults (Spectrogram.cpp:16-24): fs 48000, n 1024, feed 100 %, 1 s memory,
 * Hann, AbsMean.  `channels` is explicit (the plugin never calls setchannels). */
JSG_API int jsg_create(jsg_engine** out, int channels);
/* The same on an explicit HIP device (0 .. jsg_device_count()-1) instead of the calling thread's current one: what a
 * single-process host that drives several GPUs uses, one engine per device ("Several GPUs"). */
JSG_API int jsg_create_on_device(jsg_engine** out, int channels, int device);
JSG_API int jsg_get_device(const jsg_engine* e);
/* One engine per entry of `devices` (entries may repeat), the `channels` channels of one stream dealt out in contiguous runs
 * whose sizes differ by at most one: entry i owns [first_channel[i], first_channel[i] + channel_count[i]) and gets no engine
 * (out[i] = NULL) when that run is empty.  The engines share nothing -- the path shards by independent channels, there is no
 * collective (a cross-GPU AbsMean is the one exchange: INTEGRATION.md C).  Configure every engine with the usual setters.
 * jsg_process_block_sharded hands every engine its run of the planar pointers (enqueue only, wait-free) -- ALL OR NOTHING: if any
 * engine would not take the block now (its queue is full, it is in a geometry change, or its worker met an error) NO engine gets it,
 * every engine counts one dropped block and 1 is returned, so the rings of the shards keep the same position.  (A geometry setter of one
 * engine racing with the call is the one case that can still leave the set uneven: the caller changes the geometry of ALL engines and
 * every setter wipes the history, so it resynchronises there.)  jsg_destroy_sharded frees the set. */
JSG_API int jsg_create_sharded(jsg_engine** out, int* first_channel, int* channel_count, const int* devices, int n_devices, int channels);
JSG_API int jsg_process_block_sharded(jsg_engine* const* engines, const int* first_channel, int n_devices, const float* const* planar);
JSG_API int jsg_destroy_sharded(jsg_engine** engines, int n_devices);
JSG_API int jsg_destroy(jsg_engine* e);
JSG_API const char* jsg_last_error(const jsg_engine* e);   /* e may be NULL: last error of the calling thread */

/* setters: each rebuilds the memory like Spectrogram::buildmem (Spectrogram.cpp:213-238) */
JSG_API int jsg_set_samplerate(jsg_engine* e, float fs);                 /* Spectrogram.cpp:148-152 */
JSG_API int jsg_set_channels(jsg_engine* e, int channels);               /* :153-157 */
JSG_API int jsg_set_fft_size(jsg_engine* e, int n);                      /* :160-170 */
JSG_API int jsg_set_closest_fft_size_ms(jsg_engine* e, float ms);        /* :177-183 */
JSG_API int jsg_set_memory_time_s(jsg_engine* e, float seconds);         /* :184-188 */
JSG_API int jsg_set_feed_percent(jsg_engine* e, int feed);               /* :189-211, jsg_feed */
JSG_API int jsg_set_feed_percent_ext(jsg_engine* e, float percent);      /* extension: any overlap, e.g. 12.5 */
JSG_API int jsg_set_pause_mode(jsg_engine* e, int paused);               /* Spectrogram.h:122 */
JSG_API int jsg_set_window(jsg_engine* e, int window);                   /* Spectrogram.h:123 */
JSG_API int jsg_set_window_table(jsg_engine* e, const float* w, int n);  /* extension: caller-supplied window */
JSG_API int jsg_set_mix_mode(jsg_engine* e, int mode);                   /* m_mode has no setter in the reference (:21) */
JSG_API int jsg_set_power_scale(jsg_engine* e, float scale);             /* normalisation of spectrum::power, default 1 */
JSG_API int jsg_set_exact_log(jsg_engine* e, int on);                    /* extension: jsg_stft_args.exact_log for the engine's launches (default 0);
                                                                    keeps the ring (no buildmem) */

JSG_API int jsg_get_spectrum_size(const jsg_engine* e);                  /* Spectrogram.h:127 */
JSG_API int jsg_get_memory_size(const jsg_engine* e);                    /* Spectrogram.h:128 */
JSG_API float jsg_get_samplerate(const jsg_engine* e);                   /* Spectrogram.h:130 */
JSG_API int jsg_get_fft_size(const jsg_engine* e);
JSG_API int jsg_get_feed_samples(const jsg_engine* e);
JSG_API int jsg_get_feedblocks(const jsg_engine* e);
JSG_API int jsg_get_channels(const jsg_engine* e);
JSG_API int jsg_get_window(const jsg_engine* e, float* out, int n);      /* copy of m_window */

/* Spectrogram::processSynchronBlock (Spectrogram.cpp:37-135): `planar` = channels host pointers to fft-size samples each.
 * WAIT-FREE on the caller's (audio) thread: the block is copied into a page-locked single-producer ring and published with one
 * atomic store; a worker thread owned by the engine does the H2D copy and the launch.  No mutex, no HIP call, no allocation, never
 * a wait: when the ring is full (the GPU more than 64 blocks behind) or the engine is in the middle of a channel-count / FFT-size
 * change the block is DROPPED and counted.  Returns 0 (queued), 1 (dropped), < 0 (error -- also an error the worker thread met
 * earlier, text in jsg_last_error).  Readers, setters and jsg_sync see every block whose call returned before theirs began. */
JSG_API int jsg_process_block(jsg_engine* e, const float* const* planar);
/* The same for callers that state the geometry their pointers were sized for (host classes whose re-blocker runs unlocked beside
 * the FFT-size combo box): a block of another channel count or length than the engine's current one is dropped (returns 1)
 * instead of being read past its end.  0 = do not check that value. */
JSG_API int jsg_process_block_n(jsg_engine* e, const float* const* planar, int channels, int n);
/* The LOSSLESS form for callers that are not bound to real time (a DAW's offline bounce -- juce::AudioProcessor::isNonRealtime() --,
 * converters, test loops that push faster than the GPU takes blocks out): where jsg_process_block would drop a block because the ring is
 * full, this call waits (yield, then 100 us sleeps) until a slot is free, at most timeout_ms milliseconds (< 0: no limit).  The reference
 * never drops a block (Spectrogram.cpp:37-135 computes in place); this entry point keeps that property.  channels / n as in
 * jsg_process_block_n (0 = not checked).  Returns 0 (queued), 1 (dropped and counted: geometry change in progress, geometry mismatch, or
 * still full at the timeout), < 0 (error).  NOT for the audio thread of a live host. */
JSG_API int jsg_process_block_wait(jsg_engine* e, const float* const* planar, int channels, int n, int timeout_ms);
/* blocks that did not reach the ring since the engine was created: dropped by jsg_process_block(_n/_wait/_sharded), refused because of an
 * earlier worker error, or discarded by the worker */
JSG_API long long jsg_get_dropped_blocks(const jsg_engine* e);
/* The same for n_blocks consecutive blocks in one launch: samples[c*pitch + i], i < n_blocks*n. */
JSG_API int jsg_process_blocks(jsg_engine* e, const float* samples, int64_t pitch, int n_blocks);
/* The same with the samples already in HBM (device pointer, same layout); no host copy. */
JSG_API int jsg_process_blocks_device(jsg_engine* e, const float* d_samples, int64_t pitch, int n_blocks);

/* Spectrogram::getMem (Spectrogram.cpp:295-331): dst is the caller's dense [dst_columns][n/2+1]
 * buffer; copies all columns when at least a ring-full is new, else only the new ones (in place,
 * wrap-aware); returns the new-column count and zeroes it, -1 on size mismatch. */
JSG_API int jsg_get_mem(jsg_engine* e, float* dst, int dst_columns, int* pos);
/* The same into the reference's own container shape, vector<vector<float>> mem[W][H] (Spectrogram.h:144): rows[c]
 * points to the row_len = n/2+1 floats of column c (a NULL row is skipped); only the new columns are touched. */
JSG_API int jsg_get_mem_rows(jsg_engine* e, float* const* rows, int n_rows, int row_len, int* pos);
/* Extension: all columns of the ring as they are now, without consuming the new-column counter (returns the counter). */
JSG_API int jsg_peek_mem(jsg_engine* e, float* dst, int dst_columns, int* pos);
/* Device pointer / geometry of the dB ring (stays valid until the next setter). */
JSG_API int jsg_ring_device(jsg_engine* e, float** d_ring, int64_t* pitch, int* width, int* pos);
JSG_API int jsg_sync(jsg_engine* e);
JSG_API void* jsg_stream(jsg_engine* e);                                  /* the engine's hipStream_t */

/* ------------------------------------------------------------------------------------------------
 * 4. Display: the colour half of SpectrogramComponent::timerCallback (Spectrogram.cpp:590-731).
 * ------------------------------------------------------------------------------------------------ */
/* CColorPalette(n_colors, scheme) / setColorSceme (Spectrogram.cpp:337, :400); forces a full recolour */
JSG_API int jsg_display_set_colormap(jsg_engine* e, int n_colors, int scheme);
/* m_isRunningDisplay (Spectrogram.cpp:745-759) */
JSG_API int jsg_display_set_running(jsg_engine* e, int running);
/* m_recomputeAll = true (colour sliders, Spectrogram.cpp:370,379) */
JSG_API int jsg_display_invalidate(jsg_engine* e);
/* One timer tick: consumes the new columns (like getMem), colours them (all of them when a recolour is
 * pending) and writes the [height][width] ARGB image into host memory `argb` (`pitch` pixels per row).
 * min_color/max_color are the slider values (Spectrogram.cpp:614-617). */
JSG_API int jsg_display_update(jsg_engine* e, float min_color, float max_color, uint32_t* argb, int64_t pitch,
                       int* new_vals, int* pos);

/* Incremental tick for hosts that scroll their own image like the reference (moveImageSection + fill of the
 * right-most columns, Spectrogram.cpp:663-683): colours only the new columns and copies just them into `tile`
 * ([height][tile_pitch] pixels, oldest column first).  Returns 0 and *new_vals (<= max_cols) columns; returns 1
 * (nothing consumed) when a full recolour is pending or more than max_cols columns are new -- then call
 * jsg_display_update for the whole image. */
JSG_API int jsg_display_update_tile(jsg_engine* e, float min_color, float max_color, uint32_t* tile, int64_t tile_pitch,
                            int max_cols, int* new_vals, int* pos);

/* Frequency axis of the display image (section 2c).  scale JSG_AXIS_BINS (the default): one row per bin, height n/2+1, the other
 * arguments are ignored.  LINEAR / LOG / MEL: `height` rows over [fmin, fmax] Hz, checked against the engine's current sample rate
 * and FFT size (JSG_ERR_INVALID keeps the old axis).  An accepted call forces a full recolour: jsg_display_update_tile returns 1
 * until jsg_display_update has run, and the whole history is drawn on the new axis.  The engine keeps the requested range; after
 * jsg_set_samplerate / jsg_set_fft_size the next tick rebuilds the rows with paint()'s clamps (Spectrogram.cpp:444-452: fmin >= fs/2
 * -> 0.9 fs/2, fmax >= fs/2 -> fs/2, fmin >= fmax -> 0.9 fmax) and recolours everything; the requested range comes back with a
 * sample rate that admits it. */
JSG_API int jsg_display_set_freq_axis(jsg_engine* e, int scale, int height, float fmin, float fmax);
/* Image rows that the next jsg_display_update / _tile writes (the `argb` buffer has this many rows). */
JSG_API int jsg_display_height(const jsg_engine* e);
/* Centre frequency (Hz) of every image row, bottom row first, for tick labels: n >= jsg_display_height (else JSG_ERR_SIZE_MISMATCH);
 * BINS: k fs / n.  Returns the row count. */
JSG_API int jsg_display_axis_centres(jsg_engine* e, float* centre_hz, int n);

/* The frequency window of SpectrogramComponent::paint (Spectrogram.cpp:441-459): which image rows show
 * [min_freq, max_freq] Hz.  Pure host arithmetic (same clamps and roundings); outputs displayStartPixel,
 * displayEndPixel, heightInterval and hStart (= height - displayEndPixel, the first image row to blit). */
JSG_API int jsg_display_freq_rows(float fs, int height, float min_freq, float max_freq, int* start_pixel, int* end_pixel,
                          int* height_interval, int* h_start);

#ifdef __cplusplus
}
#endif
#endif /* JSG_H_ */
