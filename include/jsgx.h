/* jsgx.h -- the companion library of libjsg (libjsgx.so): analysis operations that live outside the plugin engine's C-ABI.
 *
 * libjsg.so (include/jsg.h) is the engine behind the reference's Spectrogram surface; its ABI is closed at version 6 with 146 entry
 * points.  Operations that a plugin host never calls are added here instead: libjsgx.so has its own ABI version (JSGX_ABI_VERSION),
 * its own error text, and neither links against libjsg.so nor uses its internals.  The two libraries meet in device memory only:
 * what one writes the other reads (section 1 takes the `lag` buffer of jsg_tempo_launch as it is).
 *
 * Conventions (those of jsg.h):
 *   - hand-written HIP for gfx950 (MI355X); there is NO CPU fallback: a launch without a HIP device fails with JSGX_ERR_NO_DEVICE
 *   - launches are enqueue-only on the caller's stream (a hipStream_t passed as void*; NULL = the default stream): no allocation,
 *     no synchronisation, so a launch can be captured into a hipGraph, a first launch included
 *   - every failure returns a negative jsgx_status and leaves a text for jsgx_last_error() (thread-local)
 *   - the definitions below are complete: every order of summation, tie rule and NaN rule is stated, all device arithmetic is
 *     float32 and uncontracted except where fmaf is written, so a CPU restatement (tests/beat_ref.py) gives the same bits
 */
#ifndef JSGX_H
#define JSGX_H

#include <stdint.h>

#if defined(__GNUC__)
#define JSGX_API __attribute__((visibility("default")))
#else
#define JSGX_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define JSGX_ABI_VERSION 1

typedef enum jsgx_status {
    JSGX_OK = 0,
    JSGX_ERR_INVALID = -2,       /* a refused argument; nothing was enqueued */
    JSGX_ERR_HIP = -4,           /* a HIP call failed */
    JSGX_ERR_NO_DEVICE = -5      /* no HIP device */
} jsgx_status;                   /* the values of the same names in jsg.h */

/* JSGX_ABI_VERSION of the library that is loaded. */
JSGX_API int jsgx_abi_version(void);
/* The text of the calling thread's last failure ("" before the first); valid until that thread's next failing call. */
JSGX_API const char* jsgx_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * 1. Beat tracking by dynamic programming (Ellis 2007, "Beat tracking by dynamic programming"; the core of
 *    librosa.beat.beat_track): from an onset envelope and a period in frames to the frames of the beats.  One row is one
 *    envelope; rows are independent.  Nothing depends on the number of rows, on the pitches, on which optional outputs are NULL
 *    or on the form of the kernel (jsgx_beat_plan).  All arithmetic is float32 and uncontracted; fmaf is written where it is meant.
 *
 *    Inputs of a row r: o[t] = in[r*in_pitch + t], t = 0..T-1;  P = period[r] (period given) or period_all (period NULL);
 *    L[k] = log_table[k] (jsgx_log_table_build: the natural logarithm of k);  tightness;  the switches smooth and normalise.
 *
 *    Bad period.  P outside 1..JSGX_BEAT_MAX_PERIOD (the -1 that jsg_tempo_launch writes for a NaN row included):
 *        n_beats[r] = -1 and nothing else is written for the row.
 *    NaN.  Any o[t] is NaN:  n_beats[r] = -1 and nothing else is written for the row.
 *    Infinities in o, and finite values so large that a sum below overflows, are outside the contract: the launch still ends and
 *    writes nothing but the row's outputs, whose values are then unspecified.
 *
 *    The lane sum of T values v[t] (the rule of jsg.h section 2j with W = 256): lane l of 256 adds t = l, l + 256, l + 512, ...
 *    ascending with plain adds from +0; then a halving tree: for h = 128, 64, ..., 1:  acc_l = acc_l + acc_(l+h) for l < h; the
 *    sum is acc_0.  The order depends on nothing but T.
 *
 *    Normalise.  normalise = 1 and T > 1:
 *        mean = (lane sum of o[t]) / (float)T;     d[t] = o[t] - mean;     q[t] = d[t] * d[t]
 *        sd = sqrtf((lane sum of q[t]) / (float)(T - 1))        (the sample standard deviation, ddof = 1; divide and root correctly rounded)
 *        s0[t] = o[t] / sd  (correctly rounded)  where sd != 0;   s0 = o where sd == 0.
 *    normalise = 0 or T == 1:  s0 = o.
 *
 *    Local score.  smooth = 0:  s = s0.   smooth = 1:
 *        z = fl(fl(32.0f * (float)k) / (float)P);    x = -0.5f * fl(z * z);    g[k] = jsgx_exp(x),   k = 0..P   (g[-k] = g[k])
 *        s[t]: acc = +0; for k = -P, -P+1, ..., P in this order, where 0 <= t + k < T:  acc = fmaf(g[|k|], s0[t+k], acc)
 *    Terms outside the row are left out, not multiplied by zero; terms whose g is +0 are not left out.
 *
 *    jsgx_exp(x), x <= 0, from plain float32 operations (add, multiply, fmaf, floor, integer bit manipulation), no hardware exp:
 *        x < -87.0f:  +0            (exp(x) < 1.7e-38: g is taken as zero there)
 *        n = floorf(fmaf(x, 1.44269502162933349609375f, 0.5f))                          (log2(e) as a float)
 *        r = fmaf(n, -0.693145751953125f, x);   r = fmaf(n, -1.42860676533018704503775e-06f, r)        (ln 2 = hi + lo, hi exact in 11 bits)
 *        p = 1.984127011382952332496643e-04f                                                         (1/5040, Horner with fmaf, degree 7)
 *        p = fmaf(p, r, 1.388888922519981861114502e-03f);  p = fmaf(p, r, 8.333333767950534820556641e-03f)
 *        p = fmaf(p, r, 4.166666790843009948730469e-02f);  p = fmaf(p, r, 1.666666716337203979492188e-01f)
 *        p = fmaf(p, r, 0.5f);   p = fmaf(p, r, 1.0f);   p = fmaf(p, r, 1.0f)
 *        jsgx_exp = p * (the float with the bits (n + 127) << 23)          (2^n, -126 <= n <= 0: the product is exact)
 *    Against exp in double over every (P, k), P <= 1024, whose x >= -87: the relative error is at most JSGX_EXP_REL_BOUND
 *    (measured: profiles/beat_accuracy.md; the test asserts this bound); below -87 the absolute error is exp(x) itself, < 1.7e-38.
 *
 *    Penalty.  a = (P + 1) / 2 (integer division).  For tau = a..2P:
 *        d = L[tau] - L[P];     pen[tau] = -(fl(tightness * d) * d)        (two multiplies, uncontracted)
 *
 *    Dynamic programme, t = 0, 1, ..., T-1:   C[u] = +0 for u < 0;
 *        v(tau) = fl(pen[tau] + C[t - tau]),  tau = a..2P
 *        tau* = the tau with the largest v, the lowest tau among equal v  (+0 and -0 are equal);   best = v(tau*)
 *        C[t] = s[t] + best
 *        link[t] = t - tau*  where t - tau* >= 0, else -1
 *    First-beat rule:  th = 0.01f * (the maximum of s[t] over the row);  t0 = the first t with s[t] >= th, T where there is none;
 *        link[t] = -1 for every t < t0.  C is not changed by this rule.
 *    End:  e = the t in [max(0, T - P), T) with the largest C[t], the lowest t among equal C.
 *    Backtrace:  the chain e, link[e], link[link[e]], ... until -1 is met;  n = its length (>= 1: e itself is a beat).
 *        n_beats[r] = n;   beats[r*beats_pitch + i], i = 0..min(n, max_beats)-1, is the chain in ASCENDING order: where the chain
 *        is longer than max_beats its earliest beats are the ones kept.  Nothing behind them is written.
 *        local_score[r*local_pitch + t] = s[t] and cum_score[r*cum_pitch + t] = C[t], t = 0..T-1, where these are given.
 *
 *    Known answers.  An all-zero row (normalise on or off): every v is pen[tau] + 0; pen[P] = -0 and every other pen is below
 *    zero, so tau* = P and best = -0 + 0 = +0; C = +0 everywhere; th = +0, t0 = 0; link[t] = t - P; e = max(0, T - P); the beats
 *    are e, e - P, e - 2P, ... down to the last >= 0.  A constant row c > 0 with normalise = 1 has sd = 0 where the lane sums are
 *    exact, so s = o.
 *
 *    Deliberate differences from librosa.beat.beat_track: the period is an integer number of frames (librosa keeps the float
 *    60 * frame_rate / bpm); the end of the chain is Ellis' rule (the best C within the last period), not librosa's median-of-
 *    maxima rule; weak leading and trailing beats are not trimmed; ties go to the lowest tau and the lowest t; the envelope is
 *    divided by its sample standard deviation as librosa does, and the smoothing window is librosa's Gaussian exp(-0.5 (32k/P)^2).
 *    Agreement with librosa has not been measured.
 *
 *    The kernel: one workgroup of JSGX_BEAT_THREADS lanes per row.  The recurrence looks back at least a frames, so the frames
 *    t .. t+a-1 depend only on C[< t]: a workgroup advances F frames per step from a ring of C and a table of pen in LDS.
 *    "beat_frames" (P >= 511, a >= 256): F = 256, one lane per frame runs over all tau.  "beat_split" (P <= 510): G = the smallest
 *    power of two <= 64 with 256 / G <= a (64 where there is none), F = min(256 / G, a); the G lanes of a frame take tau = a + j,
 *    a + j + G, ... and are reduced with the tie rule above.  Only the backtrace is serial: two walks of at most T / a steps.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_BEAT_MAX_PERIOD 1024
#define JSGX_BEAT_MAX_FRAMES 16777216      /* 2^24 */
#define JSGX_BEAT_THREADS 256
#define JSGX_BEAT_LDS_BYTES 31008          /* static: ring 4096, pen 2052, g 1028, 2 x 256 reduction slots, the vote of the NaN check */
#define JSGX_EXP_REL_BOUND 1.0e-7          /* jsgx_exp against exp in double, x >= -87 (measured 7.3e-8: profiles/beat_accuracy.md) */

/* The table L of the penalty, on the host (no device): out[0] = 0, out[k] = log((double)k) rounded to float32 once, k = 1..n-1.  The
 * launch takes the table of n = 2*JSGX_BEAT_MAX_PERIOD + 1 entries in device memory.  JSGX_ERR_INVALID: a null out, n outside
 * 1..2*JSGX_BEAT_MAX_PERIOD+1. */
JSGX_API int jsgx_log_table_build(int32_t n, float* out);

typedef struct jsgx_beat_args {
    const float* in;            /* device floats: o[r][t] at in[r*in_pitch + t] */
    int64_t in_pitch;           /* rows > 1: >= n_frames */
    int32_t rows;               /* 1..65535, independent */
    int32_t n_frames;           /* T, 1..JSGX_BEAT_MAX_FRAMES */
    const int32_t* period;      /* device int32 [rows] (what jsg_tempo_launch writes as lag), or NULL: period_all for every row */
    int32_t period_all;         /* period NULL: 1..JSGX_BEAT_MAX_PERIOD; else ignored */
    int32_t smooth;             /* 0 or 1 */
    const float* log_table;     /* device floats [2*JSGX_BEAT_MAX_PERIOD + 1]: jsgx_log_table_build */
    float tightness;            /* finite, > 0 (librosa: 100) */
    int32_t normalise;          /* 0 or 1 */
    int32_t* beats;             /* device int32: beats[r][i] at beats[r*beats_pitch + i] */
    int64_t beats_pitch;        /* rows > 1: >= max_beats */
    int32_t max_beats;          /* 1..JSGX_BEAT_MAX_FRAMES: the beats kept per row */
    int32_t reserved0;          /* 0 */
    int32_t* n_beats;           /* device int32 [rows]: the length of the chain (may exceed max_beats), -1 for a refused row */
    float* local_score;         /* device floats or NULL: s[r][t] at local_score[r*local_pitch + t] */
    int64_t local_pitch;        /* rows > 1 and local_score given: >= n_frames */
    float* cum_score;           /* device floats or NULL: C[r][t] at cum_score[r*cum_pitch + t] */
    int64_t cum_pitch;          /* rows > 1 and cum_score given: >= n_frames */
} jsgx_beat_args;

/* The bytes of scratch the launch needs: 4 * rows * T for link, and as much again for s where smooth = 1.  Refused (a negative
 * jsgx_status): what the launch refuses before it looks at the scratch. */
JSGX_API int64_t jsgx_beat_scratch_bytes(const jsgx_beat_args* args);
/* Enqueue only (one kernel): no allocation, no synchronisation; hipGraph capture works, a first launch included.  The scratch is
 * used only while the kernel runs.  Refused (JSGX_ERR_INVALID, nothing enqueued, jsgx_last_error set), in this order and before any
 * device call: null args, a null in, a null log_table, a null beats, a null n_beats, a pointer that is not 4-byte aligned, rows
 * outside 1..65535, n_frames outside 1..2^24, period NULL and period_all outside 1..1024, a tightness that is not finite and > 0,
 * smooth other than 0 or 1, normalise other than 0 or 1, max_beats outside 1..2^24, a non-zero reserved0, in_pitch below n_frames
 * (rows > 1), beats_pitch below max_beats (rows > 1), local_pitch below n_frames (rows > 1, local_score given), cum_pitch below
 * n_frames (rows > 1, cum_score given), an output (beats, n_beats, local_score, cum_score) overlapping in, one overlapping
 * period, one overlapping log_table, a null scratch, a scratch that is not 4-byte aligned, scratch_bytes below jsgx_beat_scratch_bytes.  Then
 * JSGX_ERR_NO_DEVICE without a HIP device.  Every call that passes is served. */
JSGX_API int jsgx_beat_launch(const jsgx_beat_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the kernel does for a row of this period, without a device (args->period is never read): the form ("beat_frames" or
 * "beat_split", above), the lanes of a workgroup (JSGX_BEAT_THREADS) and the bytes of LDS it holds (JSGX_BEAT_LDS_BYTES, static and
 * the same for every period since the period is known on the device only; <= 163840).  Any output pointer may be NULL (name: else
 * name_len >= 16).  Refused: a name_len below 16 with a name, then what jsgx_beat_scratch_bytes refuses, then a period outside
 * 1..1024. */
JSGX_API int jsgx_beat_plan(const jsgx_beat_args* args, int32_t period, char* name, int name_len, int32_t* threads, int32_t* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* JSGX_H */
