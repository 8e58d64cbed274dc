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
 *     float32 and uncontracted except where fmaf is written, so a CPU restatement (tests/beat_ref.py, tests/dtw_ref.py) gives the same bits
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

/* Sections 2 and 3 were added to version 1: JSGX_ABI_VERSION counts changes to what exists, and version 1 grows by addition only.
 * Section 1, its struct and its constants are as they were; a program built against the earlier header runs unchanged. */

/* ------------------------------------------------------------------------------------------------
 * 2. The pairwise cost of two feature sequences (scipy.spatial.distance.cdist for three metrics): the first half of
 *    librosa.sequence.dtw.  A pair p has N frames x[i][k] = x[p*x_pair_pitch + i*x_frame_pitch + k] and M frames
 *    y[j][k] = y[p*y_pair_pitch + j*y_frame_pitch + k], k = 0..K-1: the frame-major layout the feature kernels of libjsg.so write.
 *    A pair pitch of 0 is one sequence shared by every pair (query by example).  cost[p*cost_pair_pitch + i*cost_pitch + j] = c(i, j).
 *    All arithmetic is float32 and uncontracted; fmaf is written where it is meant; k ascends; every accumulator starts at +0;
 *    fl(.) is one rounding to float32; sqrtf and the divide are correctly rounded.
 *
 *    JSGX_METRIC_SQEUCLIDEAN:  d = fl(x[i][k] - y[j][k]);  acc = fmaf(d, d, acc);  c = acc.
 *    JSGX_METRIC_EUCLIDEAN:    the same acc;  c = sqrtf(acc).
 *    JSGX_METRIC_COSINE:       dot = fmaf(x, y, dot);  nx = fmaf(x, x, nx);  ny = fmaf(y, y, ny);  den = fl(sqrtf(nx) * sqrtf(ny));
 *                              c = 1.0f where den == 0, else fl(1.0f - fl(dot / den)).
 *    A zero vector under the cosine metric gives 1 here; scipy gives NaN: a stated difference.  NaN and infinity go through these
 *    operations as IEEE 754 has it; nothing is special-cased.  The result depends on nothing but x[i][.], y[j][.], K and the metric.
 *
 *    Error bounds against exact arithmetic on the same float32 inputs, u = 2^-24, to first order in u.  d is one rounding and d*d
 *    is exact inside the fmaf, so a term carries (1 + u)^2 and each of the K sums one more rounding; the terms are non-negative, so
 *    acc = S (1 + t) with |t| <= (K + 2) u: sqeuclidean is relative (K + 2) u.  The root halves that and adds its own rounding:
 *    euclidean is relative (K/2 + 2) u.  The second-order part is below K^2 u^2 / 2 < 0.04 u at K = 1024, so both are inside
 *    (K + 3) u, which tests/test_dtw_ref.py asserts.  Cosine: |dot - DOT| <= K u sum|x y| <= K u |x||y| (Cauchy-Schwarz); nx and
 *    ny are sums of non-negative terms, relative K u each, K u / 2 + u after their roots, so den = |x||y| (1 + h), |h| <= (K + 3) u;
 *    the quotient and the subtraction add u |q| and u |1 - q| <= 2 u.  With r = DOT / (|x||y|):  |c - C| <= (K + (K + 4) |r| + 2) u,
 *    (2 K + 6) u in the worst case (parallel vectors, every rounding in one direction) and (K + 2) u for orthogonal ones.  The test
 *    asserts the tighter (K + 5) u that was set for it; it is not a worst-case bound: the roundings of dot and of den would all have
 *    to point one way to pass it, and over normal, positive and near-duplicate data up to K = 1024 the worst error found is 24 u
 *    (34 u relative for sqeuclidean, 17 u for euclidean; profiles/dtw_accuracy.md).
 *
 *    The kernel ("cdist_64x64"): a workgroup of JSGX_CDIST_THREADS lanes computes JSGX_CDIST_TILE x JSGX_CDIST_TILE costs of one
 *    pair; panels of 32 features of 64 frames of x and of y are staged in LDS feature-major, a lane reads four x and four y with
 *    two 16-byte LDS reads per feature and holds a 4 x 4 register tile; k ascends within a lane, so the order is the one above.
 *    The accumulation order is stated, so this runs on the vector pipe, not on MFMA.  One kernel, no scratch.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_METRIC_SQEUCLIDEAN 0
#define JSGX_METRIC_EUCLIDEAN 1
#define JSGX_METRIC_COSINE 2
#define JSGX_CDIST_MAX_FEATURES 1024
#define JSGX_DTW_MAX_LEN 65536
#define JSGX_CDIST_TILE 64
#define JSGX_CDIST_THREADS 256
#define JSGX_CDIST_LDS_BYTES 17408         /* static: two panels of 32 features x 68 words */

typedef struct jsgx_cdist_args {
    const float* x;             /* device floats */
    int64_t x_frame_pitch;      /* >= n_features */
    int64_t x_pair_pitch;       /* 0 (shared), or >= (n - 1) * x_frame_pitch + n_features */
    const float* y;             /* device floats */
    int64_t y_frame_pitch;      /* >= n_features */
    int64_t y_pair_pitch;       /* 0 (shared), or >= (m - 1) * y_frame_pitch + n_features */
    int32_t pairs;              /* 1..65535 */
    int32_t n_features;         /* K, 1..JSGX_CDIST_MAX_FEATURES */
    int32_t n;                  /* N, 1..JSGX_DTW_MAX_LEN */
    int32_t m;                  /* M, 1..JSGX_DTW_MAX_LEN */
    int32_t metric;             /* JSGX_METRIC_* */
    int32_t reserved0;          /* 0 */
    float* cost;                /* device floats */
    int64_t cost_pitch;         /* >= m */
    int64_t cost_pair_pitch;    /* pairs > 1: >= (n - 1) * cost_pitch + m */
} jsgx_cdist_args;

/* Enqueue only (one kernel, no scratch).  Refused (JSGX_ERR_INVALID, nothing enqueued), in this order and before any device call:
 * null args, a null x, a null y, a null cost; a pointer that is not 4-byte aligned; pairs outside 1..65535, n_features outside
 * 1..1024, n outside 1..65536, m outside 1..65536, a metric outside 0..2; a non-zero reserved0; x_frame_pitch below n_features,
 * y_frame_pitch below n_features, a non-zero x_pair_pitch that does not cover a sequence, the same for y_pair_pitch, cost_pitch
 * below m, cost_pair_pitch that does not cover a plane (pairs > 1); cost overlapping x, cost overlapping y.  Then
 * JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_cdist_launch(const jsgx_cdist_args* args, void* stream);
/* The kernel of these arguments, without a device: its name ("cdist_64x64"), JSGX_CDIST_THREADS and JSGX_CDIST_LDS_BYTES.  Any
 * output pointer may be NULL (name: else name_len >= 16).  Refused: a name_len below 16 with a name, then what the launch refuses. */
JSGX_API int jsgx_cdist_plan(const jsgx_cdist_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes);

/* ------------------------------------------------------------------------------------------------
 * 3. Dynamic time warping over a cost plane (the second half of librosa.sequence.dtw).  C[i][j] = cost[p*cost_pair_pitch +
 *    i*cost_pitch + j], i < N, j < M: the plane of section 2 or any plane the caller filled.  Pairs are independent.  The steps are
 *    k = 0: (1, 1), k = 1: (0, 1), k = 2: (1, 0) as (di, dj): librosa's default step_sizes_sigma in its order; weights_mul[k] and
 *    weights_add[k] are librosa's.  All arithmetic is float32 and uncontracted.
 *
 *    Band.  band = 0: none.  band = R >= 1: the cell (i, j) is inside iff |j*(N-1) - i*(M-1)| <= R*max(N-1, 1), in int64.  A cell
 *    outside has D = +inf.  band together with subseq is refused.
 *
 *    Recurrence.  D[0][0] = C[0][0];  with subseq, D[0][j] = C[0][j] for every j.  For every other inside cell:
 *        e_k = fl(fl(weights_mul[k] * C[i][j]) + weights_add[k])
 *        v_k = fl(D[i - di_k][j - dj_k] + e_k),  a predecessor outside the matrix counting as +inf
 *        best = v_0;  for k = 1, 2:  if (v_k < best) best = v_k;        D[i][j] = best
 *    The comparison is strict: the lowest k wins ties and a NaN v_k never replaces best (a NaN v_0 stays).  +0 and -0 compare
 *    equal but the bits of D are what they are: 1*c + 0 is +0 for c = -0, and the operations are kept as written.  D[i][j] is a
 *    function of the cell alone: it does not depend on the tile sizes, on pairs or on the pitches.
 *
 *    End cell.  Global: (N-1, M-1).  subseq: i = N-1 and the lowest j among the minimal D[N-1][j]; if any D[N-1][j] is a NaN the
 *    pair has no path.
 *    Backtrace.  At (i, j): D[i][j] a NaN or +inf: path_len[p] = -1 and nothing else is written for the pair (D apart).  Else
 *    v_0..v_2 are recomputed from D and C with the same operations and the same selection, and the walk moves to that predecessor;
 *    it ends at (0, 0) (global) or at i = 0 (subseq).  No step matrix is kept: the recomputation repeats the forward choice.
 *    Outputs.  path_len[p] = L;  path_i and path_j at [p*path_pitch + n], n < L, ascending, the start first;  total[p] = D at the
 *    end cell.  acc receives D: acc[p*acc_pair_pitch + i*acc_pitch + j].
 *
 *    Known answers.  An all-zero C, global: D = +0 everywhere (weights 1, 0); every v ties, so step 0 is taken while i > 0 and
 *    j > 0: the path runs on the diagonal back from (N-1, M-1) and then along the edge to (0, 0).  A band whose diagonal slope
 *    (M-1)/(N-1) exceeds 2R + 1 leaves no path: 65 x 200 has none with R = 1 and one with R = 2; 10 x 100 none with R = 4, one
 *    with R = 5.
 *    total against exact arithmetic, for non-negative costs and weights: min is monotone and every sum is of non-negative terms,
 *    so a cell adds at most 3 roundings (two for e, one for v) to the relative error of its best predecessor, and a path has at
 *    most N + M - 1 cells: relative 3 (N + M) 2^-24.
 *
 *    Differences from librosa.sequence.dtw: only the three unit steps; the band is the integer rule above, not the float rule of
 *    fill_off_diagonal; the tie and NaN rules are the ones above.  Agreement with librosa has not been measured.
 *
 *    The kernels.  D is cut into tiles of JSGX_DTW_TILE_ROWS x JSGX_DTW_TILE_COLS; the tiles of one tile anti-diagonal are
 *    independent, and "dtw_tiles" is launched once per tile anti-diagonal over pairs x (tiles on it), one wavefront per tile: a
 *    tile reads its top row, left column and corner from D itself, which the earlier launches on the stream wrote, so no workgroup
 *    waits for another.  Inside a tile the sweep is skewed: lane l owns row l and computes column s - l at step s; its three
 *    neighbours are its own last value and the last two of lane l - 1, moved by a DPP wave shift.  C comes in and D goes out
 *    through LDS in whole lines; the row pitch of 64 words lets lane l read column s - l from 64 different banks.  A tile wholly
 *    outside the band is filled with +inf without reading C.  "dtw_backtrace" is one more kernel, one wavefront per pair: it
 *    finds the end cell, then fetches 32 x 32 windows of D and C that end at the current cell and walks inside each (at least 31
 *    steps per round trip to memory), writes the path backwards into the scratch and copies it out reversed.
 * ------------------------------------------------------------------------------------------------ */
/* The tile sizes were chosen by measurement on an MI355X (profiles/dtw_bench.md): the chain of dependent sweep steps decides the time, and
 * N x M takes about (N / rows + M / cols) (cols + rows - 1) of them, least at cols = rows; 128 and 256 columns were 31 % and 82 % slower at
 * 16384 x 16384.  The lane move is the DPP wave shift: 5 % ahead of __shfl_up, and it keeps the LDS pipe off the chain. */
#define JSGX_DTW_TILE_ROWS 64
#define JSGX_DTW_TILE_COLS 64
#define JSGX_DTW_THREADS 64
#define JSGX_DTW_LDS_BYTES 16656           /* static, of the forward kernel: the tile 64 x 64 words, the top row with its corner 65 + 3 */

typedef struct jsgx_dtw_args {
    const float* cost;          /* device floats: C */
    int64_t cost_pitch;         /* >= m */
    int64_t cost_pair_pitch;    /* pairs > 1: >= (n - 1) * cost_pitch + m */
    int32_t pairs;              /* 1..65535 */
    int32_t n;                  /* N, 1..JSGX_DTW_MAX_LEN */
    int32_t m;                  /* M, 1..JSGX_DTW_MAX_LEN */
    int32_t subseq;             /* 0 or 1 */
    int32_t band;               /* 0, or R in 1..JSGX_DTW_MAX_LEN */
    int32_t reserved0;          /* 0 */
    float weights_mul[3];       /* finite */
    float weights_add[3];       /* finite */
    float* acc;                 /* device floats: D, required */
    int64_t acc_pitch;          /* >= m */
    int64_t acc_pair_pitch;     /* pairs > 1: >= (n - 1) * acc_pitch + m */
    int32_t* path_i;            /* device int32 or NULL (then path_j NULL too) */
    int32_t* path_j;
    int64_t path_pitch;         /* pairs > 1 and paths given: >= max_path */
    int32_t max_path;           /* paths given: >= n + m - 1 */
    int32_t* path_len;          /* device int32 [pairs]; required with the paths, else optional */
    float* total;               /* device floats [pairs] or NULL */
} jsgx_dtw_args;

/* The bytes of scratch the launch needs: 8 * pairs * (n + m - 1) where the paths are given, else 0.  Refused: what the launch
 * refuses before it looks at the scratch. */
JSGX_API int64_t jsgx_dtw_scratch_bytes(const jsgx_dtw_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  The kernels (one per tile
 * anti-diagonal, then the backtrace where path_len or total is given) go onto the one stream as a plain chain.  Refused
 * (JSGX_ERR_INVALID, nothing enqueued), in this order and before any device call: null args, a null cost, a null acc, one of
 * path_i and path_j without the other, paths without path_len; a pointer that is not 4-byte aligned; pairs outside 1..65535, n
 * outside 1..65536, m outside 1..65536, subseq other than 0 or 1, band outside 0..65536, a weight that is not finite; a non-zero
 * reserved0; band together with subseq; max_path below n + m - 1 (paths given); cost_pitch below m, cost_pair_pitch that does
 * not cover a plane (pairs > 1), the same for acc_pitch and acc_pair_pitch, path_pitch below max_path (pairs > 1, paths given);
 * acc overlapping cost, another output (path_i, path_j, path_len, total) overlapping cost, another output overlapping acc; a
 * null scratch, a scratch that is not 4-byte aligned, scratch_bytes below the size above (each only where that size is not 0).
 * Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_dtw_launch(const jsgx_dtw_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the name of the forward kernel ("dtw_tiles"), the tile sizes, the number of kernel
 * launches (the tile anti-diagonals, ceil(n / tile_rows) + ceil(m / tile_cols) - 1, plus one for the backtrace where path_len or
 * total is given), JSGX_DTW_THREADS and JSGX_DTW_LDS_BYTES.  Any output pointer may be NULL (name: else name_len >= 16).  Refused:
 * a name_len below 16 with a name, then what the scratch size refuses. */
JSGX_API int jsgx_dtw_plan(const jsgx_dtw_args* args, char* name, int name_len, int32_t* tile_rows, int32_t* tile_cols, int32_t* n_launches,
                           int32_t* threads, int32_t* lds_bytes);

/* Section 4 was added to version 1 in the same way: sections 1 to 3, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 4. Viterbi decoding of a hidden Markov model (the first function of librosa.sequence's second half): from frame-wise
 *    log-likelihoods to the most likely state sequence.  A sequence q has T frames and S states; sequences are independent.  All
 *    arithmetic is float32 and uncontracted (there are only additions and comparisons); fl(.) is one rounding to float32.  Every
 *    input is a log-probability, and -inf (probability zero) is an ordinary value.  Nothing depends on seqs, on the pitches, on
 *    which optional outputs are NULL or on the form of the kernel (jsgx_viterbi_plan).
 *
 *    Inputs.  Emissions b[t][s] = log_emit[q*emit_seq_pitch + t*emit_frame_pitch + s]: frame-major, the state fastest, the layout
 *    the feature kernels of libjsg.so write.  The initial vector p0[s] = log_init[s] and the transition A(i, j), from the source
 *    i to the destination j, are shared by all sequences.  A comes in one of two forms (trans_form):
 *      JSGX_TRANS_DENSE:  A(i, j) = trans[i*trans_pitch + j], trans_pitch >= S; the sources of j are i = 0..S-1.
 *      JSGX_TRANS_BAND with the half-width W = band_half, 0 <= W <= JSGX_VITERBI_MAX_BAND_HALF: the sources of j are
 *          i = max(0, j-W) .. min(S-1, j+W), and A(i, j) = trans[(i - j + W)*trans_pitch + j]: diagonal-major, 2W+1 rows of S, so
 *          that consecutive destinations are consecutive words.  An entry whose source would lie outside 0..S-1 is never read.
 *          The band need not be Toeplitz: a locally normalised transition (librosa.sequence.transition_local,
 *          jsgx_viterbi_band_build) fits, and so does pYIN's voiced/unvoiced x pitch product with the two kinds of state interleaved.
 *
 *    Recurrence.  V[0][s] = fl(p0[s] + b[0][s]).  For t >= 1 and every j, over the sources i of j:
 *        v(i) = fl(V[t-1][i] + A(i, j));     w(i) = v(i), or -inf where v(i) is a NaN
 *        i* = the source with the largest w, the lowest i among equal w (+0 and -0 are equal);   best = w(i*), with the bits of that w
 *        V[t][j] = fl(best + b[t][j]);       psi[t][j] = i*
 *    The selection is a reduction with the pair rule "(w, i) beats (w', i') iff w > w', or w == w' and i < i'".  The rule is a
 *    total order on the pairs of one destination (the i are distinct), so its maximum is associative and commutative: the result
 *    does not depend on how a kernel splits the sources among lanes or in which order it meets them.
 *    End.  w_s = V[T-1][s], a NaN counted as -inf;  e = the lowest s among the largest w_s;  logp[q] = w_e.
 *    Backtrace.  states[T-1] = e;  states[t-1] = psi[t][states[t]] for t = T-1 down to 1.
 *    Outputs.  states[q*states_pitch + t] (int32);  logp[q] where given;  value[q*value_seq_pitch + t*value_frame_pitch + s] =
 *    V[t][s] where given (a NaN of V is stored as it came out of the addition).
 *    A path is always written.  logp = -inf says that no path has a probability above zero: the states are then what the tie
 *    rule gives and mean nothing.  That is a result, not a refusal: the launch returns JSGX_OK, and only a refused argument returns
 *    JSGX_ERR_INVALID.
 *
 *    NaN.  A NaN emission b[t][s] makes V[t][s] a NaN (value shows it); as a source of frame t+1 that state counts as -inf, and as
 *    an end state too.  Nothing else is touched.  A NaN in A or p0 goes the same way: v is a NaN and counts as -inf.  +inf is
 *    inside the contract only in so far as these operations define it (+inf + -inf is a NaN and counts as -inf).
 *
 *    Known answers.  All inputs +0 (S states, T frames, either form): every v is +0, every tie goes to the lowest source, V = +0
 *    everywhere, psi = 0 (dense) or max(0, j-W) (band), e = 0, so states are all 0 and logp = +0.  A band with W = 0 and a finite
 *    diagonal: psi[t][j] = j, so states are constant at the end state e.  A frame t whose emissions are all -inf: V[t'] = -inf for
 *    every t' >= t, logp = -inf, e = 0, and the states follow the tie rule (dense: all 0).  A NaN emission at (t, s): above.
 *
 *    Error bound, for finite inputs that are all <= 0, against exact arithmetic on the same float32 inputs, u = 2^-24.  Every
 *    addition is of two terms of one sign, so nothing cancels: a computed sum is the exact sum of its computed operands times
 *    (1 + d), |d| <= u.  The maximum is monotone and exact: if every candidate has the relative error g, so has the largest
 *    (all are <= 0).  V[0] carries one rounding; a frame t >= 1 adds one for v and one for V[t]: V[T-1], and so logp, carries at
 *    most 2T - 1 roundings, a relative (1 + u)^(2T-1) - 1 <= (2T - 1) u + (2T u)^2 / 2 (1 + 2T u).  For T <= 4096 the second-order
 *    part is at most 2^-23 (1 + 2^-11) < 3 u, so the whole is inside (2T + 2) u, which tests/test_viterbi_ref.py asserts against
 *    float64 (whose own error is 2^-29 of that).  The states are exact where the exact optimum leads its runners-up by more than
 *    this; elsewhere a different, nearly as likely path may come out.
 *
 *    Differences from librosa.sequence.viterbi: the inputs are logarithms (librosa takes probabilities and takes the logarithms
 *    itself) and frame-major (librosa: [states][frames]); ties go to the lowest state (librosa: numpy's argmax, the same, but over
 *    values computed in another order); log_init is required here (librosa's p_init defaults to the uniform vector; the Python
 *    layer supplies that default).  Agreement with librosa has not been measured: librosa is not installed where this was built.
 *
 *    The kernels.  Time is serial, so "the forward kernel" decodes one sequence per workgroup from t = 0 to T-1; workgroups of
 *    different sequences never wait for one another: no grid barrier, no ticket, no spin loop.  A lone sequence therefore uses one
 *    compute unit; that is accepted.  V[t-1] and V[t] are two rows in LDS with one workgroup barrier per frame.  The workgroup has
 *    threads = min(JSGX_VITERBI_THREADS, S*G rounded up to 64) lanes, G = the largest power of two <= 64 with S*G <=
 *    JSGX_VITERBI_THREADS (1 where there is none): G lanes of one wavefront share a destination j, lane g of them takes the
 *    sources lo + g, lo + g + G, ... (lo = the first source of j), and the G partial (w, i) are reduced with the pair rule by lane
 *    moves (xor 1, 2, ..., G/2); by the paragraph on the rule the result is the one above.  Where S > JSGX_VITERBI_THREADS a lane
 *    owns the destinations j and j + JSGX_VITERBI_THREADS.  V[t-1][i] is an LDS broadcast, A(i, j) for consecutive j is consecutive words, and
 *    b[t+1][.] is loaded while frame t computes.  psi goes to the scratch as uint16.  The four forms are one templated kernel:
 *      "viterbi_dense_lds"   dense, S <= JSGX_VITERBI_LDS_STATES: A staged once in LDS.         LDS bytes: 4 (S*S + 2 S)   (192: 148992)
 *      "viterbi_dense_mem"   dense, larger S: A (at most 16 MiB) re-read every frame through L2 and the Infinity Cache.   8 S
 *      "viterbi_band_lds"    band, 4 ((2W+1) S + 2 S) <= 163840: the band table staged once in LDS.   4 ((2W+1) S + 2 S)
 *      "viterbi_band_mem"    band, where that does not fit: the table re-read from memory.            8 S
 *    The backtrace is blocked over B = JSGX_VITERBI_BLOCK frames, n_blocks = ceil(T / B); block k ends at the frame
 *    L_k = min((k+1) B, T) - 1.  "viterbi_jump" (seqs x blocks 1.., left out where n_blocks = 1): for every state s at L_k it follows psi
 *    down to the state at L_(k-1): jump[k][s], uint16 in the scratch; all states and blocks in parallel.  "viterbi_ends" (a workgroup per
 *    sequence): e and logp by the pair rule, then end[n_blocks-1] = e, end[k-1] = jump[k][end[k]]: T / B dependent steps.
 *    "viterbi_trace" (seqs x blocks, a lane per block): from end[k] it walks its own frames and writes states.  Every psi value is
 *    below S by construction and every loop is bounded by T or B.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_TRANS_DENSE 0
#define JSGX_TRANS_BAND 1
#define JSGX_VITERBI_MAX_STATES 2048
#define JSGX_VITERBI_MAX_FRAMES 1048576    /* 2^20 */
#define JSGX_VITERBI_MAX_BAND_HALF 64
#define JSGX_VITERBI_LDS_STATES 192        /* dense with A in LDS: 4 * (192 * 192 + 2 * 192) = 148992 bytes, inside 160 KiB */
#define JSGX_VITERBI_THREADS 1024          /* the most lanes of a forward workgroup */
#define JSGX_VITERBI_LDS_LIMIT 163840
/* The block of the backtrace was chosen among 64, 256 and 1024 by measurement on an MI355X at T = 65536 (profiles/viterbi_bench.md). */
#ifndef JSGX_VITERBI_BLOCK                 /* tools/viterbi_bench.py builds the other two for the comparison */
#define JSGX_VITERBI_BLOCK 256
#endif

typedef struct jsgx_viterbi_args {
    const float* log_emit;      /* device floats: b[q][t][s] */
    int64_t emit_frame_pitch;   /* >= n_states */
    int64_t emit_seq_pitch;     /* seqs > 1: >= (n_frames - 1) * emit_frame_pitch + n_states */
    const float* log_init;      /* device floats [n_states] */
    const float* trans;         /* device floats: dense [n_states][trans_pitch], band [2 * band_half + 1][trans_pitch] */
    int64_t trans_pitch;        /* >= n_states */
    int32_t trans_form;         /* JSGX_TRANS_DENSE or JSGX_TRANS_BAND */
    int32_t band_half;          /* W: 0 with the dense form, 0..JSGX_VITERBI_MAX_BAND_HALF with the band form */
    int32_t seqs;               /* 1..65535, independent */
    int32_t n_states;           /* S, 1..JSGX_VITERBI_MAX_STATES */
    int32_t n_frames;           /* T, 1..JSGX_VITERBI_MAX_FRAMES */
    int32_t reserved0;          /* 0 */
    int32_t* states;            /* device int32: states[q][t] at states[q*states_pitch + t] */
    int64_t states_pitch;       /* seqs > 1: >= n_frames */
    float* logp;                /* device floats [seqs] or NULL */
    float* value;               /* device floats or NULL: V[q][t][s] at value[q*value_seq_pitch + t*value_frame_pitch + s] */
    int64_t value_frame_pitch;  /* value given: >= n_states */
    int64_t value_seq_pitch;    /* value given and seqs > 1: >= (n_frames - 1) * value_frame_pitch + n_states */
} jsgx_viterbi_args;            /* 8-byte members and pairs of 4-byte ones: 120 bytes, no padding */

/* The bytes of scratch the launch needs, with n_blocks = ceil(T / JSGX_VITERBI_BLOCK):
 *     4 * seqs * S  (V[T-1])  +  4 * seqs * n_blocks  (end)  +  2 * seqs * T * S  (psi)  +  2 * seqs * n_blocks * S  (jump),
 * rounded up to a multiple of 4, in this order.  Refused (a negative jsgx_status): what the launch refuses before it looks at the scratch. */
JSGX_API int64_t jsgx_viterbi_scratch_bytes(const jsgx_viterbi_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  The kernels (forward, jump where
 * T > JSGX_VITERBI_BLOCK, ends, trace) go onto the one stream as a plain chain.  The scratch is used only while they run.  Refused
 * (JSGX_ERR_INVALID, nothing enqueued), in this order and before any device call: null args, a null log_emit, a null log_init, a null
 * trans, a null states; a pointer that is not 4-byte aligned; seqs outside 1..65535, n_states outside 1..2048, n_frames outside
 * 1..2^20; a trans_form other than the two; a non-zero band_half with the dense form, a band_half outside 0..64 with the band form; a
 * non-zero reserved0; emit_frame_pitch below n_states, emit_seq_pitch that does not cover a sequence (seqs > 1), trans_pitch below
 * n_states, states_pitch below n_frames (seqs > 1), value_frame_pitch below n_states (value given), value_seq_pitch that does not
 * cover a sequence (value given, seqs > 1); an output (states, logp, value) overlapping log_emit, one overlapping log_init, one
 * overlapping trans, an output overlapping another output; a null scratch, a scratch that is not 4-byte aligned, scratch_bytes below
 * jsgx_viterbi_scratch_bytes.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_viterbi_launch(const jsgx_viterbi_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the form of the forward kernel (above), the lanes of its workgroup, the bytes of LDS
 * it holds (dynamic; <= JSGX_VITERBI_LDS_LIMIT) and the number of kernels (3 where T <= JSGX_VITERBI_BLOCK, else 4).  Any output
 * pointer may be NULL (name: else name_len >= 24).  Refused: a name_len below 24 with a name, then what the scratch size refuses. */
JSGX_API int jsgx_viterbi_plan(const jsgx_viterbi_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches);
/* A locally normalised band transition on the host (no device; librosa.sequence.transition_local with a given window): for every
 * source i the weights are window[j - i + W] over the j = max(0, i-W)..min(S-1, i+W); their sum is taken in double, j ascending;
 * out[(i - j + W)*out_pitch + j] = (float)log(weight / sum), the logarithm in double and rounded once; a zero weight gives -inf.
 * The entries whose source lies outside the matrix are written as -inf (the launch never reads them).  out has 2W+1 rows of out_pitch.
 * JSGX_ERR_INVALID, in this order: a null window, a null out; n_states outside 1..2048; band_half outside 0..64; a window entry that is
 * negative or not finite; window[W] <= 0 (so that no row sums to zero); out_pitch below n_states. */
JSGX_API int jsgx_viterbi_band_build(int32_t n_states, int32_t band_half, const double* window, float* out, int64_t out_pitch);

#ifdef __cplusplus
}
#endif
#endif /* JSGX_H */
