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

/* Section 5 was added to version 1 in the same way: sections 1 to 4, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 5. pYIN (Mauch and Dixon 2014; librosa.pyin): from the d' plane of jsg_yin_launch (include/jsg.h section 2i, its cmnd output) to
 *    the emissions of a hidden Markov model over P pitch bins x {voiced, unvoiced}, and the decoding of that model with its
 *    transition in factored form.  The state s = u P + p, u = 0 voiced and u = 1 unvoiced, p the pitch bin: librosa's order.  A row
 *    (a sequence) is one signal; rows and frames are independent in the observation, sequences in the decoder.  All device arithmetic
 *    is float32 and uncontracted; fl(.) is one rounding to float32; the divides are correctly rounded.  Nothing depends on the number
 *    of rows, on the pitches, on which optional outputs are NULL or on the form of a kernel.
 *
 *    5a. The tables, built on the host in double and rounded to float32 once (no device).
 *      prior (jsgx_pyin_prior_build):  out[k] = I((k+1)/N; a, b) - I(k/N; a, b), k = 0..N-1, I the regularised incomplete beta function
 *        (its continued fraction by Lentz's method on the side x < (a+1)/(a+b+2), the other side by symmetry, the front factor from
 *        lgamma).  librosa: np.diff(beta.cdf(linspace(0, 1, N+1), a, b)) with (a, b) = (2, 18), N = 100.
 *      decay, norm (jsgx_pyin_boltzmann_build):  decay[i] = exp(-lambda i), i = 0..n-1;  norm[0] = 0, norm[m] = (1 - exp(-lambda)) /
 *        (1 - exp(-lambda m)), m = 1..n.  The truncated Boltzmann pmf of the position i among m troughs is norm[m] * decay[i].
 *      edges, freqs (jsgx_pyin_bins_build):  freqs[b] = fmin 2^(b / (12 bps)), b = 0..P-1;  edges[b] = sample_rate / (fmin 2^((b - 0.5) /
 *        (12 bps))), b = 0..P: a descending table of PERIODS.  The device finds a candidate's bin by comparing with this table and takes
 *        no logarithm, so the bin is reproducible bit for bit.
 *      log_window, src_offset, log_switch (jsgx_pyin_transition_build):  log_window[k] = log(window[k]), -inf for 0, k = 0..2W;
 *        src_offset[p] = -log(the sum of window[p' - p + W] over p' = max(0, p-W)..min(P-1, p+W), p' ascending): the local normalisation
 *        of jsgx_viterbi_band_build kept as a term of the source;  log_switch[2u + u'] = log(u == u' ? 1 - switch_prob : switch_prob),
 *        -inf for 0.
 *
 *    5b. The observation (jsgx_pyin_observe_launch).  Per frame, with h[tau] = d'[tau] = cmnd[r*cmnd_row_pitch + t*cmnd_frame_pitch + tau]:
 *      1. Troughs.  tau_min is a trough iff h[tau_min] < h[tau_min+1];  tau_min < tau < tau_max iff h[tau-1] > h[tau] <= h[tau+1];  tau_max
 *         never is, and with tau_min == tau_max there is none.  No two neighbouring lags are troughs: there are at most
 *         (tau_max - tau_min + 1) / 2 of them (integer division).  Trough j = 0, 1, ... in ascending lag order, h_j = h[tau_j].
 *      2. Thresholds.  th_k = (float)((k+1) / (double)N), k = 0..N-1.  Trough j lies below threshold k iff h_j < th_k (strict), so for all
 *         k >= k0(j), k0(j) = N where there is none.  n_k = the number of troughs below threshold k;  pos_jk = the number of troughs i < j
 *         below threshold k (the rank of j among them by ascending lag, from 0).
 *      3. Probability.  term_jk = fl(prior[k] * fl(norm[n_k] * decay[pos_jk])) for k >= k0(j), +0 for k < k0(j).  The sum over k is the lane
 *         sum of 64 lanes: lane l adds term_jk for k = l, l+64, l+128, l+192 (those below N) ascending with plain adds from +0; then a
 *         halving tree: for m = 32, 16, ..., 1:  acc_l = acc_l + acc_(l+m) for l < m;  prob_j = acc_0.  The lowest trough g (the lowest h_j,
 *         the lowest lag among equal ones) gets in addition:  prob_g = fl(prob_g + fl(no_trough_prob * q)), q = the same lane sum of
 *         (k < k0(g) ? prior[k] : +0).
 *      4. Period and bin.  a, b, c = h[tau_j - 1], h[tau_j], h[tau_j + 1];  den = (a - b) + (c - b);  if den > 0:  s = (0.5f * (a - c)) / den,
 *         kept if |s| <= 1, else 0; in every other case (a NaN h[tau_min - 1] included) s = 0:  step 4 of jsg.h section 2i.
 *         period_j = (float)tau_j + s.  bin_j = the number of b in 1..P-1 with period_j <= edges[b]: a period above edges[1] is in bin 0,
 *         one at or below edges[P-1] in bin P-1, so both ends are clamped (edges[0] and edges[P] are the outer rims and are not read).  The
 *         kernel finds the number by bisection, which is that number for a descending table; for any other table it is some bin in 0..P-1.
 *      5. Accumulation.  obs[b] = the sum of prob_j over the troughs with bin_j = b, in ascending lag order with plain adds from +0.
 *         total = the lane sum of 64 lanes of obs[b] (lane l adds b = l, l+64, ... ascending from +0, then the halving tree above);
 *         voiced = 1 where total > 1, else total;  unv = fl(fl(1 - voiced) / (float)P).
 *      6. Emissions.  log_emit[p] = L(obs[p]);  log_emit[P + p] = L(unv), p = 0..P-1, at log_emit[r*emit_row_pitch + t*emit_frame_pitch + s].
 *         obs[r][t][p] and voiced_prob[r][t] = voiced where these are given.
 *      7. NaN.  If any h[tau], tau_min <= tau <= tau_max, is a NaN the frame is unobserved: obs = +0, voiced_prob = NaN, the voiced emissions
 *         are -inf and the unvoiced ones L(fl(1 / (float)P)).  No other frame is touched, and the decoder goes through such a frame.
 *
 *      L(x), the natural logarithm from plain float32 adds and multiplies and one divide, no fmaf, no hardware logarithm (the reduction
 *      and the polynomial of the freely available fdlibm e_logf.c, evaluated in this order):
 *          x == 0: -inf;   x < 0 or a NaN: NaN;   x == +inf: +inf
 *          k = 0;   x < 2^-126:  x = x * 2^24 (exact), k = -24
 *          i = (the bits of x) + 0x004afb0d;   k = k + (i >> 23) - 127;   m = the float with the bits (i & 0x007fffff) + 0x3f3504f3
 *              (x = m 2^k, sqrt(1/2) <= m < sqrt(2))
 *          f = m - 1;   s = f / (2 + f);   z = s * s;   w = z * z
 *          t1 = w * (0.40000972152 + w * 0.24279078841);   t2 = z * (0.66666662693 + w * 0.28498786688)        (floats: 0xccce13p-25,
 *              0xf89e26p-26, 0xaaaaaap-24, 0x91e9eep-25; every product and sum rounded)
 *          r = t2 + t1;   hfsq = (0.5f * f) * f;   dk = (float)k
 *          L = (((s * (hfsq + r) + dk * 9.0580006145e-06f) - hfsq) + f) + dk * 6.9313812256e-01f          (ln 2 = hi + lo)
 *      L(1) = +0.  |L(x) - ln x| <= JSGX_LOG_ABS_BOUND * max(1, |ln x|) over every float32 x in (0, 1] against log in double (measured:
 *      profiles/pyin_accuracy.md).
 *
 *      Known answers.  A silent frame (d' = 1 everywhere) has no trough: obs = +0, voiced_prob = +0, unv = fl(1 / (float)P), the voiced
 *      emissions are -inf.  A frame whose only trough has h >= 1 lies below no threshold (th_(N-1) = 1): prob = +0 + fl(no_trough_prob *
 *      (the lane sum of prior)) goes into that trough's bin and nothing else.
 *      Error bound, for tables that are >= 0, against exact arithmetic on the same float32 tables and the same troughs, bins and
 *      thresholds, u = 2^-24: a term carries two roundings, the lane sum of at most 4 + 6 additions of non-negative numbers ten more, the
 *      no-trough part at most 12 and one more for its addition, the sum into obs[b] one per trough of the bin: obs[b] is relative
 *      (13 + c_b) u to first order, c_b the troughs of bin b after the first (0 where the bins do not collide); against a float64 evaluation
 *      with unrounded tables three more (prior, norm, decay): tests/test_pyin_ref.py asserts 18 u on frames without collisions.  voiced adds ceil(P / 64) + 6 roundings.
 *      Differences from librosa.pyin, on purpose: candidates that fall into one bin add (librosa's fancy assignment keeps the last);
 *      both ends of the bin index clamp (librosa clips to P, which lands in the unvoiced half and is overwritten); the parabola is
 *      section 2i's; the troughs are defined on d' above.  Agreement with librosa has not been measured.
 *      The kernel ("pyin_observe"): one wavefront per frame (a workgroup of JSGX_PYIN_OBSERVE_THREADS lanes, one frame per workgroup),
 *      nobody waits for anybody.  d' of the frame is staged in LDS; the troughs are packed by a ballot; a lane owns four thresholds; the
 *      troughs are met in lag order, each with one xor tree over the lanes.  LDS: 4 (tau_max + 1 + 3 (max troughs + 1) + P) bytes.
 *
 *    5c. The decoder (jsgx_pyin_decode_launch).  Inputs as section 4: b[t][s] = log_emit[q*emit_seq_pitch + t*emit_frame_pitch + s],
 *      S = 2P states; p0 = log_init[2P]; the transition is A((u, p), (u', p')) = src_offset[p] + log_window[p' - p + W] + log_switch[2u + u']
 *      for |p - p'| <= W = band_half, and only these sources exist.
 *      Recurrence.  V[0][s] = fl(p0[s] + b[0][s]).  For t >= 1:
 *          U[u][p] = fl(V[t-1][uP + p] + src_offset[p])
 *          for every p' and u, over p = max(0, p'-W)..min(P-1, p'+W):   w(p) = fl(U[u][p] + log_window[p' - p + W]), a NaN counted as -inf;
 *              p*_u = the p with the largest w, the lowest p among equal w;   m_u = w(p*_u)
 *          for every u':   c_u = fl(m_u + log_switch[2u + u']), a NaN counted as -inf;   the winner is the larger c_u, u = 0 on ties;
 *              psi[t][u'P + p'] = uP + p*_u;     V[t][u'P + p'] = fl(c_u + b[t][u'P + p'])
 *      The selection over p is the pair rule of section 4, so it does not depend on how the lanes split the sources.  End, backtrace,
 *      outputs (states, logp, value), the meaning of logp = -inf and the NaN rules are section 4's with S = 2P, and the backtrace is
 *      section 4's three kernels.
 *      Against section 4 on the dense matrix A: the same maximisation, with the three terms of A added to V in another association.
 *      Where every sum is exact (multiples of 1/8 in a small range) and every destination has a source above -inf the two give the same
 *      bits; where all sources of a destination are -inf the lowest source inside the pitch band wins here, u = 0 and p = max(0, p'-W).
 *      Known answers.  All inputs +0: every w ties, V = +0, psi[t][u'P + p'] = max(0, p'-W), e = 0, the states are all 0 and logp = +0.
 *      A frame whose emissions are all -inf: logp = -inf with JSGX_OK.
 *      Error bound, for finite inputs that are all <= 0, u = 2^-24: as section 4, with four same-sign additions per frame instead of two
 *      (U, w, c, V): logp carries at most 4T - 3 roundings, inside (4T + 2) u relative for T <= 4096, which tests/test_pyin_ref.py
 *      asserts against float64.
 *      The kernel ("pyin_decode"): one workgroup per sequence, nobody waits across workgroups.  U of both u lies in LDS, two copies
 *      swapped by the parity of t, every row padded with W words of -inf at both ends: the inner loop has no bounds test.  m_0 and m_1
 *      are computed once per p' and serve both u'.  G lanes of one wavefront share a p' and take the offsets g, g + G, ...; they are
 *      joined with the pair rule by xor lane moves.  G = the largest power of two <= 64 with 8 G <= 2W + 1 (a lane has eight offsets
 *      at the least) and P*G <= 512, 1 where there is none; the workgroup has P*G lanes rounded up to 64.  The rule was chosen by
 *      measurement (profiles/pyin_bench.md): with as many lanes per bin as 1024 lanes hold, the joins cost more than the split saves.  U of frame t is
 *      written where V[t] is: one barrier per frame.  U is kept as pairs (U[0][p], U[1][p]) that a lane reads 8 bytes at a time.  The
 *      emissions of frame t + 1 are loaded while frame t computes.  psi is uint16 in the scratch in section 4's layout.  LDS: 4 (4 (P + 2W) + 2W + 1) bytes.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_PYIN_MAX_BINS 1024
#define JSGX_PYIN_MAX_BAND_HALF 128
#define JSGX_PYIN_MAX_THRESHOLDS 256
#define JSGX_PYIN_MAX_LAG 4096
#define JSGX_PYIN_OBSERVE_THREADS 64
#define JSGX_PYIN_THREADS 1024             /* the most lanes of a forward workgroup of the decoder */
#define JSGX_LOG_ABS_BOUND 1.0e-7          /* L against log in double over every float32 in (0, 1] (measured 8.07e-8: profiles/pyin_accuracy.md) */

/* out[k], k = 0..n_thresholds-1 (5a).  JSGX_ERR_INVALID, in this order: a null out; n_thresholds outside 1..256; a or b not finite and > 0. */
JSGX_API int jsgx_pyin_prior_build(int32_t n_thresholds, double a, double b, float* out);
/* decay[0..n-1] and norm[0..n] (5a).  JSGX_ERR_INVALID, in this order: a null decay, a null norm; lambda not finite and > 0; n outside
 * 1..JSGX_PYIN_MAX_LAG. */
JSGX_API int jsgx_pyin_boltzmann_build(double lambda, int32_t n, float* decay, float* norm);
/* edges[0..n_bins] and freqs[0..n_bins-1] (5a).  JSGX_ERR_INVALID, in this order: a null edges, a null freqs; sample_rate not finite and
 * > 0; fmin not finite and > 0; bins_per_semitone outside 1..1024; n_bins outside 1..JSGX_PYIN_MAX_BINS. */
JSGX_API int jsgx_pyin_bins_build(double sample_rate, double fmin, int32_t bins_per_semitone, int32_t n_bins, float* edges, float* freqs);
/* log_window[0..2W], src_offset[0..n_bins-1], log_switch[0..3] (5a).  JSGX_ERR_INVALID, in this order: a null window, a null log_window,
 * a null src_offset, a null log_switch; n_bins outside 1..1024; band_half outside 0..JSGX_PYIN_MAX_BAND_HALF; a window entry that is
 * negative or not finite; window[W] <= 0; switch_prob outside [0, 1]. */
JSGX_API int jsgx_pyin_transition_build(int32_t n_bins, int32_t band_half, const double* window, double switch_prob, float* log_window, float* src_offset,
                                        float* log_switch);

typedef struct jsgx_pyin_observe_args {
    const float* cmnd;          /* device floats: d'[r][t][tau] at cmnd[r*cmnd_row_pitch + t*cmnd_frame_pitch + tau], tau = 0..tau_max */
    int64_t cmnd_frame_pitch;   /* >= tau_max + 1 */
    int64_t cmnd_row_pitch;     /* rows > 1: >= (n_frames - 1) * cmnd_frame_pitch + tau_max + 1 */
    int32_t rows;               /* 1..65535, independent */
    int32_t n_frames;           /* 1..JSGX_VITERBI_MAX_FRAMES */
    int32_t tau_min;            /* 1..tau_max */
    int32_t tau_max;            /* 1..JSGX_PYIN_MAX_LAG */
    const float* prior;         /* device floats [n_thresholds] */
    const float* decay;         /* device floats [boltz_len] */
    const float* norm;          /* device floats [boltz_len + 1] */
    const float* edges;         /* device floats [n_bins + 1], descending */
    int32_t n_thresholds;       /* N, 1..JSGX_PYIN_MAX_THRESHOLDS */
    int32_t boltz_len;          /* max(1, (tau_max - tau_min + 1) / 2)..JSGX_PYIN_MAX_LAG: the most troughs of a frame at the least */
    int32_t n_bins;             /* P, 1..JSGX_PYIN_MAX_BINS */
    float no_trough_prob;       /* in [0, 1] */
    float* log_emit;            /* device floats: [r][t][2P] at log_emit[r*emit_row_pitch + t*emit_frame_pitch + s] */
    int64_t emit_frame_pitch;   /* >= 2 * n_bins */
    int64_t emit_row_pitch;     /* rows > 1: >= (n_frames - 1) * emit_frame_pitch + 2 * n_bins */
    float* obs;                 /* device floats or NULL: [r][t][P] at obs[r*obs_row_pitch + t*obs_frame_pitch + p] */
    int64_t obs_frame_pitch;    /* obs given: >= n_bins */
    int64_t obs_row_pitch;      /* obs given and rows > 1: >= (n_frames - 1) * obs_frame_pitch + n_bins */
    float* voiced_prob;         /* device floats or NULL: [r][t] at voiced_prob[r*voiced_pitch + t] */
    int64_t voiced_pitch;       /* voiced_prob given and rows > 1: >= n_frames */
} jsgx_pyin_observe_args;       /* 152 bytes, no padding */

/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; capture works, a first launch included.  Refused
 * (JSGX_ERR_INVALID, nothing enqueued), in this order and before any device call: null args, a null cmnd, a null prior, a null decay, a
 * null norm, a null edges, a null log_emit; a pointer that is not 4-byte aligned; rows outside 1..65535, n_frames outside 1..2^20,
 * tau_max outside 1..4096, tau_min outside 1..tau_max, n_thresholds outside 1..256, n_bins outside 1..1024, boltz_len outside
 * max(1, (tau_max - tau_min + 1) / 2)..4096, no_trough_prob outside [0, 1]; cmnd_frame_pitch below tau_max + 1, cmnd_row_pitch that does
 * not cover a row (rows > 1), emit_frame_pitch below 2 * n_bins, emit_row_pitch that does not cover a row (rows > 1), obs_frame_pitch
 * below n_bins (obs given), obs_row_pitch that does not cover a row (obs given, rows > 1), voiced_pitch below n_frames (voiced_prob
 * given, rows > 1); an output (log_emit, obs, voiced_prob) overlapping cmnd, one overlapping prior, decay, norm, edges in this order,
 * an output overlapping another output.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_pyin_observe_launch(const jsgx_pyin_observe_args* args, void* stream);
/* The kernel of these arguments, without a device: its name ("pyin_observe"), the lanes of a workgroup, the bytes of LDS it holds
 * (dynamic, <= 65536) and the frames a workgroup takes (1).  Any output pointer may be NULL (name: else name_len >= 16).  Refused: a
 * name_len below 16 with a name, then what the launch refuses. */
JSGX_API int jsgx_pyin_observe_plan(const jsgx_pyin_observe_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes,
                                    int32_t* frames_per_workgroup);

typedef struct jsgx_pyin_decode_args {
    const float* log_emit;      /* device floats: b[q][t][s], s = u*n_bins + p */
    int64_t emit_frame_pitch;   /* >= 2 * n_bins */
    int64_t emit_seq_pitch;     /* seqs > 1: >= (n_frames - 1) * emit_frame_pitch + 2 * n_bins */
    const float* log_init;      /* device floats [2 * n_bins] */
    const float* log_window;    /* device floats [2 * band_half + 1] */
    const float* src_offset;    /* device floats [n_bins] */
    const float* log_switch;    /* device floats [4] */
    int32_t n_bins;             /* P, 1..JSGX_PYIN_MAX_BINS */
    int32_t band_half;          /* W, 0..JSGX_PYIN_MAX_BAND_HALF */
    int32_t seqs;               /* 1..65535, independent */
    int32_t n_frames;           /* T, 1..JSGX_VITERBI_MAX_FRAMES */
    int32_t* states;            /* device int32: states[q][t] at states[q*states_pitch + t] */
    int64_t states_pitch;       /* seqs > 1: >= n_frames */
    float* logp;                /* device floats [seqs] or NULL */
    float* value;               /* device floats or NULL: V[q][t][s] at value[q*value_seq_pitch + t*value_frame_pitch + s] */
    int64_t value_frame_pitch;  /* value given: >= 2 * n_bins */
    int64_t value_seq_pitch;    /* value given and seqs > 1: >= (n_frames - 1) * value_frame_pitch + 2 * n_bins */
} jsgx_pyin_decode_args;        /* 120 bytes, no padding */

/* The bytes of scratch the launch needs: the formula of jsgx_viterbi_scratch_bytes with S = 2 * n_bins.  Refused (a negative jsgx_status):
 * what the launch refuses before it looks at the scratch. */
JSGX_API int64_t jsgx_pyin_decode_scratch_bytes(const jsgx_pyin_decode_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  The kernels (forward, then section 4's jump
 * where T > JSGX_VITERBI_BLOCK, ends, trace) go onto the one stream as a plain chain.  Refused (JSGX_ERR_INVALID, nothing enqueued), in
 * this order and before any device call: null args, a null log_emit, a null log_init, a null log_window, a null src_offset, a null
 * log_switch, a null states; a pointer that is not 4-byte aligned; seqs outside 1..65535, n_bins outside 1..1024, band_half outside
 * 0..128, n_frames outside 1..2^20; emit_frame_pitch below 2 * n_bins, emit_seq_pitch that does not cover a sequence (seqs > 1),
 * states_pitch below n_frames (seqs > 1), value_frame_pitch below 2 * n_bins (value given), value_seq_pitch that does not cover a
 * sequence (value given, seqs > 1); an output (states, logp, value) overlapping log_emit, one overlapping log_init, log_window,
 * src_offset, log_switch in this order, an output overlapping another output; a null scratch, a scratch that is not 4-byte aligned,
 * scratch_bytes below jsgx_pyin_decode_scratch_bytes.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_pyin_decode_launch(const jsgx_pyin_decode_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the name of the forward kernel ("pyin_decode"), G (the lanes that share a pitch bin), the
 * lanes of its workgroup, the bytes of LDS it holds (dynamic, <= 65536) and the number of kernels (3 where T <= JSGX_VITERBI_BLOCK, else
 * 4).  Any output pointer may be NULL (name: else name_len >= 16).  Refused: a name_len below 16 with a name, then what the scratch
 * size refuses. */
JSGX_API int jsgx_pyin_decode_plan(const jsgx_pyin_decode_args* args, char* name, int name_len, int32_t* lanes_per_bin, int32_t* threads, int32_t* lds_bytes,
                                   int32_t* n_launches);

/* Sections 6 to 8 were added to version 1 in the same way: sections 1 to 5, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 6. The k nearest frames (the selection behind librosa.segment.recurrence_matrix and cross_similarity): for every frame i of x the k
 *    frames j of y with the lowest cost, without the N x M plane ever reaching memory.  x, y, their pitches, pairs, n_features, n, m and
 *    metric are those of jsgx_cdist_args with the same limits; a pair pitch of 0 is a shared sequence; c(i, j) is the cost of section 2
 *    bit for bit: the same k-ascending fmaf chain per output.
 *
 *    Definition.  The candidates of row i are the j in 0..M-1 with |i - j| >= width and c(i, j) not a NaN (width 0 excludes nothing,
 *    width 1 only the main diagonal, as in librosa).  They are ordered by the key (c, j): the float comparison on c, so -0 == +0, then
 *    the lower j: a total order, the j being distinct.  With cnt = min(k, the number of candidates):
 *        nn_index[p*index_pair_pitch + i*index_pitch + r], nn_dist[p*dist_pair_pitch + i*dist_pitch + r], r < cnt:  j and c(i, j) of the
 *        cnt smallest candidates in that order;   r = cnt..k-1:  index -1 and distance +inf.
 *    A +inf cost is a candidate like any other.  Nothing behind entry k-1 of a row is written.  The result is a set of exact
 *    comparisons on section 2's costs: it does not depend on pairs, on the pitches, on split or on how the kernel finds it.
 *
 *    Against librosa.  librosa takes the k + 2 width nearest of every frame from sklearn's NearestNeighbors, drops the band |i - j| <
 *    width from them and keeps the nearest k of the rest.  A band holds at most 2 width - 1 frames, so the k nearest outside the band
 *    are among the k + 2 width nearest of all: the two selections are the same set in the same order wherever the costs are distinct.
 *    The differences: ties go to the lower j here (sklearn: whatever its partial sort leaves); a NaN cost is no candidate here (sklearn
 *    refuses NaN input); a zero vector under the cosine metric costs 1 as in section 2 (scipy: NaN); the costs are section 2's float32
 *    chain (sklearn: float64, euclidean by the expanded form); k is at most JSGX_KNN_MAX_K: a larger k is out of scope.  Agreement with
 *    librosa has not been measured: librosa is not installed where this was built.
 *
 *    The kernel ("knn_64"): a workgroup of JSGX_KNN_THREADS lanes owns a strip of JSGX_KNN_STRIP rows of one pair and sweeps its column
 *    tiles of JSGX_KNN_TILE columns in ascending order with the inner loop of "cdist_64x64": the same staging, the same order.  Each
 *    tile of costs is dropped into the LDS the panels have left (64 rows of 68 words).  Every row keeps its running sorted list in LDS:
 *    k float costs and k 16-bit indices (M <= 65536), 6 k bytes a row.  A wavefront serves 16 rows of the strip; its lane l holds
 *    candidate j0 + l of the row.  A candidate survives if the list is not full or c is below the k-th cost, as the row's last merge
 *    left it and as the row keeps it in a word of its own (an equal cost loses: every j of the list is lower).  A tile whose 64 candidates of a row all fail costs one ballot and nothing else.  Survivors are appended
 *    (a prefix count over the ballot) to the row's 64 pending places in LDS and merged only when the next tile's survivors no longer fit,
 *    and at the end of the sweep: a merge serves up to 64 survivors instead of a tile's few, and a survivor that a later, lower k-th cost
 *    has overtaken falls away in the merge.  The merge is by rank: a candidate's rank among the candidates is counted with lane reads (equal
 *    costs: the earlier, which has the lower j) and their costs are laid down sorted; a candidate's place is its rank + the list entries
 *    with cost <= its own (bisection of the list), a list entry's place is its index + the candidates with cost < its own (bisection of
 *    the candidates); places >= k fall away.  The places are a permutation, so every lane reads first and writes afterwards, with no second
 *    copy of the list.
 *    LDS: JSGX_KNN_LDS_STATIC + 6 * JSGX_KNN_STRIP * k bytes (the second part dynamic), 142080 at k = 256, inside 160 KiB.
 *    Column splits.  T = ceil(M / 64) column tiles are divided among S = min(split, T) workgroups per strip, workgroup s taking the tiles
 *    floor(s T / S) .. floor((s + 1) T / S) - 1.  S = 1 writes the outputs; S > 1 writes partial lists (cost and int32 index, 8 k S bytes
 *    a row) to the scratch and "knn_merge" (one wavefront per row, the same merge by rank over the S lists in ascending s) writes the
 *    outputs.  Selecting the k smallest of a total order is associative: the outputs are the same bits for every split.  split = 0 is
 *    automatic: the smallest S in {1, 2, 4, 8, 16} with pairs * ceil(N / 64) * S >= the compute units of the device; where there is none,
 *    or a workgroup would be left without a tile, the largest S of the set that is <= T.
 *    The accumulation order is stated, so this runs on the vector pipe, not on MFMA.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_KNN_MAX_K 256
#define JSGX_KNN_MAX_SPLIT 16
#define JSGX_KNN_STRIP 64
#define JSGX_KNN_TILE 64
#define JSGX_KNN_THREADS 256
#define JSGX_KNN_LDS_STATIC 43776          /* the panels and then the tile 17408, 64 pending survivors a row 24576, the sorted costs of four merges 1024, lengths and k-th costs 768 */
#define JSGX_KNN_LDS_LIMIT 163840
#define JSGX_KNN_MERGE_THREADS 256         /* "knn_merge": four rows a workgroup */

typedef struct jsgx_knn_args {
    const float* x;             /* device floats, as jsgx_cdist_args */
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
    int32_t k;                  /* 1..JSGX_KNN_MAX_K */
    int32_t width;              /* >= 0 */
    int32_t split;              /* 0 (automatic), or 1..JSGX_KNN_MAX_SPLIT */
    int32_t* nn_index;          /* device int32: [p][i][r] */
    int64_t index_pitch;        /* >= k */
    int64_t index_pair_pitch;   /* pairs > 1: >= (n - 1) * index_pitch + k */
    float* nn_dist;             /* device floats: [p][i][r] */
    int64_t dist_pitch;         /* >= k */
    int64_t dist_pair_pitch;    /* pairs > 1: >= (n - 1) * dist_pitch + k */
} jsgx_knn_args;                /* 128 bytes, no padding */

/* The bytes of scratch the launch needs: 8 * pairs * n * k * S for the partial lists where S > 1, else 0; S = min(split, ceil(m / 64)),
 * and for split = 0 the largest S the automatic rule can give (the largest of 1, 2, 4, 8, 16 that is <= ceil(m / 64)), since the device is not asked here.  Refused (a
 * negative jsgx_status): what the launch refuses before it looks at the scratch. */
JSGX_API int64_t jsgx_knn_scratch_bytes(const jsgx_knn_args* args);
/* Enqueue only ("knn_64", then "knn_merge" where S > 1): no allocation, no synchronisation; capture works, a first launch included.
 * The scratch is used only while the kernels run.  Refused (JSGX_ERR_INVALID, nothing enqueued), in this order and before any device
 * call: null args, a null x, a null y, a null nn_index, a null nn_dist; a pointer that is not 4-byte aligned; pairs outside 1..65535,
 * n_features outside 1..1024, n outside 1..65536, m outside 1..65536, a metric outside 0..2, k outside 1..256, a negative width, split
 * outside 0..16; x_frame_pitch below n_features, y_frame_pitch below n_features, a non-zero x_pair_pitch that does not cover a sequence,
 * the same for y_pair_pitch, index_pitch below k, index_pair_pitch that does not cover a plane (pairs > 1), dist_pitch below k,
 * dist_pair_pitch that does not cover a plane (pairs > 1); an output (nn_index, nn_dist) overlapping x, one overlapping y, nn_index
 * overlapping nn_dist; a null scratch, a scratch that is not 4-byte aligned, scratch_bytes below jsgx_knn_scratch_bytes (each only
 * where that size is not 0).  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_knn_launch(const jsgx_knn_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues on a device of n_cu compute units, without a device: the name of the forward kernel ("knn_64"), the rows of a
 * strip, S (as the launch resolves it: split = 0 by the automatic rule for n_cu), JSGX_KNN_THREADS and the bytes of LDS of a workgroup
 * (JSGX_KNN_LDS_STATIC + 384 k <= JSGX_KNN_LDS_LIMIT).  Any output pointer may be NULL (name: else name_len >= 16).  Refused: a name_len
 * below 16 with a name, then what the scratch size refuses, then an n_cu below 1. */
JSGX_API int jsgx_knn_plan(const jsgx_knn_args* args, int32_t n_cu, char* name, int name_len, int32_t* strip_rows, int32_t* split, int32_t* threads,
                           int32_t* lds_bytes);

/* ------------------------------------------------------------------------------------------------
 * 7. The dense recurrence plane from the lists of section 6 (librosa.segment.recurrence_matrix and cross_similarity, their modes):
 *    out[p*out_pair_pitch + i*out_pitch + j], i < N, j < M, float32.  list(i) = the entries r < k of row i of nn_index that lie in 0..M-1.
 *        link(i, j) holds where j is in list(i); with sym = 1 (refused unless n == m) i must also be in list(j): mutual neighbours,
 *        librosa's minimum(rec, rec.T).
 *        The value of a link, d = nn_dist of row i at the entry that holds j:
 *            JSGX_REC_CONNECTIVITY:  1.0f                                (nn_dist is not read and may be NULL)
 *            JSGX_REC_DISTANCE:      d
 *            JSGX_REC_AFFINITY:      jsgx_exp(-fl(d / bw)), bw = bandwidth[p] read on the device (nothing returns to the host): section 1's
 *                                    routine, restated on the device operation by operation; NaN where !(bw > 0) or d is a NaN.
 *                                    (A cosine cost a rounding below zero gives an argument a rounding above zero: the same operations.)
 *        Every other element is +0.  With diag = 1, out[i][i] (i < min(N, M)) is 1.0f in connectivity and affinity mode and 0.0f in
 *        distance mode, link or not.  Every element of the plane is written; nothing outside it is written.
 *    A list of section 6 holds every j at most once.  A list from elsewhere that holds a j twice gives one of the two values.
 *    Symmetry.  For x == y the costs of sections 2 and 6 are bitwise symmetric: for (sq)euclidean fl(a - b) = -fl(b - a) and the chain of
 *    squares is the same; for cosine the products commute.  So sym = 1 loses nothing by keeping row i's distance, and out is symmetric.
 *    Orientation.  Query-major: row i holds the neighbours of frame i.  librosa documents the transpose (rec[i, j] non-zero where i is a
 *    neighbour of j); with sym the two are the same.  Sparse outputs are out of scope: the lists are the sparse form.
 *    The kernel ("recurrence_rows"): a workgroup of JSGX_REC_THREADS lanes per row; the row is built in LDS in pieces of JSGX_REC_CHUNK
 *    columns (zeros, then the links of the piece, then the diagonal) and goes out as whole lines: every element is stored once.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_REC_CONNECTIVITY 0
#define JSGX_REC_DISTANCE 1
#define JSGX_REC_AFFINITY 2
#define JSGX_REC_THREADS 256
#define JSGX_REC_CHUNK 4096
#define JSGX_REC_LDS_BYTES 18432           /* static: the piece 16384, the row's list 256 x (index, value) */

typedef struct jsgx_recurrence_args {
    const int32_t* nn_index;    /* device int32: [p][i][r] */
    int64_t index_pitch;        /* >= k */
    int64_t index_pair_pitch;   /* pairs > 1: >= (n - 1) * index_pitch + k */
    const float* nn_dist;       /* device floats [p][i][r]; NULL allowed in connectivity mode */
    int64_t dist_pitch;         /* nn_dist given: >= k */
    int64_t dist_pair_pitch;    /* nn_dist given and pairs > 1: >= (n - 1) * dist_pitch + k */
    const float* bandwidth;     /* device floats [pairs]; affinity mode only, else not read and may be NULL */
    int32_t pairs;              /* 1..65535 */
    int32_t n;                  /* N, 1..JSGX_DTW_MAX_LEN */
    int32_t m;                  /* M, 1..JSGX_DTW_MAX_LEN */
    int32_t k;                  /* 1..JSGX_KNN_MAX_K */
    int32_t mode;               /* JSGX_REC_* */
    int32_t sym;                /* 0 or 1; 1 needs n == m */
    int32_t diag;               /* 0 or 1 */
    int32_t reserved0;          /* 0 */
    float* out;                 /* device floats: [p][i][j] */
    int64_t out_pitch;          /* >= m */
    int64_t out_pair_pitch;     /* pairs > 1: >= (n - 1) * out_pitch + m */
} jsgx_recurrence_args;         /* 112 bytes, no padding */

/* Enqueue only (one kernel, no scratch); capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing enqueued), in this
 * order and before any device call: null args, a null nn_index, a null out; a pointer that is not 4-byte aligned; pairs outside
 * 1..65535, n outside 1..65536, m outside 1..65536, k outside 1..256, a mode outside 0..2, sym other than 0 or 1, diag other than 0 or
 * 1; a non-zero reserved0; sym with n != m; a null nn_dist in distance or affinity mode, a null bandwidth in affinity mode;
 * index_pitch below k, index_pair_pitch that does not cover a plane (pairs > 1), the same for dist_pitch and dist_pair_pitch (nn_dist
 * given), out_pitch below m, out_pair_pitch that does not cover a plane (pairs > 1); out overlapping nn_index, out overlapping nn_dist,
 * out overlapping bandwidth.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_recurrence_launch(const jsgx_recurrence_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * 8. Neighbour aggregation of a plane (librosa.decompose.nn_filter with the mean or a weighted mean; square only: the neighbours of
 *    frame i are frames of the same plane).  S[j][f] = s[p*s_pair_pitch + j*s_frame_pitch + f], j < N, f < F, frame-major.  For row i
 *    let r ascend over the entries r < k of nn_index whose index is in 0..N-1, cnt their number:
 *        mean (weights NULL):  acc = fl(acc + S[idx][f]) from +0;   out[i][f] = fl(acc / (float)cnt)
 *        weighted:  w = weights[p*weights_pair_pitch + i*weights_pitch + r];   num = fmaf(w, S[idx][f], num);  den = fl(den + w), both
 *                   from +0;   out[i][f] = fl(num / den)
 *        a row with cnt == 0, or a weighted row with den == 0, takes S[i][f]: librosa's rule for a frame without neighbours.
 *    out[p*out_pair_pitch + i*out_frame_pitch + f]; nothing else is written.  The median aggregate (librosa's default) is out of scope.
 *    The kernel ("nn_filter_rows"): one wavefront per row; lane l takes the features l, l + 64, ...; the index and the weight of an
 *    entry are one broadcast read each, the reads of S run along f.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_NNF_MAX_FEATURES 65536
#define JSGX_NNF_THREADS 64

typedef struct jsgx_nn_filter_args {
    const float* s;             /* device floats: S[p][j][f] */
    int64_t s_frame_pitch;      /* >= n_features */
    int64_t s_pair_pitch;       /* pairs > 1: >= (n - 1) * s_frame_pitch + n_features */
    const int32_t* nn_index;    /* device int32: [p][i][r] */
    int64_t index_pitch;        /* >= k */
    int64_t index_pair_pitch;   /* pairs > 1: >= (n - 1) * index_pitch + k */
    const float* weights;       /* device floats [p][i][r], or NULL: the mean */
    int64_t weights_pitch;      /* weights given: >= k */
    int64_t weights_pair_pitch; /* weights given and pairs > 1: >= (n - 1) * weights_pitch + k */
    int32_t pairs;              /* 1..65535 */
    int32_t n;                  /* N, 1..JSGX_DTW_MAX_LEN */
    int32_t n_features;         /* F, 1..JSGX_NNF_MAX_FEATURES */
    int32_t k;                  /* 1..JSGX_KNN_MAX_K */
    float* out;                 /* device floats: out[p][i][f] */
    int64_t out_frame_pitch;    /* >= n_features */
    int64_t out_pair_pitch;     /* pairs > 1: >= (n - 1) * out_frame_pitch + n_features */
} jsgx_nn_filter_args;          /* 112 bytes, no padding */

/* Enqueue only (one kernel, no scratch); capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing enqueued), in this
 * order and before any device call: null args, a null s, a null nn_index, a null out; a pointer that is not 4-byte aligned; pairs
 * outside 1..65535, n outside 1..65536, n_features outside 1..65536, k outside 1..256; s_frame_pitch below n_features, s_pair_pitch that
 * does not cover a plane (pairs > 1), index_pitch below k, index_pair_pitch that does not cover a plane (pairs > 1), the same for
 * weights_pitch and weights_pair_pitch (weights given), out_frame_pitch below n_features, out_pair_pitch that does not cover a plane
 * (pairs > 1); out overlapping s, out overlapping nn_index, out overlapping weights.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_nn_filter_launch(const jsgx_nn_filter_args* args, void* stream);

/* Section 9 was added to version 1 in the same way: sections 1 to 8, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 9. Recurrence quantification alignment (librosa.sequence.rqa, the third function of librosa.sequence): the best-scoring aligned run
 *    through a similarity plane, with gaps and, optionally, knight moves.  R[i][j] = sim[p*sim_pair_pitch + i*sim_pitch + j], i < N,
 *    j < M: a plane of section 7 (affinity mode, or cross-similarity) or any plane the caller filled.  Pairs are independent.  All
 *    arithmetic is float32 and uncontracted (there are only additions, subtractions and comparisons); fl(.) is one rounding to float32.
 *
 *    Links.  A cell is a link iff R[i][j] > 0, the comparison as written: a NaN, a zero or a negative value is no link.
 *    Steps, as (di, dj):  k = 0: (1, 1),  k = 1: (1, 2),  k = 2: (2, 1).  With knight = 0 only k = 0 is a step.  The candidates of a cell
 *    are the steps whose predecessor pred_k = (i - di, j - dj) lies inside the matrix; for i, j >= 1, k = 0 always is one.
 *
 *    Border cells (i == 0 or j == 0):  S = R, with its bits;  step = -2 where the cell is a link, else -1.
 *    Every other cell, over its candidates in ascending k:
 *        link cell:      v_k = S[pred_k]
 *        non-link cell:  v_k = fl(S[pred_k] - pen_k),  pen_k = gap_onset where pred_k is a link, else gap_extend
 *        best = v of the lowest candidate;  for each later candidate:  if (v_k > best) best = v_k;      k* = the k that was kept
 *        link cell:      S = fl(best + R[i][j]);  step = k*
 *        non-link cell:  if (best > 0) { S = best; step = k*; } else { S = +0; step = -1; }
 *    The comparison is strict: the lowest k wins ties, a NaN v_k never replaces best, a NaN first candidate stays, and a NaN best
 *    resets a non-link cell.  S[i][j] is a function of the plane alone: it does not depend on the tile sizes, on pairs, on the pitches
 *    or on which outputs are NULL.
 *
 *    End cell.  Among the cells with S > 0 the one with the largest S; among equal S the lowest i, then the lowest j: numpy's flat
 *    argmax order, stated as a total order on (S, i, j), so its maximum is associative and commutative and does not depend on how a
 *    kernel splits the cells.  Where no cell has S > 0:  path_len[p] = 0, total[p] = +0, end[p] = (-1, -1) and no path is written: a
 *    result, not a refusal.
 *    Backtrace.  No step plane is kept for it: as in section 3 the step of the current cell is recomputed from S and R with the same
 *    operations and the same selection.  At each cell:  step -1: stop, the cell is not part of the path.  Otherwise the cell is part of
 *    the path;  step -2: stop;  otherwise move to pred_k*.  Every step lowers both i and j, so a path has at most min(N, M) cells.
 *    Outputs.  score[p*score_pair_pitch + i*score_pitch + j] = S, required.  step[p*step_pair_pitch + i*step_pitch + j]: the int8
 *    values above, optional.  path_i and path_j at [p*path_pitch + n], n < path_len[p], ascending, the start first.  end[2p], end[2p+1] =
 *    (i, j) of the end cell.  total[p] = S there.
 *
 *    Known answers.  An all-zero plane: S = +0 everywhere, every step is -1, path_len is 0.  The N x N identity, either knight: the
 *    path is the main diagonal, total = N exactly, and the end cell is unique.  The identity with R[g][g] and R[g+1][g+1] cleared,
 *    2 <= g, knight = 0:  total = N - 2 - gap_onset - gap_extend and the path is still the whole diagonal, the two gap cells having
 *    S > 0 (N = 70, g = 2, penalties 0.5 and 0.25: 67.25); with knight = 1 the same plane is bridged by a knight move: total 67.5,
 *    69 cells.
 *
 *    Differences from librosa.sequence.rqa: a link is R > 0 everywhere (librosa tests truthiness on the border); the NaN and tie rules
 *    are the ones above; score is float32.  Agreement with librosa has not been measured: librosa is not installed where this was
 *    built.  No error bound is claimed, since gaps subtract; on planes and penalties that are small integers or dyadic fractions every
 *    operation is exact.
 *
 *    The kernels.  The three predecessors lie in an earlier row AND an earlier column, so the cells of one row are independent of each
 *    other and the skewed sweep of section 3 is not needed.  S is cut into the tiles of section 3 (JSGX_DTW_TILE_ROWS x
 *    JSGX_DTW_TILE_COLS) and "rqa_tiles" is launched once per tile anti-diagonal over pairs x (tiles on it), one wavefront per tile.  A
 *    tile reads its halo from score itself -- the two rows above, the two columns to the left and the corner between them, which
 *    earlier launches on the stream wrote -- and the matching cells of sim; no workgroup waits for another.  Inside the tile lane l
 *    owns column l and the rows are walked top to bottom, 64 steps: S(i-1, j-1) is one DPP wave shift of the row above (lane 0 takes
 *    the left halo), S(i-1, j-2) a second shift of that, S(i-2, j-1) the first shift of the step before; the penalties of the
 *    predecessors travel the same way.  R comes in and S goes out through LDS in whole lines, and a step's LDS operands are read two
 *    steps ahead.  The forms with and without knight moves and with and without a step plane are separate kernels, and the tiles that
 *    hold row 0 or column 0 take a form of their own, so the border rule is not in the hot one.  Where path_len, end or total is given
 *    a tile also reduces its best (S, i, j) by the key above into the scratch (8 bytes a tile: S and i * 65536 + j), and
 *    "rqa_backtrace", one wavefront per pair, reduces those entries, so the plane is not read a second time for the end cell; it then
 *    fetches JSGX_RQA_WINDOW x JSGX_RQA_WINDOW windows of S and R that end at the current cell and walks inside each while two rows
 *    and two columns of halo remain (at least 15 steps per round trip to memory), writes the path backwards into the scratch and copies
 *    it out reversed.  Every loop is bounded by min(N, M).
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_RQA_THREADS 64
#define JSGX_RQA_LDS_BYTES 17408           /* static, of the forward kernels: the tile 64 x 64 words, the left halo 64 x 4 words */
#define JSGX_RQA_WINDOW 32

typedef struct jsgx_rqa_args {
    const float* sim;           /* device floats: R */
    int64_t sim_pitch;          /* >= m */
    int64_t sim_pair_pitch;     /* pairs > 1: >= (n - 1) * sim_pitch + m */
    int32_t pairs;              /* 1..65535 */
    int32_t n;                  /* N, 1..JSGX_DTW_MAX_LEN */
    int32_t m;                  /* M, 1..JSGX_DTW_MAX_LEN */
    int32_t knight;             /* 0 or 1 */
    float gap_onset;            /* finite, >= 0 */
    float gap_extend;           /* finite, >= 0 */
    int32_t reserved0;          /* 0 */
    int32_t max_path;           /* paths given: >= min(n, m) */
    float* score;               /* device floats: S, required */
    int64_t score_pitch;        /* >= m */
    int64_t score_pair_pitch;   /* pairs > 1: >= (n - 1) * score_pitch + m */
    int8_t* step;               /* device int8 or NULL */
    int64_t step_pitch;         /* step given: >= m */
    int64_t step_pair_pitch;    /* step given and pairs > 1: >= (n - 1) * step_pitch + m */
    int32_t* path_i;            /* device int32 or NULL (then path_j NULL too) */
    int32_t* path_j;
    int64_t path_pitch;         /* pairs > 1 and paths given: >= max_path */
    int32_t* path_len;          /* device int32 [pairs]; required with the paths, else optional */
    int32_t* end;               /* device int32 [pairs][2] or NULL */
    float* total;               /* device floats [pairs] or NULL */
} jsgx_rqa_args;                /* 152 bytes, no padding */

/* The bytes of scratch the launch needs: 8 * pairs * tiles for the tiles' best cells where path_len, end or total is given (tiles =
 * ceil(n / JSGX_DTW_TILE_ROWS) * ceil(m / JSGX_DTW_TILE_COLS)), plus 8 * pairs * min(n, m) where the paths are given; else 0.  Refused
 * (a negative jsgx_status): what the launch refuses before it looks at the scratch. */
JSGX_API int64_t jsgx_rqa_scratch_bytes(const jsgx_rqa_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  The kernels (one per tile anti-diagonal,
 * then the backtrace where path_len, end or total is given) go onto the one stream as a plain chain.  Refused (JSGX_ERR_INVALID,
 * nothing enqueued), in this order and before any device call: null args, a null sim, a null score, one of path_i and path_j without
 * the other, paths without path_len; a float or int32 pointer that is not 4-byte aligned; pairs outside 1..65535, n outside 1..65536,
 * m outside 1..65536, knight other than 0 or 1, a gap_onset that is not finite and >= 0, the same for gap_extend; a non-zero
 * reserved0; max_path below min(n, m) (paths given); sim_pitch below m, sim_pair_pitch that does not cover a plane (pairs > 1), the
 * same for score_pitch and score_pair_pitch and (step given) for step_pitch and step_pair_pitch, path_pitch below max_path (pairs > 1,
 * paths given); score overlapping sim, another output (step, path_i, path_j, path_len, end, total) overlapping sim, two outputs
 * (score among them) overlapping each other; a null scratch, a scratch that is not 4-byte aligned, scratch_bytes below the size above
 * (each only where that size is not 0).  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_rqa_launch(const jsgx_rqa_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the name of the forward kernel ("rqa_tiles"), the tile sizes, the number of kernel
 * launches (the tile anti-diagonals, ceil(n / tile_rows) + ceil(m / tile_cols) - 1, plus one for "rqa_backtrace" where path_len, end or
 * total is given), JSGX_RQA_THREADS and JSGX_RQA_LDS_BYTES.  Any output pointer may be NULL (name: else name_len >= 16).  Refused: a
 * name_len below 16 with a name, then what the scratch size refuses. */
JSGX_API int jsgx_rqa_plan(const jsgx_rqa_args* args, char* name, int name_len, int32_t* tile_rows, int32_t* tile_cols, int32_t* n_launches,
                           int32_t* threads, int32_t* lds_bytes);

/* Sections 10 and 11 were added to version 1 in the same way: sections 1 to 9, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 10. Path enhancement of a recurrence plane (librosa.segment.path_enhance, the step between sections 7 and 9): a bank of sparse
 *     two-dimensional filters over the plane and the maximum over the bank.  R[i][j] = r[p*r_pair_pitch + i*r_pitch + j], i < N, j < M,
 *     float32; Rz is R inside the plane and +0 outside (scipy.ndimage's mode="constant", cval=0).  Pairs are independent.
 *
 *     A bank is a tap list in device memory: tap_w[t] float32 weights; tap_at[t] int32 holding two signed 16-bit offsets, di in the high
 *     half and dj in the low half; filter_first[f], f <= F, int32, ascending, filter_first[F] = n_taps.  For filter f, the taps in list order:
 *         acc_f = +0
 *         for t in filter_first[f] .. filter_first[f+1]-1 :   acc_f = fmaf(tap_w[t], Rz[i + di_t][j + dj_t], acc_f)
 *     Across the filters in ascending f:
 *         best = acc_0;   later f:  if (acc_f > best || acc_f != acc_f) best = acc_f          (np.maximum: a NaN wins and stays)
 *     With clip:  out = best < 0 ? +0 : best  (a NaN stays); without:  out = best.
 *     out[p*out_pair_pitch + i*out_pitch + j]; every element of the plane is written and nothing else.
 *     A filter with no taps gives acc_f = +0.  A tap with |di| > reach_i or |dj| > reach_j is skipped; reach_i and reach_j are host
 *     arguments in 0..JSGX_PE_MAX_REACH.  The host cannot see the device table: this rule, and every filter_first entry being clamped into
 *     0..n_taps, keep a bad table from reading outside the arrays or outside the staged window (a filter_first that descends gives an
 *     empty filter).
 *     For finite weights, skipping a tap that falls outside the plane and adding w * (+0) give the same bits: acc starts at +0 and
 *     x + (+-0) = x for x != 0, (+0) + (+-0) = +0, so acc never becomes -0.  A kernel may therefore zero-fill its halo.  (An infinite or
 *     NaN weight times the +0 outside the plane is a NaN: stated, not avoided.)
 *     out[i][j] is a function of the plane and the list alone: it does not depend on tiles, pairs, pitches or how a kernel groups taps.
 *
 *     Against scipy.  For a table K of shape (h, w), scipy.ndimage.convolve(R, K, mode="constant")[i][j] = sum K[a][b] * Rz[i + h/2 - a][j +
 *     w/2 - b] (integer halves; even and odd h, w): the tap of K[a][b] has di = h/2 - a, dj = w/2 - b.  scipy sums in float64 in an order of
 *     its own; for non-negative planes and weights this chain is within T u / (1 - T u) relative of the exact sum, T the taps of the
 *     largest filter, u = 2^-24.
 *
 *     The builder (host, double precision, no device) restates librosa.segment.path_enhance's bank: slopes 2 ** linspace(log2(min_ratio),
 *     log2(max_ratio), n_filters); each filter starts as diag(window) (n x n) and stays so where |slope - 1| <= 1e-8 + 1e-5 (numpy's
 *     isclose); otherwise it is rotated as scipy.ndimage.rotate(win, -(atan(slope) * 180 / pi - 45), order=5, prefilter=False) does: with
 *     c, s the cosine and sine of that angle, Rm = [[c, s], [-s, c]]; the output shape is int(ptp(Rm @ [[0,0,n,n],[0,n,0,n]], axis=1) +
 *     0.5); offset = (n-1)/2 - Rm @ ((shape-1)/2); output cell (y, x) maps to p = Rm @ (y, x) + offset; a cell with a coordinate of p < 0
 *     or > n - 1 is 0, every other is the 6 x 6 sum of B5(p_y - yy) B5(p_x - xx) win[mirror(yy)][mirror(xx)], yy from floor(p_y) - 2, B5
 *     the centred quintic B-spline and mirror the reflection about the end samples, period 2 (n - 1).  Then the table is clipped at 0 and
 *     divided by its sum; with zero_mean its mean is subtracted, which makes it dense (every entry a tap: up to 129 x 129 a filter
 *     instead of a few hundred, and the kernel's time grows with it).  The taps are the non-zero entries in row-major order (a, then b,
 *     ascending), rounded to float32; an entry whose float32 is zero or subnormal, or below drop_below times the largest magnitude of
 *     its table, is dropped (drop_below 0, the default in Python: librosa's filters, untrimmed).
 *
 *     The kernel ("path_enhance_tiles", vector pipe: the summation order is the contract).  A workgroup of JSGX_PE_THREADS lanes owns a
 *     JSGX_PE_TILE x JSGX_PE_TILE output tile and stages it with its halo of reach_i rows and reach_j columns once into LDS, zero-filled
 *     outside the plane: (64 + 2 reach_i) rows of W words, W = 64 + 2 reach_j rounded up to 1 (mod 4), so that the eight rows a
 *     wavefront reads at once fall on different banks.  A lane holds 4 rows x 4 adjacent columns of outputs in registers.  Weights and
 *     offsets are the same for every lane: they are fetched by scalar loads, eight taps ahead, and enter v_fma_f32 as scalar operands.
 *     Row-major order puts horizontal runs of taps next to each other in the list; a uniform branch on the run length (8, 4, 2, 1) lets
 *     the L taps of a run share L + 3 LDS reads per output row instead of 4 L, and every output still sees its taps in list order.
 *     LDS: 4 * (64 + 2 reach_i) * W bytes, dynamic: 148224 at the largest reach (inside 160 KiB), 66048 at reach 32 (two workgroups a
 *     compute unit).
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_PE_MAX_REACH 64
#define JSGX_PE_MAX_FILTERS 32
#define JSGX_PE_MAX_TAPS 1048576
#define JSGX_PE_TILE 64
#define JSGX_PE_THREADS 256
#define JSGX_PE_LDS_LIMIT 163840
#define JSGX_PE_MIN_WINDOW 3
#define JSGX_PE_MAX_WINDOW 101

typedef struct jsgx_path_enhance_args {
    const float* r;             /* device floats: R */
    int64_t r_pitch;            /* >= m */
    int64_t r_pair_pitch;       /* pairs > 1: >= (n - 1) * r_pitch + m */
    const float* tap_w;         /* device floats [n_taps] */
    const int32_t* tap_at;      /* device int32 [n_taps]: (di << 16) | (dj & 0xffff) */
    const int32_t* filter_first;/* device int32 [n_filters + 1] */
    int32_t pairs;              /* 1..65535 */
    int32_t n;                  /* N, 1..JSGX_DTW_MAX_LEN */
    int32_t m;                  /* M, 1..JSGX_DTW_MAX_LEN */
    int32_t n_filters;          /* F, 1..JSGX_PE_MAX_FILTERS */
    int32_t n_taps;             /* 1..JSGX_PE_MAX_TAPS */
    int32_t reach_i;            /* 0..JSGX_PE_MAX_REACH */
    int32_t reach_j;            /* 0..JSGX_PE_MAX_REACH */
    int32_t clip;               /* 0 or 1 */
    float* out;                 /* device floats: [p][i][j] */
    int64_t out_pitch;          /* >= m */
    int64_t out_pair_pitch;     /* pairs > 1: >= (n - 1) * out_pitch + m */
} jsgx_path_enhance_args;       /* 104 bytes, no padding */

/* Enqueue only (one kernel, no scratch): no allocation, no synchronisation; capture works, a first launch included.  Refused
 * (JSGX_ERR_INVALID, nothing enqueued), in this order and before any device call: null args, a null r, a null tap_w, a null tap_at, a
 * null filter_first, a null out; a pointer that is not 4-byte aligned; pairs outside 1..65535, n outside 1..65536, m outside 1..65536,
 * n_filters outside 1..32, n_taps outside 1..2^20, reach_i outside 0..64, reach_j outside 0..64, clip other than 0 or 1; r_pitch below m,
 * r_pair_pitch that does not cover a plane (pairs > 1), the same for out_pitch and out_pair_pitch; out overlapping r, out overlapping
 * tap_w, tap_at, filter_first in this order.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_path_enhance_launch(const jsgx_path_enhance_args* args, void* stream);
/* The kernel of these arguments, without a device: its name ("path_enhance_tiles"), the rows and columns of a tile, the lanes of a
 * workgroup and the bytes of LDS it holds for these reaches.  Any output pointer may be NULL (name: else name_len >= 32).  Refused: a
 * name_len below 32 with a name, then what the launch refuses. */
JSGX_API int jsgx_path_enhance_plan(const jsgx_path_enhance_args* args, char* name, int name_len, int32_t* tile_rows, int32_t* tile_cols, int32_t* threads,
                                    int32_t* lds_bytes);
/* The dense table of one filter of the builder, in double: *rows x *cols, row-major into table where table is not NULL and capacity
 * (in doubles) holds it; with table NULL only the shape is returned.  JSGX_ERR_INVALID, in this order: a null window, a null rows, a
 * null cols; n outside 3..101; a slope that is not finite and > 0; zero_mean other than 0 or 1; a window entry that is not finite; a
 * table whose sum after clipping is not > 0; a capacity below rows * cols (table given). */
JSGX_API int jsgx_diagonal_filter_table(const double* window, int32_t n, double slope, int32_t zero_mean, int32_t* rows, int32_t* cols, double* table,
                                        int64_t capacity);
/* The bank of librosa.segment.path_enhance as a tap list (above).  *n_taps, *reach_i and *reach_j are always written (the size query:
 * tap_w, tap_at and filter_first all NULL); with the three arrays, tap_w and tap_at take *n_taps entries and filter_first n_filters + 1.
 * JSGX_ERR_INVALID, in this order: a null window, a null n_taps, a null reach_i, a null reach_j; some but not all of the three arrays;
 * n outside 3..101; min_ratio or max_ratio not finite and > 0, min_ratio above max_ratio; n_filters outside 1..32; zero_mean other
 * than 0 or 1; drop_below not in [0, 1); a window entry that is not finite; a table whose sum after clipping is not > 0; a bank with
 * no tap or with more than JSGX_PE_MAX_TAPS; a reach above JSGX_PE_MAX_REACH; a capacity below *n_taps (arrays given). */
JSGX_API int jsgx_diagonal_filter_build(const double* window, int32_t n, double min_ratio, double max_ratio, int32_t n_filters, int32_t zero_mean,
                                        double drop_below, int32_t* n_taps, int32_t* reach_i, int32_t* reach_j, float* tap_w, int32_t* tap_at,
                                        int32_t* filter_first, int64_t capacity);

/* ------------------------------------------------------------------------------------------------
 * 11. Time-lag conversion of a square plane (librosa.segment.recurrence_to_lag and lag_to_recurrence) in this library's index order.
 *     L = 2 N with pad, else N.  Rz is R with +0 for rows (axis 1) or columns (axis 0) >= N.
 *         axis 1, to lag (inverse 0):     lag[l][j] = Rz[(l + j) mod L][j],  l < L, j < N     (in N x N, out L x N)
 *         axis 1, from lag (inverse 1):   R[i][j] = lag[(i - j) mod L][j],   i, j < N         (in L x N, out N x N)
 *         axis 0, to lag:                 lag[i][l] = Rz[i][(l + i) mod L],  i < N, l < L     (in N x N, out N x L)
 *         axis 0, from lag:               R[i][j] = lag[i][(j - i) mod L]                     (in N x L, out N x N)
 *     librosa's axis=-1 on a two-dimensional array is axis 1 here.  The output is a pure permutation (and the zeros of the padding):
 *     every output element is written once, bits unchanged, and nothing else is written.  Planes are [p][row][col] with a pitch and a pair
 *     pitch as in section 7, whose query-major orientation note holds: lag l of column j (axis 1) is the row distance of a neighbour.
 *     The kernels: "lag_columns" (axis 1) takes a 64 x 64 output tile per workgroup: its source is a parallelogram of 127 row pieces of
 *     64 columns, read as whole 256-byte lines into LDS (a source line is read by two tiles) and written out as whole lines; "lag_rows"
 *     (axis 0) rotates every row: reads and writes run along the row.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_LAG_THREADS 256
#define JSGX_LAG_TILE 64
#define JSGX_LAG_LDS_BYTES 32512           /* static, "lag_columns": 127 pieces of 64 words */

typedef struct jsgx_lag_args {
    const float* in;            /* device floats */
    int64_t in_pitch;           /* >= the input's columns */
    int64_t in_pair_pitch;      /* pairs > 1: covers the input plane */
    int32_t pairs;              /* 1..65535 */
    int32_t n;                  /* N, 1..JSGX_DTW_MAX_LEN */
    int32_t pad;                /* 0 or 1 */
    int32_t axis;               /* 0 or 1 */
    int32_t inverse;            /* 0: to lag, 1: from lag */
    int32_t reserved0;          /* 0 */
    float* out;                 /* device floats */
    int64_t out_pitch;          /* >= the output's columns */
    int64_t out_pair_pitch;     /* pairs > 1: covers the output plane */
} jsgx_lag_args;                /* 72 bytes, no padding */

/* Enqueue only (one kernel, no scratch); capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing enqueued), in this
 * order and before any device call: null args, a null in, a null out; a pointer that is not 4-byte aligned; pairs outside 1..65535, n
 * outside 1..65536, pad other than 0 or 1, axis other than 0 or 1, inverse other than 0 or 1; a non-zero reserved0; in_pitch below the
 * input's columns, in_pair_pitch that does not cover a plane (pairs > 1), the same for out_pitch and out_pair_pitch; out overlapping
 * in.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_lag_launch(const jsgx_lag_args* args, void* stream);

/* Section 12 was added to version 1 in the same way: sections 1 to 11, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 12. Non-negative matrix factorisation (librosa.decompose.decompose with scikit-learn's NMF, solver="mu", beta_loss="frobenius"):
 *     a plane V of T frames and K bins is factored into r spectral templates and their activations over time, V ~ A C.
 *     Planes are frame-major, as everywhere here:
 *         V[t][k] = v[p*v_problem_pitch + t*v_pitch + k],  t < T, k < K        the input, read only
 *         A[t][c] = a[p*a_problem_pitch + t*a_pitch + c],  c < r               the activations, [T][r]
 *         C[c][k] = c[p*c_problem_pitch + c*c_pitch + k]                       the components, [r][K]
 *     librosa documents the transposes: its `components` is K x r (C transposed) and its `activations` r x T (A transposed); scikit-learn's
 *     W is A and its H is C for X = V.  The P problems are independent.  A and C hold the start when the launch begins and are
 *     updated in place, n_iter times.
 *
 *     Data: non-negative finite float32.  Negative, NaN or infinite inputs, and values so large that a sum below overflows, are
 *     outside the contract: the launch still ends and writes nothing outside A and C (and the scratch), as in section 1.  Subnormals
 *     are kept (the default kernel mode).
 *
 *     The chunked sum of n products x_i * y_i with chunk length L, the one rule for every long sum here: chunk q covers i in
 *     [q L, min(n, q L + L));  p_q is the chain  acc = +0;  acc = fmaf(x_i, y_i, acc)  for i ascending over the chunk;  the sum is
 *     ((p_0 + p_1) + p_2) + ... with plain adds, q ascending (one chunk: p_0 itself).  L is JSGX_NMF_CHUNK_K for sums over bins and
 *     JSGX_NMF_CHUNK_T for sums over frames; both are multiples of 64 and depend on nothing: not on the device, the grid, P, the pitches
 *     or r.  (The unit started from 256 and 1024; frame chunks of 256 measured faster, DESIGN.md 6u, and no other value was tried.)
 *
 *     One iteration, in scikit-learn's order: the activations first, then the components from the new activations.
 *         N[t][c]  = chunked sum over k (CHUNK_K) of V[t][k] * C[c][k]
 *         G[c][c'] = chunked sum over k (CHUNK_K) of C[c][k] * C[c'][k]
 *         D[t][c]  = acc = +0;  acc = fmaf(A[t][c'], G[c'][c], acc),  c' = 0..r-1 ascending             (one chain, no chunks)
 *         Dz = D where D != 0, else 2^-23 (JSGX_NMF_EPSILON)                                             (scikit-learn's EPSILON rule)
 *         A[t][c]  = fl(A[t][c] * fl(N[t][c] / Dz))                                                      (the divide correctly rounded)
 *     and, where update_components is 1, with the new A:
 *         N2[c][k]  = chunked sum over t (CHUNK_T) of A[t][c] * V[t][k]
 *         G2[c][c'] = chunked sum over t (CHUNK_T) of A[t][c] * A[t][c']
 *         D2[c][k]  = acc = +0;  acc = fmaf(G2[c][c'], C[c'][k], acc),  c' ascending
 *         C[c][k]   = fl(C[c][k] * fl(N2[c][k] / D2z))                                                   (D2z from D2 as Dz from D)
 *     With update_components 0 the components stay as they are (scikit-learn's transform with update_H=False) and G is the same in
 *     every iteration.
 *
 *     Padding.  On non-negative data every acc is +0 or positive, and fmaf(+0, +0, acc) = acc bit for bit; so a chain may be extended
 *     by operand pairs that are both +0 wherever a kernel likes.  This is why r, K, T and the chunk tails need not be multiples of a
 *     tile: the kernels zero-fill their panels.  fmaf(x, y, acc) = fmaf(y, x, acc), so G and G2 are symmetric bit for bit.
 *
 *     Known answers.  V = A C from small integers (every sum exact in float32) is a fixed point: N = D and N2 = D2, every ratio is
 *     exactly 1, A and C come back bit-identical.  An all-zero frame of V has N = +0 and zeroes its row of A; an all-zero bin zeroes its
 *     column of C.  An all-zero row of A has D = +0, takes the 2^-23 rule and stays zero.
 *
 *     Deliberate differences from librosa.decompose.decompose / scikit-learn: a fixed iteration count, no `tol` stopping (the launch
 *     is enqueue-only); no "nndsvd" initialisation (the caller gives the start; Python offers scikit-learn's init="random" rule); the
 *     Frobenius loss only (`loss` is carried for a later Kullback-Leibler form and any value but JSGX_NMF_FROBENIUS is refused); no
 *     regularisation.  In float64 this definition equals sklearn.decomposition.non_negative_factorization(init="custom",
 *     solver="mu", beta_loss="frobenius", tol=0) exactly (tests/test_nmf_ref.py); agreement with librosa itself is not measured.
 *
 *     The kernels (the matrix pipe: v_mfma_f32_16x16x4_f32 on float32 inputs is, on gfx950, bit for bit the k-ascending fmaf chain from
 *     its accumulator input, one rounding a product and no wider accumulator; tests/test_gpu_nmf.py checks that first, and it is the one
 *     stated exception to this library's vector-pipe rule).  Workgroups of JSGX_NMF_THREADS lanes (four wavefronts) stage 64 x 64
 *     panels into JSGX_NMF_LDS_BYTES of LDS, zero-filled outside the planes, the next panel on its way from memory into registers while
 *     the current one is multiplied; a wavefront owns 16 x 16 output tiles, one accumulator each.
 *         "nmf_gram"      one (chunk, problem): the r x r chain of that chunk of C C^T (or A^T A) into the scratch
 *         "nmf_chunk_sum" one element a lane: adds the chunks' partials of a Gram matrix, or of N2, in ascending chunk order
 *         "nmf_update_a"  one strip of 64 frames: sweeps k chunk by chunk (a chain a chunk, then the plain add), then the D chain, the
 *                         divide and the multiply; it alone reads and writes its rows of A
 *         "nmf_partial_c" one (tile of 64 bins, frame chunk, problem): the chain of that chunk of N2 into the scratch
 *         "nmf_update_c"  one tile of 64 bins, every component: the D2 chain, the divide and the multiply; it alone reads and writes its
 *                         columns of C
 *     An iteration is 8 launches on the one stream with update_components (gram, chunk_sum, update_a, gram, chunk_sum, partial_c,
 *     chunk_sum, update_c) and 1 without (update_a; gram and chunk_sum run once in front of the first).  No workgroup waits for another and
 *     there are no atomics.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_NMF_MAX_COMPONENTS 64
#define JSGX_NMF_MAX_BINS 16384
#define JSGX_NMF_MAX_FRAMES 16777216
#define JSGX_NMF_MAX_ITER 65536
#define JSGX_NMF_CHUNK_K 256
#define JSGX_NMF_CHUNK_T 256
#define JSGX_NMF_FROBENIUS 0
#define JSGX_NMF_EPSILON 1.1920928955078125e-07f        /* 2^-23 */
#define JSGX_NMF_THREADS 256
#define JSGX_NMF_LDS_BYTES 40960           /* static: two panels of 64 rows of 80 words */

typedef struct jsgx_nmf_args {
    const float* v;             /* device floats: V */
    int64_t v_pitch;            /* >= n_bins */
    int64_t v_problem_pitch;    /* problems > 1: >= (n_frames - 1) * v_pitch + n_bins */
    float* a;                   /* device floats: A, the start on entry */
    int64_t a_pitch;            /* >= n_components */
    int64_t a_problem_pitch;    /* problems > 1: >= (n_frames - 1) * a_pitch + n_components */
    float* c;                   /* device floats: C, the start on entry */
    int64_t c_pitch;            /* >= n_bins */
    int64_t c_problem_pitch;    /* problems > 1: >= (n_components - 1) * c_pitch + n_bins */
    int32_t problems;           /* P, 1..65535 */
    int32_t n_frames;           /* T, 1..JSGX_NMF_MAX_FRAMES */
    int32_t n_bins;             /* K, 1..JSGX_NMF_MAX_BINS */
    int32_t n_components;       /* r, 1..JSGX_NMF_MAX_COMPONENTS */
    int32_t n_iter;             /* 1..JSGX_NMF_MAX_ITER */
    int32_t update_components;  /* 0 or 1 */
    int32_t loss;               /* JSGX_NMF_FROBENIUS */
    int32_t reserved0;          /* 0 */
} jsgx_nmf_args;                /* 104 bytes, no padding */

/* The bytes of scratch the launch needs, with cK = ceil(K / CHUNK_K) and cT = ceil(T / CHUNK_T):  4 * P * r * r * (2 + cK)  without
 * update_components (G, G2 unused, the chunks' partials of G), else  4 * P * r * (r * (2 + max(cK, cT)) + cT * K)  (also the partials
 * of G2, in the same place, and of N2).  A larger scratch changes nothing.  Refused (a negative jsgx_status): what the launch refuses
 * before it looks at the scratch. */
JSGX_API int64_t jsgx_nmf_scratch_bytes(const jsgx_nmf_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing
 * enqueued), in this order and before any device call: null args, a null v, a null a, a null c; a pointer that is not 4-byte aligned;
 * problems outside 1..65535, n_frames outside 1..2^24, n_bins outside 1..16384, n_components outside 1..64, n_iter outside 1..65536,
 * update_components other than 0 or 1, a loss other than JSGX_NMF_FROBENIUS, a non-zero reserved0; v_pitch below n_bins,
 * v_problem_pitch that does not cover a plane (problems > 1), the same for a_pitch (against n_components) and a_problem_pitch and for
 * c_pitch (against n_bins) and c_problem_pitch; a overlapping v, c overlapping v, a overlapping c; a null scratch, a scratch that is
 * not 4-byte aligned, scratch_bytes below the size above; the scratch (the bytes of that size) overlapping v, a, c in this order.
 * Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_nmf_launch(const jsgx_nmf_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the name of the kernel that sweeps V ("nmf_update_a"), JSGX_NMF_THREADS,
 * JSGX_NMF_LDS_BYTES, the launches of an iteration (8, or 1 without update_components) and cT, the frame chunks.  Any output pointer may
 * be NULL (name: else name_len >= 16).  Refused: a name_len below 16 with a name, then what the scratch size refuses. */
JSGX_API int jsgx_nmf_plan(const jsgx_nmf_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* launches_per_iter,
                           int32_t* t_chunks);

/* Section 13 was added to version 1 in the same way: sections 1 to 12, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 13. Per-channel energy normalisation (librosa.pcen; Wang et al. 2017, Lostanlen et al. 2019): an automatic gain control per band
 *     followed by root compression, the alternative to 10 log10 between a mel plane and whatever reads it.  The plane is
 *         M[r][t][m] = in[r*row_pitch + t*frame_pitch + m],  r < rows, t < T (n_frames), m < B (n_bands)
 *     as in jsg.h sections 2j to 2l; out and smooth_out have pitches of their own, state_in and state_out are [rows][B] at a row
 *     pitch.  Rows and bands are independent.  The scalars b (the smoothing coefficient), gain, bias, power and eps are float32;
 *     a = fl(1.0f - b).  The chunk length JSGX_PCEN_CHUNK = 256 frames depends on nothing: not on the shape, the device or the launch.
 *
 *     Smoother.  q[j] = (float)(a^(j+1)), j = 0..255: the table `decay`, pow in double of the float a, rounded once
 *     (jsgx_pcen_decay_build).  The state that enters a row is s = state_in[r][m] where state_in is given, else M[r][0][m]: in exact
 *     arithmetic that is librosa's default zi, which gives S[0] = M[0].  For chunk c over the frames t = 256 c + j, c ascending:
 *         p = +0;   for j ascending:   p = fmaf(a, p, fl(b * M[t]));   S[t] = fmaf(q[j], s, p)
 *         s = S[the last frame of the chunk]        (the state that enters chunk c + 1; behind the last chunk: state_out[r][m])
 *     In exact arithmetic S[t] = a S[t-1] + b M[t].  S goes to smooth_out where that is given.
 *
 *     Compression.  Every product and sum is rounded on its own, no contraction:
 *         g   = E(fl(-gain * L(fl(eps + S[t]))))                      ((eps + S)^-gain)
 *         y   = fl(bias + fl(M[t] * g))
 *         out = fl(E(fl(power * L(y))) - d),   d = E(fl(power * L(bias)))  by the same routines        ((M g + bias)^power - bias^power)
 *     L(x) is the logarithm of section 5, here over every positive float32, subnormals included (against log in double over all of them:
 *     JSGX_LOG_ABS_BOUND holds, profiles/pcen_accuracy.md).  E(x) is the exponential of section 1 carried to the whole line:
 *         a NaN: NaN;   x < -87.0f: +0;   x > 88.72f: +inf
 *         otherwise n, r and the polynomial p of section 1 (n = -126 .. 128), and
 *         E = fl(fl(p * 2^h) * 2^(n - h)),  h = floor(n / 2), both factors floats built from their exponent bits: the first product is exact
 *     For -87 <= x <= 0 the bits of E are those of section 1's routine (one routine serves both).  Against exp in double over every
 *     float32 in [-87, 88.72] the relative error is within JSGX_EXP_REL_BOUND (profiles/pcen_accuracy.md).
 *
 *     Known answers.  A silent frame (M[t] = 0, g finite) has y = bias and out = fl(x - x) = +0 exactly, for every bias >= 0; with
 *     bias = 0, L(0) = -inf and E(-inf) = +0 serve without a special case.  b = 1: a = +0, q = +0, S = M.
 *
 *     Consequences.  A NaN at (r, t0, m) makes p, S and every later state NaN: it poisons (r, t >= t0, m) and nothing else.  A
 *     negative value gives NaN wherever eps + S < 0 or y < 0, in its own (r, m) only.  No output depends on the number of rows, on the
 *     pitches or on the launch geometry.  A plane processed in two calls, split at a multiple of 256 frames with state_out fed to
 *     state_in, equals the single call bit for bit; split elsewhere it differs in the last bits (another association of the same sum).
 *
 *     Deliberate differences from librosa.pcen: the state is the previous smoothed value, not scipy's filter delay (zi = a * state);
 *     power > 0 only (the log1p limit at power = 0 is not built); no max_size maximum filter across bands; no axis argument (frames
 *     are the second-to-last axis); float32 throughout.  Against the float64 route through scipy.signal.lfilter the restatement of
 *     this definition is within the figures of profiles/pcen_accuracy.md; agreement with librosa itself is not measured.
 *
 *     The kernels.  A lane owns one chain: one band of one chunk of one row.  The chains are numbered (row, chunk, band), the band
 *     fastest, and dealt to workgroups of JSGX_PCEN_THREADS lanes in that order: a wavefront reads neighbouring floats of a frame, and
 *     with fewer than 64 bands it holds several chunks or rows, so no lane idles but in the last workgroup.  No LDS.
 *         "pcen_chunked" (T > 256), three launches: "pcen_scan" (p of every chunk but a row's last, into the scratch), "pcen_carry"
 *                        (one lane a (row, band): s_(c+1) = fmaf(q[255], s_c, p_c), the entering states into the scratch), "pcen_apply"
 *                        (p again, S, the compression, the stores, state_out: four lanes a chain, each runs p from the chunk's start, the
                        same chain and the same bits, and compresses 64 frames of its own, since the compression is some 170 vector
                        operations a value and p is two)
 *         "pcen_single"  (T <= 256), one launch: "pcen_apply" with the entering state read directly; no scratch
 *     No workgroup waits for another and there are no atomics.  The plane is read twice and written once.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_PCEN_CHUNK 256
#define JSGX_PCEN_MAX_BANDS 65536
#define JSGX_PCEN_MAX_CHAINS 68719476736           /* 2^36: rows * ceil(n_frames / JSGX_PCEN_CHUNK) * n_bands; four lanes a chain at the most */
#define JSGX_PCEN_THREADS 256

typedef struct jsgx_pcen_args {
    const float* in;            /* device floats: M */
    int64_t frame_pitch;        /* >= n_bands */
    int64_t row_pitch;          /* rows > 1: >= (n_frames - 1) * frame_pitch + n_bands */
    const float* decay;         /* device floats: q, JSGX_PCEN_CHUNK of them, from jsgx_pcen_decay_build(b) */
    const float* state_in;      /* device floats [rows][n_bands] or NULL: the first frame is the state */
    int64_t state_in_pitch;     /* rows > 1: >= n_bands */
    float* state_out;           /* device floats [rows][n_bands] or NULL */
    int64_t state_out_pitch;    /* rows > 1: >= n_bands */
    float* smooth_out;          /* device floats: S, or NULL */
    int64_t smooth_frame_pitch; /* >= n_bands */
    int64_t smooth_row_pitch;   /* rows > 1: covers a plane */
    float* out;                 /* device floats */
    int64_t out_frame_pitch;    /* >= n_bands */
    int64_t out_row_pitch;      /* rows > 1: covers a plane */
    int32_t rows;               /* 1..65535 */
    int32_t n_bands;            /* B, 1..JSGX_PCEN_MAX_BANDS */
    int32_t n_frames;           /* T, 1..2^31-1 */
    float b;                    /* in (0, 1]; decay was built from the same b */
    float gain;                 /* >= 0 */
    float bias;                 /* >= 0 */
    float power;                /* > 0 */
    float eps;                  /* > 0 */
} jsgx_pcen_args;               /* 144 bytes, no padding */

/* The table q on the host (no device): out[j] = (float)pow((double)fl(1.0f - b), j + 1), j = 0..JSGX_PCEN_CHUNK-1.
 * JSGX_ERR_INVALID: a null out; a b that is not finite or lies outside (0, 1]. */
JSGX_API int jsgx_pcen_decay_build(float b, float* out);
/* The bytes of scratch the launch needs: 0 where n_frames <= JSGX_PCEN_CHUNK, else 4 * rows * ceil(n_frames / 256) * n_bands.  A larger
 * scratch changes nothing.  Refused (a negative jsgx_status): what the launch refuses before it looks at the scratch. */
JSGX_API int64_t jsgx_pcen_scratch_bytes(const jsgx_pcen_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing
 * enqueued), in this order and before any device call: null args, a null in, a null decay, a null out; a pointer (the optional ones
 * included) that is not 4-byte aligned; rows outside 1..65535, n_bands outside 1..65536, n_frames below 1, more than
 * JSGX_PCEN_MAX_CHAINS chains; frame_pitch below n_bands, row_pitch that does not cover a plane (rows > 1); state_in_pitch and then
 * state_out_pitch below n_bands (where the buffer is given and rows > 1); the same two for smooth_out (where given) and for out; b not
 * finite or outside (0, 1]; gain, then bias, negative or not finite; power, then eps, not finite or not positive; out, then smooth_out,
 * then state_out overlapping in, decay, state_in in this order; out overlapping smooth_out, out overlapping state_out, smooth_out
 * overlapping state_out; and where the scratch size is not 0: a null scratch, a scratch that is not 4-byte aligned, scratch_bytes
 * below the size, the scratch (the bytes of that size) overlapping in, decay, state_in, out, smooth_out, state_out in this order.
 * Then JSGX_ERR_NO_DEVICE without a HIP device.  That decay holds the table of b is the caller's to see to. */
JSGX_API int jsgx_pcen_launch(const jsgx_pcen_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the form ("pcen_single" or "pcen_chunked"), JSGX_PCEN_THREADS, the bytes of LDS (0), the
 * launches (1 or 3) and the chunks of a row.  Any output pointer may be NULL (name: else name_len >= 16).  Refused: a name_len below
 * 16 with a name, then what the scratch size refuses. */
JSGX_API int jsgx_pcen_plan(const jsgx_pcen_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches,
                            int32_t* chunks);

/* Section 14 was added to version 1 in the same way: sections 1 to 13, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 14. Peak picking and onset backtracking (librosa.util.peak_pick, librosa.onset.onset_detect, librosa.onset.onset_backtrack): at which
 *     frames of an envelope are the onsets.  The input is what jsg_onset_strength_launch (jsg.h section 2j) writes, taken as it is:
 *         x[t] = in[r*in_pitch + t],  r < rows, t < T (n_frames)
 *     and, for backtracking, an optional energy plane e[t] = energy[r*energy_pitch + t].  Rows are independent.  The four reaches
 *     pre_max, post_max, pre_avg, post_avg (0..JSGX_PEAK_MAX_REACH) and wait (0..JSGX_PEAK_MAX_FRAMES) are integers in frames, delta is
 *     a finite float32.  All arithmetic is float32, every operation rounded on its own (no contraction), and every result is an
 *     integer: a restatement on the CPU gives the same integers (tests/peak_ref.py).  No result depends on the number of rows, on the
 *     pitches, on which optional outputs are NULL or on the form of the kernels.
 *
 *     Refused row.  A row with a NaN or an infinity in x, or in e where energy is given, has n_peaks[r] = -1 and nothing else is
 *     written for it (not its candidates, not its peaks).  The other rows are as if it were not there.
 *
 *     Normalise.  normalise = 1: mn and mx are the row's minimum and maximum (they depend on no order), range = fl(mx - mn) and
 *         y[t] = fl(fl(x[t] - mn) / range)   (the divide correctly rounded);   y = +0 everywhere where range == 0
 *     normalise = 0: y = x.  The sign of a zero of y is never observable: y is only compared, and summed from +0.  A finite row
 *     whose mx - mn overflows is outside the contract; the launch still ends and writes only that row's outputs.
 *
 *     Candidate.  Two windows, inclusive and clipped to the row (nothing outside the row is read or padded):
 *         Wm(t) = [max(0, t - pre_max), min(T-1, t + post_max)]      Wa(t) = [max(0, t - pre_avg), min(T-1, t + post_avg)]
 *         top(t): y[t] >= y[j] for every j in Wm(t)                  (equal neighbours are candidates on both sides)
 *         acc = +0;  for j ascending over Wa(t): acc = fl(acc + y[j]);   avg = fl(acc / (float)|Wa(t)|);   thr = fl(avg + delta)
 *         c[t] = top(t) and y[t] >= thr
 *     c goes to the optional plane candidate[r*candidate_pitch + t] as bytes 0 / 1.
 *
 *     Wait rule (greedy, librosa's).  E = 0; for t ascending: if c[t] and t >= E then t is a peak and E = t + wait + 1.  A candidate
 *     inside a wait is dropped, not deferred.
 *
 *     Backtrack (where energy is given).  Frame 0 is a minimum; frame t in 1..T-2 is one iff e[t] <= e[t-1] and e[t] < e[t+1]; frame
 *     T-1 never is (T = 1 has frame 0).  back(p) is the largest minimum <= p.  Two peaks may share one: duplicates are kept, the list
 *     is non-decreasing.
 *
 *     Outputs.  n_peaks[r] = n, the whole count, which may exceed max_peaks.  peaks[r*peaks_pitch + i], i < min(n, max_peaks),
 *     ascending: where the list is cut the earliest peaks are kept.  backtracked[r*peaks_pitch + i] = back(peaks[i]) where given;
 *     it needs energy and energy needs it.  Nothing behind the written entries is touched.
 *
 *     Known answers.  An all-zero row with delta <= 0: every frame is a candidate, the peaks are 0, w+1, 2(w+1), ... (w = wait) and
 *     n = ceil(T / (w+1)).  An all-zero row with delta > 0, or any constant row with normalise = 1 and delta > 0: no candidate,
 *     n = 0.  Unit impulses every 6 frames from frame 0, reaches (1, 1, 2, 2), delta = 0.07: the peaks are every
 *     6 * ceil((wait + 1) / 6) frames from 0, which tells wait = 5 (every 6) from wait = 6 (every 12).  T = 1: frame 0 is a candidate
 *     iff 0 >= delta (normalised) or x[0] >= fl(x[0] + delta) (not normalised).
 *
 *     Deliberate differences from librosa: the windows are clipped at both ends of the row (librosa treats frame 0 on its own, and
 *     older versions padded with the row's minimum); reaches and wait are whole frames with post_max and post_avg inclusive (the
 *     Python layer converts seconds); normalise divides by mx - mn with no tiny added; float32 throughout.  Agreement with librosa
 *     itself is not measured.
 *
 *     The kernels.  A row is cut into blocks of B = JSGX_PEAK_BLOCK frames; workgroups of JSGX_PEAK_THREADS lanes, no atomics, no
 *     workgroup waits for another.  The wait rule in parallel: with nxt(t) the first candidate >= t, a chain that enters a block at
 *     frame E picks nxt(E) first and from there on depends on that pick alone: s(p) = nxt(p + wait + 1) inside the block.  The
 *     tables s^(2^k), k < log2 B, built in LDS by squaring, give the count and the last pick of the chain from any p in log2 B steps
 *     and its i-th pick in as many.  A chain enters a block at an offset of at most min(wait, B - 1).
 *         "peak_blocked" (T > B), five launches: "peak_stats" (minimum, maximum and the non-finite vote of every block), "peak_row"
 *                        (a workgroup a row: the row's three out of its blocks'), "peak_cand" (a workgroup a block: y with a halo
 *                        of the largest reach into LDS, the candidates by direct evaluation, the tables, and for every entering
 *                        offset the count and the last pick; the block's last energy minimum), "peak_carry" (a lane a row walks
 *                        the blocks: the entering frame, the running count and the last minimum so far of every block; a wait
 *                        longer than a block is skipped by arithmetic, no table is read for it), "peak_emit" (a workgroup a block:
 *                        the tables again from the stored candidates, lane i writes the block's i-th pick and its back())
 *         "peak_single"  (T <= B), one launch, no scratch: a workgroup a row does all of it from LDS; with T <= 64 a wavefront a
 *                        row, four rows a workgroup
 *     JSGX_PEAK_BLOCK was chosen among 256, 512, 1024 and 2048 by measurement (profiles/peak_bench.md, tools/peak_bench.py).
 * ------------------------------------------------------------------------------------------------ */
#ifndef JSGX_PEAK_BLOCK
#define JSGX_PEAK_BLOCK 1024               /* a power of two, 256..2048 */
#endif
#define JSGX_PEAK_MAX_REACH 256
#define JSGX_PEAK_MAX_FRAMES 16777216      /* 2^24 */
#define JSGX_PEAK_THREADS 256
#define JSGX_PEAK_SHORT 64                 /* up to this many frames a wavefront takes a row of "peak_single" */
#define JSGX_PEAK_LOG2_BLOCK (JSGX_PEAK_BLOCK == 256 ? 8 : JSGX_PEAK_BLOCK == 512 ? 9 : JSGX_PEAK_BLOCK == 1024 ? 10 : 11)
/* static, of "peak_cand", "peak_emit" and "peak_single": log2 B tables of B 16-bit offsets (y and its halo lie there first), nxt
 * (B + 4 of them), the last minimum of every frame (B of them): 24584 bytes at B = 1024, 53256 at B = 2048 */
#define JSGX_PEAK_LDS_BYTES (2 * JSGX_PEAK_BLOCK * JSGX_PEAK_LOG2_BLOCK + 2 * (JSGX_PEAK_BLOCK + 4) + 2 * JSGX_PEAK_BLOCK)
#define JSGX_PEAK_LDS_LIMIT 163840

typedef struct jsgx_peak_args {
    const float* in;            /* device floats: x */
    int64_t in_pitch;           /* rows > 1: >= n_frames */
    const float* energy;        /* device floats: e, or NULL (then backtracked is NULL) */
    int64_t energy_pitch;       /* rows > 1: >= n_frames */
    uint8_t* candidate;         /* device bytes: c, or NULL */
    int64_t candidate_pitch;    /* rows > 1: >= n_frames */
    int32_t* peaks;             /* device int32 [rows][max_peaks] */
    int32_t* backtracked;       /* device int32 [rows][max_peaks] at peaks_pitch, or NULL (then energy is NULL) */
    int64_t peaks_pitch;        /* rows > 1: >= max_peaks */
    int32_t* n_peaks;           /* device int32 [rows] */
    int32_t rows;               /* 1..65535 */
    int32_t n_frames;           /* T, 1..JSGX_PEAK_MAX_FRAMES */
    int32_t pre_max;            /* 0..JSGX_PEAK_MAX_REACH, and so the next three */
    int32_t post_max;
    int32_t pre_avg;
    int32_t post_avg;
    float delta;                /* finite */
    int32_t wait;               /* 0..JSGX_PEAK_MAX_FRAMES */
    int32_t normalise;          /* 0 or 1 */
    int32_t max_peaks;          /* 1..JSGX_PEAK_MAX_FRAMES */
} jsgx_peak_args;               /* 120 bytes, no padding */

/* The bytes of scratch the launch needs: 0 where n_frames <= B, else with nb = ceil(n_frames / B)
 *     rows * nb * (32 + 4 * min(wait + 1, B) + B)
 * (a record of 32 bytes a block, a word for every entering offset of a block, a byte a frame of whole blocks): below 16 bytes a frame plus
 * 32 a block a row.  A larger scratch changes nothing.  Refused (a negative jsgx_status): what the launch refuses before it looks at the
 * scratch. */
JSGX_API int64_t jsgx_peak_scratch_bytes(const jsgx_peak_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing
 * enqueued), in this order and before any device call: null args, a null in, a null peaks, a null n_peaks; in, energy, peaks,
 * backtracked or n_peaks not 4-byte aligned (candidate is bytes); rows outside 1..65535, n_frames outside 1..2^24; pre_max, post_max,
 * pre_avg, post_avg outside 0..256 in this order; delta not finite; wait outside 0..2^24; normalise not 0 or 1; max_peaks outside
 * 1..2^24; backtracked without energy or energy without backtracked; with rows > 1: in_pitch, then energy_pitch, then candidate_pitch
 * below n_frames (where the buffer is given), peaks_pitch below max_peaks; peaks, then backtracked, then n_peaks, then candidate
 * overlapping in and then energy; peaks overlapping backtracked, n_peaks, candidate; backtracked overlapping n_peaks, candidate; n_peaks
 * overlapping candidate; and where the scratch size is not 0: a null scratch, a scratch that is not 4-byte aligned, scratch_bytes below
 * the size, the scratch (the bytes of that size) overlapping in, energy, peaks, backtracked, n_peaks, candidate in this order.  Then
 * JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_peak_launch(const jsgx_peak_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the form ("peak_single" or "peak_blocked"), JSGX_PEAK_THREADS, the bytes of LDS
 * (JSGX_PEAK_LDS_BYTES), the launches (1 or 5) and the blocks of a row.  Any output pointer may be NULL (name: else name_len >= 16).
 * Refused: a name_len below 16 with a name, then what the scratch size refuses. */
JSGX_API int jsgx_peak_plan(const jsgx_peak_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches,
                            int32_t* blocks);

/* Sections 15 and 16 were added to version 1 in the same way: sections 1 to 14, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 15. Aggregation of a plane over segments (librosa.util.sync): one row of the output for every stretch of frames between two
 *     boundaries.  The plane is frame-major, what the feature kernels write,
 *         X[t][f] = x[p*x_pair_pitch + t*x_frame_pitch + f],  p < pairs, t < N (n_frames), f < F (n_features)
 *     and the boundaries are frames b[i] = bounds[p*bounds_pitch + i] with a count of their own per pair: the beats / n_beats of
 *     section 1 or the peaks, backtracked / n_peaks of section 14, taken as they are.  A bounds_pitch of 0 is one list for every pair.
 *     The count of a pair is m = min(n_bounds[p], max_bounds); with n_bounds NULL, m = bounds_all for every pair.
 *
 *     Segments (kernel "sync_segments", a workgroup a pair).
 *     Refused pair.  n_bounds[p] < 0 (the -1 of a refused row upstream), or b[i] < b[i-1] for some i < m on the raw values:
 *     n_segments[p] = -1 and nothing else is written for the pair, neither its segments nor its output rows.  Otherwise
 *         c[i] = min(max(b[i], 0), N)
 *         s    = (0 where pad = 1), c[0], ..., c[m-1], (N where pad = 1)
 *         u    = s without every entry that equals its predecessor:  u[0] < u[1] < ... < u[U-1]
 *         n_segments[p] = max(U - 1, 0)                      the whole count, which may exceed max_segments
 *         segments[p*segments_pitch + j] = u[j],  j <= min(U - 1, max_segments), where U >= 2; nothing behind these entries is written
 *     Segment o is the frames u[o] .. u[o+1]-1, cnt = u[o+1] - u[o] >= 1 of them.  segments holds max_segments + 1 entries a pair.
 *
 *     Aggregate (kernel "sync_aggregate"), for o < min(n_segments[p], max_segments) and every f:
 *     out[p*out_pair_pitch + o*out_frame_pitch + f] is
 *         JSGX_SYNC_MEAN    the segment is cut from its start into chunks of JSGX_SYNC_CHUNK frames; part_j is the chain
 *                           acc = fl(acc + X[t][f]) from +0 over the frames of chunk j ascending, tot the chain fl(tot + part_j) from
 *                           +0 over j ascending, the value fl(tot / (float)cnt), the divide correctly rounded.  The order depends on
 *                           nothing but cnt.
 *         JSGX_SYNC_MIN,    the least and the greatest under the order of key(v): the bits of v, all of them flipped where the sign
 *         JSGX_SYNC_MAX     is set, else the sign alone (-0 < +0, the infinities at the ends).  No order of evaluation shows.
 *         JSGX_SYNC_MEDIAN  with v[0..cnt-1] the segment's values sorted by key: v[(cnt-1)/2] for an odd cnt, else
 *                           0.5f * fl(v[cnt/2 - 1] + v[cnt/2]), the formula of section 7's bandwidth.  A sum that overflows gives the
 *                           infinity: stated, not avoided.
 *     NaN.  Min, max and median of a segment with a NaN at feature f are the bits JSGX_SYNC_NAN_BITS there; a mean that is a NaN, and
 *     an even median whose two middle values are the two infinities, is written as those bits.  Every output is comparable bit for
 *     bit (tests/sync_ref.py restates both kernels in numpy).  Nothing depends on pairs, on the pitches or on the form of the kernel.
 *
 *     Deliberate differences from librosa.util.sync: frame-major planes; boundaries are clipped to 0..N, where librosa raises on a
 *     negative one; a non-decreasing list is required, where librosa sorts; these four aggregates only; float32.  Agreement with
 *     librosa itself is not measured.
 *
 *     The kernel.  Workgroups of JSGX_SYNC_THREADS lanes, lane = feature (64 features a workgroup, reads coalesced along f), four
 *     segments a workgroup; no atomics, no workgroup waits for another; a workgroup whose first segment is behind the pair's count
 *     leaves after one uniform read.  Where none of its segments is longer than JSGX_SYNC_WAVE_MAX frames (median) or JSGX_SYNC_CHUNK
 *     (the other three), a wavefront takes a segment on its own.  Otherwise the four wavefronts take the segments one after the other
 *     together: for the mean wavefront w takes the chunks j = w (mod 4) and the partials are added in ascending order from LDS, for the
 *     others it takes the frames t = w (mod 4).  The median is a bitwise selection, no sort: 32 counting passes over the keys, most
 *     significant bit first, find the k-th smallest, and for an even cnt one more pass finds its successor.  A segment of up to
 *     JSGX_SYNC_WAVE_MAX frames (a wavefront alone) or JSGX_SYNC_STAGE frames (the four together) is staged in LDS as keys, a longer
 *     one is read again through the caches.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_SYNC_MEAN 0
#define JSGX_SYNC_MIN 1
#define JSGX_SYNC_MAX 2
#define JSGX_SYNC_MEDIAN 3
#define JSGX_SYNC_CHUNK 256                /* frames of a partial sum of the mean; the longest segment a wavefront takes alone */
#ifndef JSGX_SYNC_WAVE_MAX                 /* the two thresholds of the median can be set at build time, for tools/sync_bench.py */
#define JSGX_SYNC_WAVE_MAX 64              /* median: the longest segment a wavefront takes alone, staged in its quarter of the tile */
#endif
#ifndef JSGX_SYNC_STAGE
#define JSGX_SYNC_STAGE 256                /* median: the longest segment the four wavefronts stage in LDS; at least 4 JSGX_SYNC_WAVE_MAX */
#endif
#define JSGX_SYNC_THREADS 256
#define JSGX_SYNC_MAX_FRAMES 16777216      /* 2^24 */
#define JSGX_SYNC_MAX_FEATURES 65536
#define JSGX_SYNC_MAX_BOUNDS 1048576       /* 2^20 */
#define JSGX_SYNC_MAX_SEGMENTS 1048577     /* 2^20 + 1 */
#define JSGX_SYNC_NAN_BITS 0x7FC00000u
#define JSGX_SYNC_LDS_BYTES 4096           /* static, of "sync_aggregate": what the four wavefronts hand each other, two rounds */
#define JSGX_SYNC_LDS_TILE 65536           /* dynamic, median only: JSGX_SYNC_STAGE = 256 frames of 64 keys */

typedef struct jsgx_sync_args {
    const float* x;             /* device floats: X */
    int64_t x_frame_pitch;      /* >= n_features */
    int64_t x_pair_pitch;       /* pairs > 1: covers a plane */
    const int32_t* bounds;      /* device int32 [pairs][max_bounds]; may be NULL where max_bounds == 0 */
    int64_t bounds_pitch;       /* pairs > 1: 0 (one list for every pair) or >= max_bounds */
    const int32_t* n_bounds;    /* device int32 [pairs], or NULL: bounds_all for every pair */
    int32_t* segments;          /* device int32 [pairs][max_segments + 1]: u */
    int64_t segments_pitch;     /* pairs > 1: >= max_segments + 1 */
    int32_t* n_segments;        /* device int32 [pairs] */
    float* out;                 /* device floats [pairs][max_segments][n_features] */
    int64_t out_frame_pitch;    /* >= n_features */
    int64_t out_pair_pitch;     /* pairs > 1: covers max_segments rows */
    int32_t pairs;              /* 1..65535 */
    int32_t n_frames;           /* N, 1..JSGX_SYNC_MAX_FRAMES */
    int32_t n_features;         /* F, 1..JSGX_SYNC_MAX_FEATURES */
    int32_t max_bounds;         /* 0..JSGX_SYNC_MAX_BOUNDS */
    int32_t bounds_all;         /* n_bounds NULL: 0..max_bounds; else not looked at */
    int32_t max_segments;       /* 1..JSGX_SYNC_MAX_SEGMENTS */
    int32_t aggregate;          /* JSGX_SYNC_MEAN .. JSGX_SYNC_MEDIAN */
    int32_t pad;                /* 0 or 1 */
    int32_t reserved0;          /* 0 */
    int32_t reserved1;          /* 0 */
} jsgx_sync_args;               /* 136 bytes, no padding beyond the two reserved words */

/* Enqueue only, two kernels and no scratch: segments and n_segments are required outputs and hand the segments from "sync_segments"
 * to "sync_aggregate" (which is not launched where no segment can exist: max_bounds, or bounds_all with n_bounds NULL, + 2 pad < 2).
 * No allocation, no synchronisation; capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing enqueued), in this order and before any device call:
 * null args, a null x, a null out, a null segments, a null n_segments; a null bounds with max_bounds > 0; a pointer (n_bounds
 * included) that is not 4-byte aligned; pairs outside 1..65535, n_frames outside 1..2^24, n_features outside 1..65536; max_bounds
 * outside 0..2^20; with n_bounds NULL, bounds_all outside 0..max_bounds; max_segments outside 1..2^20+1; aggregate outside 0..3; pad not
 * 0 or 1; reserved0 or reserved1 not 0; x_frame_pitch below n_features, x_pair_pitch that does not cover a plane (pairs > 1); the
 * same two for out (a plane of max_segments rows); with pairs > 1: bounds_pitch neither 0 nor >= max_bounds (where bounds is given),
 * segments_pitch below max_segments + 1; out, then segments, then n_segments overlapping x, bounds, n_bounds in this order; out
 * overlapping segments, out overlapping n_segments, segments overlapping n_segments.  Then JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_sync_launch(const jsgx_sync_args* args, void* stream);
/* What the launch enqueues, without a device: the aggregate's kernel ("sync_mean", "sync_min", "sync_max" or "sync_median"),
 * JSGX_SYNC_THREADS, the bytes of LDS of a workgroup (JSGX_SYNC_LDS_BYTES, with the median JSGX_SYNC_LDS_TILE more) and the launches (2,
 * or 1).  Any output pointer may be NULL (name: else name_len >= 16).  Refused: a name_len below 16 with a name, then what the launch
 * refuses. */
JSGX_API int jsgx_sync_plan(const jsgx_sync_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes, int32_t* n_launches);

/* ------------------------------------------------------------------------------------------------
 * 16. Time-delay embedding (librosa.feature.stack_memory): n_steps copies of a frame-major plane side by side, each delayed further,
 *         out[p*out_pair_pitch + t*out_frame_pitch + s*F + f] = X[t - s*delay][f],   s < n_steps, t < N, f < F
 *     the link between section 15 and the recurrence plane of section 7.  A negative delay stacks the future, as librosa does.  Where
 *     t - s*delay is outside 0..N-1, JSGX_STACK_CONSTANT writes fill and JSGX_STACK_EDGE writes X[clamp(t - s*delay, 0, N-1)][f].  A
 *     pure permutation: bits are copied unchanged, NaN payloads included, fill's too.  Kernel "stack_memory": one launch, workgroups of
 *     JSGX_STACK_THREADS lanes, each a run of whole frames of the output, lanes along the row; no LDS.  Frame-major, where librosa
 *     stacks along the first axis of a feature-major plane; float32.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_STACK_CONSTANT 0
#define JSGX_STACK_EDGE 1
#define JSGX_STACK_MAX_STEPS 256
#define JSGX_STACK_MAX_DELAY 16777216      /* 2^24 */
#define JSGX_STACK_MAX_WIDTH 1048576       /* 2^20: n_steps * n_features */
#define JSGX_STACK_THREADS 256

typedef struct jsgx_stack_memory_args {
    const float* x;             /* device floats: X */
    int64_t x_frame_pitch;      /* >= n_features */
    int64_t x_pair_pitch;       /* pairs > 1: covers a plane */
    float* out;                 /* device floats [pairs][n_frames][n_steps * n_features] */
    int64_t out_frame_pitch;    /* >= n_steps * n_features */
    int64_t out_pair_pitch;     /* pairs > 1: covers a plane */
    int32_t pairs;              /* 1..65535 */
    int32_t n_frames;           /* N, 1..2^24 */
    int32_t n_features;         /* F, 1..65536 */
    int32_t n_steps;            /* 1..JSGX_STACK_MAX_STEPS, n_steps * n_features <= JSGX_STACK_MAX_WIDTH */
    int32_t delay;              /* not 0, |delay| <= JSGX_STACK_MAX_DELAY */
    int32_t mode;               /* JSGX_STACK_CONSTANT or JSGX_STACK_EDGE */
    float fill;                 /* JSGX_STACK_CONSTANT: the value outside, any bits */
    int32_t reserved0;          /* 0 */
} jsgx_stack_memory_args;       /* 80 bytes, no padding */

/* Enqueue only, one kernel and no scratch; capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing enqueued), in
 * this order and before any device call: null args, a null x, a null out; a pointer that is not 4-byte aligned; pairs outside
 * 1..65535, n_frames outside 1..2^24, n_features outside 1..65536; n_steps outside 1..256, n_steps * n_features above 2^20; delay 0 or
 * |delay| above 2^24; mode not 0 or 1; reserved0 not 0; x_frame_pitch below n_features, x_pair_pitch that does not cover a plane
 * (pairs > 1); out_frame_pitch below n_steps * n_features, out_pair_pitch that does not cover a plane; out overlapping x.  Then
 * JSGX_ERR_NO_DEVICE without a HIP device. */
JSGX_API int jsgx_stack_memory_launch(const jsgx_stack_memory_args* args, void* stream);

/* Section 17 was added to version 1 in the same way: sections 1 to 16, their structs and their constants are as they were. */

/* ------------------------------------------------------------------------------------------------
 * 17. Temporally constrained agglomerative segmentation (librosa.segment.agglomerative and librosa.segment.subsegment): Ward clustering
 *     of the frames of a plane in which a cluster is a run of consecutive frames and every step merges two neighbours.  The plane is
 *     section 15's, frame-major, X[t][f] = x[p*x_pair_pitch + t*x_frame_pitch + f], and so are the boundary inputs, with the same names
 *     and meanings: bounds, bounds_pitch (0: one list for every pair), n_bounds, max_bounds, bounds_all, pad.  The list u[0] < ... <
 *     u[U-1] is built by section 15's rule (one copy of it serves both sections) and goes to segments / n_segments as there.  Each
 *     stretch o, the frames u[o] .. u[o+1]-1 (len of them), is clustered on its own into min(k, len) clusters, k = n_clusters >= 1.
 *     max_bounds = 0 with pad = 1 is the one stretch 0..N: librosa.segment.agglomerative.  A list of beats: librosa.segment.subsegment.
 *     max_segments must cover every stretch the list can give: min(n_frames, entries - 1) with entries = max_bounds (bounds_all where
 *     n_bounds is NULL) + 2 pad, so that every stretch is handed on through segments.
 *
 *     Definition.  A cluster C has a start frame, a count m_C and float32 sums S_C[f].  A frame alone: S = X[t][f], m = 1.  Merging the
 *     left cluster A with its right neighbour B: S[f] = fl(S_A[f] + S_B[f]), m = m_A + m_B.  The mean is M_C[f] = fl(S_C[f] / (float)m_C),
 *     the divide correctly rounded.  The cost of a pair of neighbours A (left), B (right):
 *         d_f  = fl(M_A[f] - M_B[f])
 *         q_l  = fmaf(d_f, d_f, q_l) from +0 over f = l, l + 64, ... ascending, for each lane l < 64 (a lane with no feature: +0)
 *         q_l  = fl(q_l + q_{l xor s}) for s = 32, 16, 8, 4, 2, 1: the same value Q in every lane
 *         w    = fl(fl((float)m_A * (float)m_B) / (float)(m_A + m_B)),  cost = fl(w * Q);  a cost that is a NaN is JSGX_SYNC_NAN_BITS
 *     The order depends on F alone.  A step: among the pairs of neighbours take the least under section 15's key() of the cost bits (a
 *     total order on every bit pattern: an overflowed sum that makes a cost an infinity or the NaN still sorts, the NaN last), a tie to
 *     the lower start frame; merge the pair; recompute the costs to its two neighbours.  Stop at min(k, len) clusters.  All of this is
 *     float32 with every operation rounded on its own; tests/agglo_ref.py restates it in numpy and every output is compared as bits.
 *     Nothing depends on pairs, on the pitches, on the form of the kernel or on how the minimum is searched.
 *
 *     Outputs.  out_bounds[p*out_pitch + i], int32: the start frames of the final clusters of all stretches of the pair, ascending, the
 *     stretches one behind the other: stretch o begins at index sum over o' < o of min(k, len_o') with the entry u[o].  Entries at or
 *     beyond max_out are not written.  n_out[p]: the whole count.  segments, n_segments: as in section 15 (required).  order (int32)
 *     and height (float32), [pairs][n_frames] at tree_pitch, both or neither: step j of stretch o writes the boundary it removes (the
 *     start of B) and its cost at index u[o] + j; no other entry is touched.  With k = 1 that is the whole dendrogram of a stretch: the
 *     clusters for any k' are u[o] and the boundaries removed by its last k' - 1 steps.
 *
 *     Refused pair: n_out[p] = -1 and nothing else is written for the pair except n_segments, where n_bounds[p] < 0 or the list
 *     decreases (n_segments[p] = -1, as in section 15); where a value in the frames u[0] .. u[U-1]-1 of the pair is a NaN or an
 *     infinity; where a stretch is longer than JSGX_AGGLO_MAX_STRETCH.  In the last two cases segments and n_segments are written.
 *
 *     Deliberate differences from librosa / scikit-learn: frame-major planes; a tie goes to the lower frame (sklearn: its heap's
 *     order); float32 (sklearn: float64); boundaries are clipped and a non-decreasing list is required, as in section 15; Ward linkage
 *     on a chain only: no other linkage, no distance threshold in place of k, no other connectivity.  The greedy merge of neighbours
 *     gave scikit-learn's boundaries on every plane of tests/test_agglo_ref.py.  Agreement with librosa itself is not measured.
 *
 *     The kernels.  No atomics, no workgroup waits for another; a stretch is served by one wavefront, so no barrier stands in a step.
 *         "agglo_segments"  a workgroup a pair: section 15's rule
 *         "agglo_copy"      a wavefront a frame, lane = feature, JSGX_AGGLO_COPY_FRAMES frames a workgroup: X into the plane of sums in
 *                           the scratch, the cost of every frame with its successor, and the workgroup's non-finite vote
 *         "agglo_offsets"   a workgroup a pair: the votes, the over-long stretches, the prefix sums of min(k, len), n_out
 *         "agglo_wave"      stretches of up to JSGX_AGGLO_SHORT frames, four to a workgroup of 256 lanes, a wavefront each: the costs (as
 *                           keys) and 16-bit left / right links one per lane in LDS, the minimum one reduction over (key, frame)
 *         "agglo_group"     longer stretches, a workgroup of one wavefront each: keys and links of every frame in LDS (8 bytes a frame)
 *                           and a minimum (key, frame) for every block of 64 frames.  A merge dirties at most three blocks: a step is a
 *                           reduction over the block minima and one over each dirty block, not a sweep.  Launched where n_frames >
 *                           JSGX_AGGLO_SHORT; a workgroup whose stretch is short leaves at once, as "agglo_wave" leaves the long ones.
 *     The sums of the touched clusters are read and written through the caches, lane = feature; a step reads four rows and writes one.
 *     A launch is len - k dependent steps a stretch and is bound by their latency.  Measured on one MI355X (profiles/agglo_bench.md,
 *     tools/agglo_bench.py): a step of "agglo_wave" takes 1.2 to 1.3 microseconds, a step of "agglo_group" 1.8 to 2.1 (20 to 128
 *     features); 24448 stretches of 43 frames to four clusters each (64 x 16384 x 128) take 0.86 ms.
 * ------------------------------------------------------------------------------------------------ */
#define JSGX_AGGLO_MAX_STRETCH 16384       /* the longest stretch: 8 bytes of LDS a frame and 8 a block of 64 are 133120 bytes */
#define JSGX_AGGLO_SHORT 64                /* up to this many frames a stretch is one of four in a workgroup of "agglo_wave" */
#define JSGX_AGGLO_THREADS 256             /* all kernels but "agglo_group" */
#define JSGX_AGGLO_GROUP_THREADS 64        /* "agglo_group" */
#define JSGX_AGGLO_COPY_FRAMES 64          /* frames of a workgroup of "agglo_copy": one vote each */
#define JSGX_AGGLO_MAX_OUT 16777216        /* 2^24 */
#define JSGX_AGGLO_LDS_BYTES 2048          /* static, of "agglo_wave": 8 bytes a frame, four stretches */
#define JSGX_AGGLO_LDS_LIMIT 133120        /* dynamic, of "agglo_group", at most: 8 L + 8 ceil(L / 64) for L = min(n_frames, JSGX_AGGLO_MAX_STRETCH) */

typedef struct jsgx_agglomerative_args {
    const float* x;             /* device floats: X */
    int64_t x_frame_pitch;      /* >= n_features */
    int64_t x_pair_pitch;       /* pairs > 1: covers a plane */
    const int32_t* bounds;      /* device int32 [pairs][max_bounds]; may be NULL where max_bounds == 0 */
    int64_t bounds_pitch;       /* pairs > 1: 0 (one list for every pair) or >= max_bounds */
    const int32_t* n_bounds;    /* device int32 [pairs], or NULL: bounds_all for every pair */
    int32_t* segments;          /* device int32 [pairs][max_segments + 1]: u */
    int64_t segments_pitch;     /* pairs > 1: >= max_segments + 1 */
    int32_t* n_segments;        /* device int32 [pairs] */
    int32_t* out_bounds;        /* device int32 [pairs][max_out] */
    int64_t out_pitch;          /* pairs > 1: >= max_out */
    int32_t* n_out;             /* device int32 [pairs] */
    int32_t* order;             /* device int32 [pairs][n_frames], or NULL (then height is NULL) */
    float* height;              /* device floats [pairs][n_frames], or NULL (then order is NULL) */
    int64_t tree_pitch;         /* pairs > 1 and order given: >= n_frames */
    int32_t pairs;              /* 1..65535 */
    int32_t n_frames;           /* N, 1..2^24 */
    int32_t n_features;         /* F, 1..65536 */
    int32_t max_bounds;         /* 0..JSGX_SYNC_MAX_BOUNDS */
    int32_t bounds_all;         /* n_bounds NULL: 0..max_bounds; else not looked at */
    int32_t max_segments;       /* 1..JSGX_SYNC_MAX_SEGMENTS, and every stretch the list can give */
    int32_t max_out;            /* 1..JSGX_AGGLO_MAX_OUT */
    int32_t n_clusters;         /* k >= 1 */
    int32_t pad;                /* 0 or 1 */
    int32_t reserved0;          /* 0 */
} jsgx_agglomerative_args;      /* 160 bytes, no padding beyond the reserved word */

/* The bytes of scratch the launch needs, with S the stretches max_segments must cover and V = ceil(n_frames / JSGX_AGGLO_COPY_FRAMES):
 *     4 * pairs * (n_frames * n_features + n_frames + V + S + 1)
 * (the plane of sums, a cost a frame, a vote a workgroup of "agglo_copy", an offset a stretch, a verdict a pair).  The layout is private,
 * the contents on entry are undefined, a larger scratch changes nothing.  Refused (a negative jsgx_status): what the launch refuses
 * before it looks at the scratch. */
JSGX_API int64_t jsgx_agglomerative_scratch_bytes(const jsgx_agglomerative_args* args);
/* Enqueue only: no allocation, no synchronisation; capture works, a first launch included.  Refused (JSGX_ERR_INVALID, nothing
 * enqueued), in this order and before any device call: null args, a null x, a null segments, a null n_segments, a null out_bounds, a
 * null n_out; a null bounds with max_bounds > 0; order without height or height without order; a pointer that is not 4-byte aligned;
 * pairs outside 1..65535, n_frames outside 1..2^24, n_features outside 1..65536; max_bounds outside 0..2^20; with n_bounds NULL,
 * bounds_all outside 0..max_bounds; max_segments outside 1..2^20+1; max_out outside 1..2^24; n_clusters below 1; pad not 0 or 1;
 * reserved0 not 0; max_segments below the stretches the list can give; n_frames above JSGX_AGGLO_MAX_STRETCH where no boundary can
 * come (max_bounds, or bounds_all with n_bounds NULL, is 0) and pad = 1; x_frame_pitch below n_features, x_pair_pitch that does not
 * cover a plane (pairs > 1); with pairs > 1: bounds_pitch neither 0 nor >= max_bounds (where bounds is given), segments_pitch below
 * max_segments + 1, out_pitch below max_out, tree_pitch below n_frames (where order is given); out_bounds, then n_out, segments,
 * n_segments, order, height overlapping x, bounds, n_bounds in this order; any two of those six outputs overlapping, in that order;
 * a null scratch, a scratch that is not 4-byte aligned, scratch_bytes below the size, the scratch (the bytes of that size)
 * overlapping x, bounds, n_bounds, out_bounds, n_out, segments, n_segments, order, height in this order.  Then JSGX_ERR_NO_DEVICE
 * without a HIP device. */
JSGX_API int jsgx_agglomerative_launch(const jsgx_agglomerative_args* args, void* scratch, int64_t scratch_bytes, void* stream);
/* What the launch enqueues, without a device: the form of the merge that takes the longest stretch the shape allows ("agglo_wave" where
 * n_frames <= JSGX_AGGLO_SHORT, else "agglo_group"), its lanes per workgroup (256 or 64), its bytes of LDS (JSGX_AGGLO_LDS_BYTES, or 8 L +
 * 8 ceil(L / 64)) and the launches (5 with "agglo_group", else 4; 2 where the list can give no stretch).  Any output pointer may be NULL
 * (name: else name_len >= 16).  Refused: a name_len below 16 with a name, then what the scratch size refuses. */
JSGX_API int jsgx_agglomerative_plan(const jsgx_agglomerative_args* args, char* name, int name_len, int32_t* threads, int32_t* lds_bytes,
                                     int32_t* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* JSGX_H */
