"""Onset strength, autocorrelation tempogram and tempo (include/jsg.h section 2j): the definitions evaluated in float64, the float32
restatements in the library's stated orders, the per-element cap on the tempogram, the decided tempo cases, the shared signals.  numpy
only; tests/test_rhythm_ref.py checks this module on the CPU, tests/test_gpu_rhythm.py compares the GPU against it.

The restatements: onset strength, lane l of W (64 where B > 32, else the smallest power of two >= B) adds b = l, l + W, ... ascending,
then a halving tree; the tempogram, one accumulator per lag and acc = fmaf(y[j], y[j + tau], acc) for j ascending; tempo, the mean over
the frames in blocks of 64.  The float32 fmaf is emulated exactly as in tests/yin_ref.py: the product is exact in float64, the sum with
the accumulator is rounded to odd in float64 (TwoSum gives the sign of what was lost) and then to nearest in float32.
"""
import functools

import numpy as np

# bound (a) of tests/test_gpu_rhythm.py: GPU error <= YARDSTICKS x the restatement's error on the same signal.  4 before any GPU run;
# afterwards 1.25 x the worst ratio measured by tools/rhythm_accuracy.py, rounded up to the next half (the rule of
# profiles/stft_power_accuracy.md).  Measured on an MI355X: the worst ratio over the cases of tools/rhythm_accuracy.py is 1.000 (the GPU's
# bits equal the restatement's in every element; profiles/rhythm_accuracy.md), so 1.25 x 1.000 rounded up to the next half.
YARDSTICKS = 1.5

U = 2.0 ** -24
FRAME_RATE = 22050.0 / 512.0
# (win_length, envelope length, period, best / runner-up of the float64 score): impulse trains plus a floor of 0.01, the default prior
DECIDED = ((64, 200, 20, 17.0), (384, 600, 20, 1.6), (384, 600, 30, 3.1), (100, 300, 25, 8.9))


def fma32(a, b, acc):
    """float32 fmaf(a, b, acc), exactly (no overflow or underflow of the product in float64: float32 inputs)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)            # 48 bits: exact
        c = np.broadcast_to(acc, p.shape).astype(np.float64)
        s = c + p
        t = s - c
        lost = (c - (s - t)) + (p - t)           # TwoSum: c + p = s + lost exactly
        fix = (lost != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)), s)      # round to odd
        return s.astype(np.float32)


# ---------------------------------------------------------------------------------------------------- onset strength
def _ref_max(prev, m):
    """The clipped maximum filter over the last axis, b' ascending, a NaN stays."""
    B = prev.shape[-1]
    lo, hi = m // 2, (m - 1) // 2
    out = np.empty_like(prev)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            b0, b1 = max(0, b - lo), min(B - 1, b + hi)
            mx = prev[..., b0].copy()
            for c in range(b0 + 1, b1 + 1):
                v = prev[..., c]
                mx = np.where((v > mx) | np.isnan(v), v, mx)
            out[..., b] = mx
    return out


def _flux(S, lag, m):
    """p(b) of the frames t >= lag: [..., T - lag, B] in the type of S."""
    with np.errstate(invalid="ignore"):
        e = S[..., lag:, :] - _ref_max(S[..., :S.shape[-2] - lag, :], m)
        return np.where((e > 0) | np.isnan(e), e, np.zeros((), S.dtype))


def onset64(S, lag=1, m=1):
    """S [..., T, B] float32 -> o [..., T] in float64."""
    S = np.asarray(S, np.float32).astype(np.float64)
    T, B = S.shape[-2:]
    out = np.zeros(S.shape[:-1])
    if T > lag:
        out[..., lag:] = _flux(S, lag, m).sum(axis=-1) / B
    return out


def onset32(S, lag=1, m=1):
    """The float32 restatement: [..., T] float32."""
    S = np.asarray(S, np.float32)
    T, B = S.shape[-2:]
    out = np.zeros(S.shape[:-1], np.float32)
    if T <= lag:
        return out
    W = 64 if B > 32 else 1 << max(0, (B - 1).bit_length())
    p = _flux(S, lag, m)
    acc = np.zeros(p.shape[:-1] + (W,), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b0 in range(0, B, W):
            n = min(W, B - b0)
            acc[..., :n] = acc[..., :n] + p[..., b0:b0 + n]
        s = W // 2
        while s >= 1:
            acc = acc[..., :s] + acc[..., s:2 * s]
            s //= 2
        out[..., lag:] = acc[..., 0] / np.float32(B)
    return out


# ---------------------------------------------------------------------------------------------------- tempogram
def frames(n_in, hop):
    return 1 + (n_in - 1) // hop


def windowed(o, w, hop, n_frames):
    """y of every frame: o [R][T] float32, w [Wn] float32 -> [R][n_frames][Wn] float32, +0 outside the row."""
    o, w = np.atleast_2d(np.asarray(o, np.float32)), np.asarray(w, np.float32)
    R, T = o.shape
    Wn = w.size
    idx = np.arange(n_frames)[:, None] * hop - Wn // 2 + np.arange(Wn)[None, :]
    inside = (idx >= 0) & (idx < T)
    with np.errstate(invalid="ignore", over="ignore"):
        y = o[:, np.clip(idx, 0, T - 1)] * w[None, None, :]
    return np.where(inside[None], y, np.float32(0)).astype(np.float32)


def autocorr64(y, lags):
    """(A, M) in float64 of y [..., Wn] float32: A[tau] = sum y[j] y[j + tau], M[tau] = sum |y[j]| |y[j + tau]|, tau < lags."""
    y = y.astype(np.float64)
    Wn = y.shape[-1]
    A, M = np.zeros(y.shape[:-1] + (lags,)), np.zeros(y.shape[:-1] + (lags,))
    with np.errstate(invalid="ignore", over="ignore"):
        for tau in range(lags):
            prod = y[..., :Wn - tau] * y[..., tau:]
            A[..., tau], M[..., tau] = prod.sum(axis=-1), np.abs(prod).sum(axis=-1)
    return A, M


def autocorr32(y, lags):
    """A of the float32 restatement: [..., lags] float32."""
    Wn = y.shape[-1]
    acc = np.zeros(y.shape[:-1] + (lags,), np.float32)
    finite = bool(np.isfinite(y).all())
    for j in range(Wn):
        n = min(lags, Wn - j)               # the lags tau with j + tau < Wn
        if finite and not y[..., j].any() and not (np.signbit(acc) & (acc == 0)).any():
            continue                        # fmaf(+-0, finite, acc) == acc unless acc is -0
        acc[..., :n] = fma32(y[..., j:j + 1], y[..., j:j + n], acc[..., :n])
    return acc


def normalised(A):
    """A / A[0] in the type of A, +0 where A[0] == 0."""
    a0 = A[..., :1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return np.where(a0 == 0, np.zeros((), A.dtype), A / np.where(a0 == 0, np.ones((), A.dtype), a0))


def sums(o, w, lags, hop, n_frames, restate=True):
    """(Wn, A64, M, A32 or None) of every frame: what both normalise values share."""
    y = windowed(o, w, hop, n_frames)
    A, M = autocorr64(y, lags)
    return y.shape[-1], A, M, autocorr32(y, lags) if restate else None


def tempogram(o, w, lags, hop, n_frames, normalise, restate=True, shared=None):
    """dict: tg64 [R][n_frames][lags], cap of the same shape, and with restate tg32 (float32).  shared: sums() of the same arguments."""
    Wn, A, M, A32 = shared if shared is not None else sums(o, w, lags, hop, n_frames, restate)
    tau = np.arange(lags, dtype=np.float64)
    out = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if normalise:
            out["tg64"] = normalised(A)
            a0 = A[..., :1]
            out["cap"] = np.where(a0 == 0, 0.0, ((Wn - tau + 4) * M / np.where(a0 == 0, 1.0, a0) + (Wn + 8) * np.abs(out["tg64"])) * U)
        else:
            out["tg64"] = A
            out["cap"] = (Wn - tau + 4) * U * M
    if A32 is not None:
        out["tg32"] = normalised(A32) if normalise else A32
    return out


def cap_units(tg, ref):
    """max over a row's elements of |tg - tg64| in units of the cap: [R] (elements whose reference is not finite are left out)."""
    ok = np.isfinite(ref["tg64"]) & np.isfinite(ref["cap"])
    err = np.where(ok, np.abs(tg.astype(np.float64) - np.where(ok, ref["tg64"], 0.0)), 0.0)
    cap = np.where(ok, ref["cap"], 1.0)
    q = np.where(cap > 0, err / np.where(cap > 0, cap, 1.0), np.where(err > 0, np.inf, 0.0))
    return q.reshape(q.shape[0], -1).max(axis=1)


# ---------------------------------------------------------------------------------------------------- tempo
def prior64(lags, frame_rate=FRAME_RATE, start_bpm=120.0, std_bpm=1.0, max_bpm=320.0):
    out = np.zeros(lags)
    tau = np.arange(1, lags, dtype=np.float64)
    bpm = 60.0 * frame_rate / tau
    out[1:] = np.exp(-0.5 * ((np.log2(bpm) - np.log2(start_bpm)) / std_bpm) ** 2)
    if max_bpm > 0:
        out[1:][bpm > max_bpm] = 0.0
    return out


def tempo64(tg, prior, frame_rate=FRAME_RATE):
    """tg [N][lags] (any float type) -> (lag, bpm, best / runner-up, g) in float64."""
    g = np.asarray(tg, np.float64).mean(axis=0)
    s = (1.0 + 1e6 * g[1:]) * np.asarray(prior, np.float64)[1:]
    best = int(np.argmax(s))
    rest = np.delete(s, best)
    margin = s[best] / rest.max() if rest.size and rest.max() > 0 else np.inf
    return best + 1, 60.0 * frame_rate / (best + 1), margin, g


def tempo32(tg, prior, frame_rate=FRAME_RATE):
    """The float32 restatement on tg [N][lags] float32, prior [lags] float32: (lag int, bpm float32, g [lags] float32); lag -1 and bpm
    NaN where a g[tau], tau >= 1, is NaN."""
    tg, prior = np.asarray(tg, np.float32), np.asarray(prior, np.float32)
    N, lags = tg.shape
    total = np.zeros(lags, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, N, 64):
            P = np.zeros(lags, np.float32)
            for i in range(i0, min(N, i0 + 64)):
                P = P + tg[i]
            total = total + P
        g = total / np.float32(N)
        s = fma32(np.full(lags, 1e6, np.float32), g, np.float32(1.0)) * prior
    if np.isnan(g[1:]).any():
        return -1, np.float32(np.nan), g
    best, best_tau = -np.inf, None
    for tau in range(1, lags):
        if s[tau] > best or (best_tau is None and s[tau] == best):
            best, best_tau = s[tau], tau
    tau = 1 if best_tau is None else best_tau
    return tau, np.float32(np.float32(60.0) * np.float32(frame_rate)) / np.float32(tau), g


# ---------------------------------------------------------------------------------------------------- shared signals
def hann(n):
    """The periodic Hann window in float32 (what the library's own table holds, up to its rounding)."""
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def impulse_train(T, period, floor=0.01):
    o = np.full(T, floor, np.float32)
    o[::period] = 1.0
    return o


@functools.lru_cache(maxsize=None)
def envelopes(n=600):
    """[5][n] float32: an impulse train of period 20, noise, a decaying pulse train of period 30 on noise, silence, a ramp with steps.
    Read-only."""
    rng = np.random.default_rng(20261019)
    x = np.zeros((5, n), np.float64)
    x[0] = impulse_train(n, 20)
    x[1] = np.abs(rng.standard_normal(n))
    x[2] = 0.1 * np.abs(rng.standard_normal(n))
    for k in range(0, n, 30):
        x[2, k:k + 4] += np.array([1.0, 0.5, 0.25, 0.125])[:max(0, min(4, n - k))]
    x[4] = (np.arange(n) % 47) / 47.0 + (np.arange(n) // 150) * 0.5
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def planes(T=40, B=200):
    """[3][T][B] float32 dB-like planes: noise, noise with onsets every 7 frames, a slowly rising plane.  Read-only."""
    rng = np.random.default_rng(7)
    S = np.zeros((3, T, B), np.float64)
    S[0] = -40.0 + 10.0 * rng.standard_normal((T, B))
    S[1] = -50.0 + 3.0 * rng.standard_normal((T, B))
    S[1, ::7] += 25.0
    S[2] = -30.0 + 0.5 * np.arange(T)[:, None] + rng.standard_normal((T, B))
    S = S.astype(np.float32)
    S.setflags(write=False)
    return S
