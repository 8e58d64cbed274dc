"""YIN fundamental-frequency tracking (include/jsg.h section 2i): the definition evaluated in float64, the float32 restatement in the
library's stated orders, the per-element cap on d', whether a frame's lag is decided, the shared signals.  numpy only;
tests/test_yin_ref.py checks this module on the CPU, tests/test_gpu_yin.py compares the GPU against it.

The restatement: one accumulator per lag, j walked as j = jb + j0 + 64 jj (jb = 0, 512, ...; j0 = 0..63; jj = 0..7; j < w) with
e = x[j] - x[j + tau], acc = fmaf(e, e, acc); the running sum in groups of 64 lags (a Hillis-Steele scan with the offsets 1, 2, ..., 32
and a carry from group to group); d' = (d * float(tau)) / S.  The float32 fmaf is emulated exactly: e * e is exact in float64, the sum
with the accumulator is rounded to odd in float64 (TwoSum gives the sign of what was lost) and then to nearest in float32.
"""
import functools

import numpy as np

# bound (a) of tests/test_gpu_yin.py: GPU error <= YARDSTICKS x the restatement's error on the same signal.  4 before any GPU run;
# afterwards 1.25 x the worst ratio measured by tools/yin_accuracy.py, rounded up to the next half (the rule of
# profiles/stft_power_accuracy.md).  Measured on an MI355X: the worst ratio over the cases of tools/yin_accuracy.py is 1.000 (the GPU's
# bits equal the restatement's in every d'; profiles/yin_accuracy.md), so 1.25 x 1.000 rounded up to the next half.
YARDSTICKS = 1.5

SR, L, W, TAU_MIN, TAU_MAX, HOP, THRESHOLD = 8000.0, 3000, 256, 8, 200, 64, 0.1
NAMES = ("tone", "harmonic", "noise", "pulses", "silence", "onset")
MOSTLY_DECIDED = ("tone", "harmonic", "noise", "pulses")        # at most 10 % of their frames may be undecided
PULSE_PERIOD = 73
U = 2.0 ** -24


def frames(n, w, tau_max, hop):
    return 1 + (n - w - tau_max) // hop if n >= w + tau_max else 0


@functools.lru_cache(maxsize=None)
def signals(n=L):
    """[6][n] float32 in the order of NAMES.  Read-only."""
    rng = np.random.default_rng(20261019)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((6, n), np.float64)
    x[0] = 0.5 * np.sin(2 * np.pi * 220.0 / SR * t)
    phase = 2 * np.pi * np.cumsum(110.0 * (1.0 + 0.2 * t / n)) / SR         # a fundamental gliding from 110 Hz to 132 Hz
    x[1] = 0.5 * np.sin(phase) + 0.3 * np.sin(2 * phase) + 0.2 * np.sin(3 * phase) + 0.02 * rng.standard_normal(n)
    x[2] = 0.3 * rng.standard_normal(n)
    x[3, ::PULSE_PERIOD] = 1.0
    x[5, 1500:] = 0.5 * np.sin(2 * np.pi * 330.0 / SR * t[:n - 1500])
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def order(w):
    """The j of the sum of d in the order they are added."""
    out = []
    for jb in range(0, w, 512):
        for j0 in range(64):
            for jj in range(8):
                j = jb + j0 + 64 * jj
                if j < w:
                    out.append(j)
    return out


def fma_square(e, acc):
    """float32 fmaf(e, e, acc), exactly."""
    p = e.astype(np.float64) ** 2            # 48 bits: exact
    a = acc.astype(np.float64)
    s = a + p
    b = s - a
    lost = (a - (s - b)) + (p - b)           # TwoSum: a + p = s + lost exactly
    fix = (lost != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)), s)      # round to odd
    return s.astype(np.float32)


def framed(x, w, tau_max, hop, T):
    """[R][T][w + tau_max] view of x [R][n]."""
    x = np.ascontiguousarray(x)
    R = x.shape[0]
    return np.lib.stride_tricks.as_strided(x, (R, T, w + tau_max), (x.strides[0], hop * x.strides[1], x.strides[1]), writeable=False)


def cmnd64(X, w, tau_max):
    """d' in float64 of frames X [..., w + tau_max] float32: [..., tau_max + 1]."""
    X = X.astype(np.float64)
    d = np.zeros(X.shape[:-1] + (tau_max + 1,))
    for tau in range(1, tau_max + 1):
        e = X[..., :w] - X[..., tau:tau + w]
        d[..., tau] = (e * e).sum(axis=-1)
    S = np.cumsum(d, axis=-1)
    tau = np.arange(tau_max + 1, dtype=np.float64)
    out = np.where(S == 0, 1.0, d * tau / np.where(S == 0, 1.0, S))
    out[..., 0] = 1.0
    return out


def cmnd32(X, w, tau_max):
    """d' of the float32 restatement: [..., tau_max + 1] float32."""
    acc = np.zeros(X.shape[:-1] + (tau_max,), np.float32)
    for j in order(w):
        e = X[..., j:j + 1] - X[..., j + 1:j + 1 + tau_max]
        acc = fma_square(e, acc)
    groups = -(-tau_max // 64)
    v = np.zeros(X.shape[:-1] + (groups * 64,), np.float32)
    v[..., :tau_max] = acc
    v = v.reshape(X.shape[:-1] + (groups, 64))
    for s in (1, 2, 4, 8, 16, 32):
        v = np.concatenate([v[..., :s], v[..., s:] + v[..., :-s]], axis=-1)
    S = np.zeros_like(v)
    carry = np.zeros(X.shape[:-1], np.float32)
    for c in range(groups):
        S[..., c, :] = carry[..., None] + v[..., c, :]
        carry = S[..., c, 63]
    S = S.reshape(X.shape[:-1] + (groups * 64,))[..., :tau_max]
    tau = np.arange(1, tau_max + 1, dtype=np.float32)
    out = np.ones(X.shape[:-1] + (tau_max + 1,), np.float32)
    out[..., 1:] = np.where(S == 0, np.float32(1), (acc * tau) / np.where(S == 0, np.float32(1), S))
    return out


def select(dp, tau_min, tau_max, threshold, sr):
    """Steps 3 to 6 on one frame's d' (float32 or float64; the arithmetic is done in its type): (tau, s, f0, aper).  threshold and sr
    are taken at their float32 values."""
    ft = dp.dtype.type
    thr, rate = ft(np.float32(threshold)), ft(np.float32(sr))
    seg = dp[tau_min:tau_max + 1]
    below = np.flatnonzero(seg < thr)
    if below.size:
        tau = tau_min + int(below[0])
        while tau + 1 <= tau_max and dp[tau + 1] < dp[tau]:
            tau += 1
    else:
        finite = np.where(np.isnan(seg), np.inf, seg)
        tau = tau_min + int(np.argmin(finite))          # the lowest lag on ties
    s = ft(0)
    if tau + 1 <= tau_max:
        a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
        den = (a - b) + (c - b)
        if den > 0:
            s = (ft(0.5) * (a - c)) / den
            if not abs(s) <= 1:
                s = ft(0)
    if np.isnan(seg).any():
        return tau, s, ft(np.nan), ft(np.nan)
    return tau, s, rate / (ft(tau) + s), dp[tau]


def cap(dp64, w):
    """Cap (b) on |d' - d'64| per element: (2 w + tau + 12) 2^-24 d'64[tau] (every term of d and of S is non-negative: d carries at
    most (w + 4) u, S at most (w + tau + 4) u, then the product, the divide and the conversion)."""
    tau = np.arange(dp64.shape[-1], dtype=np.float64)
    return (2 * w + tau + 12) * U * dp64


def decided(dp64, caps, tau_min, tau_max, threshold):
    """Whether no change of every d'[tau] within its cap moves the lag select() picks (a sufficient test on the intervals)."""
    if np.isnan(dp64[tau_min:tau_max + 1]).any():
        return False
    thr = np.float64(np.float32(threshold))
    lo, hi = dp64 - caps, dp64 + caps
    rng = np.arange(tau_min, tau_max + 1)
    below = rng[dp64[rng] < thr]
    if below.size:
        first = int(below[0])
        if not (lo[tau_min:first] >= thr).all() or not hi[first] < thr:
            return False
        tau = first
        while tau + 1 <= tau_max and dp64[tau + 1] < dp64[tau]:
            if not hi[tau + 1] < lo[tau]:
                return False
            tau += 1
        return tau + 1 > tau_max or bool(lo[tau + 1] >= hi[tau])
    if not (lo[rng] >= thr).all():
        return False
    m = tau_min + int(np.argmin(dp64[rng]))
    others = rng[rng != m]
    return bool((hi[m] < lo[others]).all())


def evaluate(x, w, tau_min, tau_max, hop, T, threshold, sr, restate=True):
    """x [R][n] float32 -> dict: dp64 [R][T][tau_max + 1], cap (b) of the same shape, tau64, f064, aper64, decided [R][T]; with restate
    also dp32, tau32, f032, aper32 of the float32 restatement."""
    x = np.atleast_2d(x)
    R = x.shape[0]
    X = framed(x, w, tau_max, hop, T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        out = dict(dp64=cmnd64(X, w, tau_max))
        out["cap"] = cap(out["dp64"], w)
        kinds = [("64", out["dp64"])]
        if restate:
            out["dp32"] = cmnd32(X, w, tau_max)
            kinds.append(("32", out["dp32"]))
        for tag, dp in kinds:
            tau, f0, ap = np.zeros((R, T), np.int64), np.zeros((R, T), dp.dtype), np.zeros((R, T), dp.dtype)
            for r in range(R):
                for t in range(T):
                    tau[r, t], _, f0[r, t], ap[r, t] = select(dp[r, t], tau_min, tau_max, threshold, sr)
            out["tau" + tag], out["f0" + tag], out["aper" + tag] = tau, f0, ap
        out["decided"] = np.array([[decided(out["dp64"][r, t], out["cap"][r, t], tau_min, tau_max, threshold) for t in range(T)] for r in range(R)])
    return out


def implied_lag(f0, aper, dp, sr, tau_min, tau_max):
    """The lag behind one frame's outputs: the tau in tau_min..tau_max with d'[tau] == aper that lies nearest to sr / f0 (f0 is
    sr / (tau + s) with |s| <= 1), or -1 where there is none within 1.001 of it."""
    hits = tau_min + np.flatnonzero(dp[tau_min:tau_max + 1] == aper)
    if not hits.size or not np.isfinite(f0) or f0 <= 0:
        return -1
    period = float(np.float32(sr)) / float(f0)
    tau = int(hits[np.argmin(np.abs(hits - period))])
    return tau if abs(tau - period) <= 1.001 else -1


@functools.lru_cache(maxsize=None)
def shared():
    """evaluate() of the shared signals, computed once.  Read-only."""
    out = evaluate(signals(), W, TAU_MIN, TAU_MAX, HOP, frames(L, W, TAU_MAX, HOP), THRESHOLD, SR)
    for v in out.values():
        v.setflags(write=False)
    return out


def cap_units(dp, ref):
    """max over a signal's elements of |d' - d'64| in units of the cap: [R]."""
    err = np.abs(dp.astype(np.float64) - ref["dp64"])
    q = np.where(ref["cap"] > 0, err / np.where(ref["cap"] > 0, ref["cap"], 1.0), np.where(err > 0, np.inf, 0.0))
    return q.reshape(q.shape[0], -1).max(axis=1)
