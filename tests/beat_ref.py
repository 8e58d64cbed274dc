"""Beat tracking by dynamic programming (include/jsgx.h section 1): the float32 restatement in the library's stated orders, a plain
float64 version for known answers, the exp routine against exp in double, the shared signals.  numpy only; tests/test_beat_ref.py checks
this module on the CPU, tests/test_gpu_beat.py compares the GPU against it bit for bit.

The restatement: the lane sums of 256 lanes with a halving tree, the smoothing as acc = fmaf(g[|k|], s0[t + k], acc) for k ascending,
jsgx_exp operation by operation, the recurrence with the lowest tau on ties.  The float32 fmaf is emulated exactly as in
tests/rhythm_ref.py: the product is exact in float64, the sum with the accumulator is rounded to odd in float64 (TwoSum gives the sign of
what was lost) and then to nearest in float32.
"""
import functools

import numpy as np

MAX_PERIOD = 1024
LANES = 256
EXP_REL_BOUND = 1.0e-7        # JSGX_EXP_REL_BOUND of include/jsgx.h
F32 = np.float32


def fma32(a, b, acc):
    """float32 fmaf(a, b, acc), exactly (no overflow or underflow of the product in float64: float32 inputs)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)            # 48 bits: exact
        c = np.broadcast_to(acc, p.shape).astype(np.float64)
        s = c + p
        t = s - c
        lost = (c - (s - t)) + (p - t)           # TwoSum: c + p = s + lost exactly
        fix = (lost != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)), s)      # round to odd
        return s.astype(F32)


def log_table(n=2 * MAX_PERIOD + 1):
    out = np.zeros(n, F32)
    out[1:] = np.log(np.arange(1, n, dtype=np.float64)).astype(F32)
    return out


def form(P):
    """(a, G, F) of include/jsgx.h, "The kernel"."""
    a = (P + 1) // 2
    G = 1
    while G < 64 and LANES // G > a:
        G *= 2
    return a, G, min(LANES // G, a)


# The periods of the GPU test over the kernel's forms (tests/test_gpu_beat.py): every (G, F) and plan name that a period in 1..1024 gives, and
# both periods wherever one of them changes (3, 5, 7, 15, 31, 63, 127, 255, 511); 1, 16, 33, 64, 100, 200, 257 and 1024 lie inside a form.
# tests/test_jsgx_forms_host.py derives the forms from form() and jsgx_beat_plan and fails where this list misses one.
FORM_PERIODS = (1, 2, 3, 4, 5, 6, 7, 14, 15, 16, 30, 31, 33, 62, 63, 64, 100, 126, 127, 200, 254, 255, 257, 510, 511, 1024)


# ---------------------------------------------------------------------------------------------------- jsgx_exp
def exp32(x):
    """jsgx_exp of an array of float32 x <= 0, operation by operation."""
    x = np.asarray(x, F32)
    n = np.floor(fma32(x, F(1.44269502162933349609375), F(0.5)))
    r = fma32(n, F(-0.693145751953125), x)
    r = fma32(n, F(-1.42860676533018704503775e-06), r)
    p = np.full(x.shape, 1.984127011382952332496643e-04, F32)
    for c in (1.388888922519981861114502e-03, 8.333333767950534820556641e-03, 4.166666790843009948730469e-02, 1.666666716337203979492188e-01,
              0.5, 1.0, 1.0):
        p = fma32(p, r, F(c))
    scale = ((np.clip(n, -126, 0).astype(np.int32) + 127) << 23).astype(np.uint32).view(F32)
    return np.where(x < F(-87.0), F(0), p * scale).astype(F32)


def F(v):
    return np.float32(v)


def gauss_arg(P):
    """x of k = 0..P: -0.5f * fl(z * z), z = fl(fl(32 k) / P)."""
    k = np.arange(P + 1, dtype=F32)
    z = (F(32.0) * k) / F(P)
    return F(-0.5) * (z * z)


def gauss32(P):
    return exp32(gauss_arg(P))


@functools.lru_cache(maxsize=None)
def exp_accuracy():
    """(worst relative error of jsgx_exp against exp in double over every (P, k), P <= 1024, with x >= -87; the number of such points; the
    largest exp(x) among the points below -87; their number)."""
    worst, count, below, n_below = 0.0, 0, 0.0, 0
    for P in range(1, MAX_PERIOD + 1):
        x = gauss_arg(P)
        g = exp32(x).astype(np.float64)
        want = np.exp(x.astype(np.float64))
        inside = x >= F(-87.0)
        worst = max(worst, float(np.max(np.abs(g[inside] - want[inside]) / want[inside])))
        count += int(inside.sum())
        if (~inside).any():
            assert (g[~inside] == 0).all()
            below = max(below, float(want[~inside].max()))
            n_below += int((~inside).sum())
    return worst, count, below, n_below


# ---------------------------------------------------------------------------------------------------- the float32 restatement
def lane_sum(v):
    """The lane sum of include/jsgx.h: 256 lanes with a stride, then a halving tree."""
    v = np.asarray(v, F32)
    acc = np.zeros(LANES, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, v.size, LANES):
            n = min(LANES, v.size - t0)
            acc[:n] = acc[:n] + v[t0:t0 + n]
        h = LANES // 2
        while h >= 1:
            acc = acc[:h] + acc[h:2 * h]
            h //= 2
    return acc[0]


def local_score32(o, P, smooth, normalise):
    """s of one row [T] or of rows [R][T] that share P."""
    o = np.asarray(o, F32)
    if o.ndim == 2:
        return np.stack([local_score32(row, P, smooth, normalise) for row in o]) if not smooth else _smooth32(np.stack([_scaled32(row, normalise) for row in o]), P)
    s0 = _scaled32(o, normalise)
    return _smooth32(s0[None], P)[0] if smooth else s0.copy()


def _scaled32(o, normalise):
    T = o.size
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if normalise and T > 1:
            mean = lane_sum(o) / F(T)
            d = o - mean
            sd = np.sqrt(lane_sum(d * d) / F(T - 1))
            if sd != 0:
                return (o / sd).astype(F32)
    return o


def _smooth32(s0, P):
    """[R][T] -> [R][T]: acc = fmaf(g[|k|], s0[t + k], acc) for k ascending."""
    T = s0.shape[1]
    g = gauss32(P)
    acc = np.zeros(s0.shape, F32)
    finite = bool(np.isfinite(s0).all())
    for k in range(-P, P + 1):
        lo, hi = max(0, -k), min(T, T - k)          # the t with 0 <= t + k < T
        if lo >= hi:
            continue
        if g[abs(k)] == 0 and finite and not (np.signbit(acc) & (acc == 0)).any():
            continue                                # fmaf(+0, finite, acc) == acc unless acc is -0
        acc[:, lo:hi] = fma32(g[abs(k)], s0[:, lo + k:hi + k], acc[:, lo:hi])
    return acc


def penalty32(P, tightness, L=None):
    """pen[tau - a], tau = a..2P."""
    L = log_table() if L is None else L
    a = (P + 1) // 2
    d = L[a:2 * P + 1] - L[P]
    return -((F(tightness) * d) * d)


def dp32(s, P, pen):
    """(C float32, link int32) of the recurrence and the first-beat rule on the local score s: one row [T] or rows [R][T]."""
    if s.ndim == 1:
        C, link = dp32(s[None], P, pen)
        return C[0], link[0]
    R, T = s.shape
    a = (P + 1) // 2
    n = 2 * P + 1 - a
    pad = 2 * P
    C = np.zeros((R, pad + T), F32)           # C[u] at C[pad + u]; +0 for u < 0
    link = np.empty((R, T), np.int32)
    rev = pen[::-1].copy()                    # rev[i] pairs with u = t - 2P + i, i.e. tau = 2P - i
    rows = np.arange(R)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            v = rev[None] + C[:, t:t + n]     # u = t - 2P .. t - a
            m = v.max(axis=1)
            i = n - 1 - np.argmax(v[:, ::-1] == m[:, None], axis=1)       # the highest i of the maximum: the lowest tau
            C[:, pad + t] = s[:, t] + v[rows, i]
            back = t - (2 * P - i)
            link[:, t] = np.where(back >= 0, back, -1)
        th = F(0.01) * s.max(axis=1)
    for r in range(R):
        hit = np.nonzero(s[r] >= th[r])[0]
        link[r, :int(hit[0]) if hit.size else T] = -1
    return C[:, pad:].copy(), link


def backtrace(C, link, P):
    T = C.size
    e0 = max(0, T - P)
    e = e0 + int(np.argmax(C[e0:]))           # the first of the maximum
    chain = []
    while e >= 0:
        chain.append(e)
        e = int(link[e])
    return np.array(chain[::-1], np.int32)


def beat32_rows(o, P, tightness=100.0, smooth=True, normalise=True, L=None):
    """Rows [R][T] (no NaN) that share a good P: a list of dict(n, beats, s, C)."""
    o = np.asarray(o, F32)
    s = local_score32(o, P, smooth, normalise)
    C, link = dp32(s, P, penalty32(P, tightness, L))
    out = []
    for r in range(o.shape[0]):
        beats = backtrace(C[r], link[r], P)
        out.append({"n": beats.size, "beats": beats, "s": s[r], "C": C[r]})
    return out


def beat32(o, P, tightness=100.0, smooth=True, normalise=True, L=None):
    """One row: dict(n, beats, s, C), or dict(n=-1) for a bad period or a NaN."""
    o = np.asarray(o, F32)
    if P < 1 or P > MAX_PERIOD or np.isnan(o).any():
        return {"n": -1}
    s = local_score32(o, P, smooth, normalise)
    C, link = dp32(s, P, penalty32(P, tightness, L))
    beats = backtrace(C, link, P)
    return {"n": beats.size, "beats": beats, "s": s, "C": C}


# ---------------------------------------------------------------------------------------------------- plain float64
def beat64(o, P, tightness=100.0, smooth=True, normalise=True):
    """The definition in float64 with numpy's own sums: beats (ascending)."""
    o = np.asarray(o, np.float64)
    T = o.size
    s = o
    if normalise and T > 1 and o.std(ddof=1) != 0:
        s = o / o.std(ddof=1)
    if smooth:
        k = np.arange(-P, P + 1)
        g = np.exp(-0.5 * (k * 32.0 / P) ** 2)
        s = np.convolve(s, g, "same") if T >= g.size else np.convolve(g, s, "full")[P:P + T]
    a = (P + 1) // 2
    taus = np.arange(a, 2 * P + 1)
    pen = -tightness * np.log(taus / P) ** 2
    C = np.zeros(T)
    link = np.full(T, -1)
    th = 0.01 * s.max()
    started = False
    for t in range(T):
        prev = np.where(t - taus >= 0, C[np.maximum(t - taus, 0)], 0.0)
        v = pen + prev
        i = int(np.argmax(v))
        C[t] = s[t] + v[i]
        started = started or s[t] >= th
        if started and t - taus[i] >= 0:
            link[t] = t - taus[i]
    return backtrace(C, link, P)


# ---------------------------------------------------------------------------------------------------- shared signals
def impulse_train(T, period, start=0, missing=()):
    o = np.zeros(T, F32)
    o[start::period] = 1.0
    for m in missing:
        o[start + m * period] = 0.0
    return o


@functools.lru_cache(maxsize=None)
def envelope(kind, T, P):
    """A read-only float32 row: "zero", "const", "random" (seeded by T and P), "train" (impulses every P from P // 3 on a small floor)."""
    if kind == "zero":
        o = np.zeros(T, F32)
    elif kind == "const":
        o = np.full(T, 0.75, F32)
    elif kind == "random":
        o = np.abs(np.random.default_rng(1000003 * T + P).standard_normal(T)).astype(F32)
    else:
        o = np.full(T, 0.0625, F32)
        o[P // 3::P] = 1.0
    o.setflags(write=False)
    return o
