"""Section 14 of include/jsgx.h restated in numpy float32: the candidates (vectorised over the frames by looping over the window offsets,
so a reach of 256 stays cheap), the greedy wait rule, the energy minima and back(), the blocked decomposition the kernels use (the
tables of 2^k-th successors inside a block, a serial carry over the blocks, the i-th pick by the bits of i), and the shapes, parameters
and inputs the peak tests share.  Every result is an integer, so the GPU must give the same ones."""
import os
import re

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = int(re.search(r"#define JSGX_PEAK_BLOCK (\d+)", open(os.path.join(ROOT, "include", "jsgx.h")).read()).group(1))
MAX_REACH, MAX_FRAMES, SHORT = 256, 1 << 24, 64
END = 0xFFFF


def normalised(x, normalise):
    x = np.asarray(x, f32)
    if not normalise:
        return x
    mn, mx = x.min(), x.max()
    rng = f32(mx - mn)
    return np.zeros(x.size, f32) if rng == 0 else ((x - mn).astype(f32) / rng).astype(f32)


def candidates(x, pre_max, post_max, pre_avg, post_avg, delta, normalise):
    """c[t] as bool [T], or None for a row with a NaN or an infinity."""
    x = np.asarray(x, f32)
    T = x.size
    if not np.isfinite(x).all():
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        y = normalised(x, normalise)
        t = np.arange(T)
        top = np.ones(T, bool)
        for d in range(-pre_max, post_max + 1):
            j = t + d
            ok = (j >= 0) & (j < T)
            top[ok] &= ~(y[j[ok]] > y[ok])
        acc = np.zeros(T, f32)
        for d in range(-pre_avg, post_avg + 1):          # j ascending for every t
            j = t + d
            ok = (j >= 0) & (j < T)
            acc[ok] = (acc[ok] + y[j[ok]]).astype(f32)
        count = np.minimum(T - 1, t + post_avg) - np.maximum(0, t - pre_avg) + 1
        avg = (acc / count.astype(f32)).astype(f32)
        thr = (avg + f32(delta)).astype(f32)
        return top & (y >= thr)


def candidates_serial(x, pre_max, post_max, pre_avg, post_avg, delta, normalise):
    """The same, frame by frame as the header writes it."""
    x = np.asarray(x, f32)
    T = x.size
    if not np.isfinite(x).all():
        return None
    y = normalised(x, normalise)
    c = np.zeros(T, bool)
    for t in range(T):
        lo, hi = max(0, t - pre_max), min(T - 1, t + post_max)
        if not all(y[t] >= y[j] for j in range(lo, hi + 1)):
            continue
        lo, hi = max(0, t - pre_avg), min(T - 1, t + post_avg)
        acc = f32(0)
        for j in range(lo, hi + 1):
            acc = f32(acc + y[j])
        avg = f32(acc / f32(hi - lo + 1))
        c[t] = y[t] >= f32(avg + f32(delta))
    return c


def greedy(c, wait):
    out, e = [], 0
    for t in np.flatnonzero(c):
        if t >= e:
            out.append(int(t))
            e = t + wait + 1
    return out


def minima(e):
    e = np.asarray(e, f32)
    T = e.size
    m = np.zeros(T, bool)
    m[0] = True
    if T > 2:
        m[1:-1] = (e[1:-1] <= e[:-2]) & (e[1:-1] < e[2:])
    return m


def back(peaks, e):
    m = np.flatnonzero(minima(e))
    return [int(m[np.searchsorted(m, p, side="right") - 1]) for p in peaks]


def back_serial(peaks, e):
    e = np.asarray(e, f32)
    T = e.size
    out = []
    for p in peaks:
        t = p
        while not (t == 0 or (t < T - 1 and e[t] <= e[t - 1] and e[t] < e[t + 1])):
            t -= 1
        out.append(t)
    return out


def blocked(c, wait, B):
    """The wait rule as the kernels run it: per block nxt and the tables lev[k] = the pick 2^k picks on, for every entering offset the
    count and the last pick by descending the tables, a serial carry over the blocks that reads one of those per block it enters, then
    the i-th pick of a block by the bits of i."""
    T = len(c)
    nb = -(-T // B)
    L = max(1, int(B - 1).bit_length())
    offsets = min(wait + 1, B)
    words, levs, nxts = [], [], []
    for k in range(nb):
        n = min(B, T - k * B)
        nxt = np.full(B + 1, END, np.int64)
        for o in range(n - 1, -1, -1):
            nxt[o] = o if c[k * B + o] else nxt[o + 1]
        lev = np.full((L, B), END, np.int64)
        for p in range(n):
            lev[0, p] = nxt[p + wait + 1] if p + wait + 1 < n else END
        for j in range(1, L):
            for p in range(n):
                a = lev[j - 1, p]
                lev[j, p] = END if a == END else lev[j - 1, a]
        w = []
        for o in range(offsets):
            f = nxt[o] if o < n else END
            if f == END:
                w.append((0, 0))
                continue
            q, cnt = f, 0
            for j in range(L - 1, -1, -1):
                if lev[j, q] != END:
                    q, cnt = lev[j, q], cnt + (1 << j)
            w.append((cnt + 1, int(q)))
        words.append(w), levs.append(lev), nxts.append(nxt)
    enter, out = 0, []
    for k in range(nb):
        t0, end = k * B, min(k * B + B, T)
        if enter >= end:
            continue          # the wait passes the whole block: nothing of it is read
        assert enter - t0 < offsets
        count, last = words[k][enter - t0]
        f = nxts[k][enter - t0]
        for i in range(count):
            q = f
            for j in range(L):
                if (i >> j) & 1:
                    q = levs[k][j, q]
            out.append(t0 + int(q))
        if count:
            enter = t0 + last + wait + 1
        enter = max(enter, end)
    return out


def peak_pick32(x, pre_max, post_max, pre_avg, post_avg, delta, wait, normalise=False, energy=None, max_peaks=None):
    """One row: (n, peaks, backtracked or None, candidates) with the lists cut at max_peaks; (-1, None, None, None) for a refused row."""
    c = candidates(x, pre_max, post_max, pre_avg, post_avg, delta, normalise)
    if c is None or (energy is not None and not np.isfinite(np.asarray(energy, f32)).all()):
        return -1, None, None, None
    p = greedy(c, wait)
    b = None if energy is None else back(p, energy)
    cut = len(p) if max_peaks is None else min(len(p), max_peaks)
    return len(p), p[:cut], None if b is None else b[:cut], c.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ what the tests share
ROWS_SET = (1, 3)
T_SET = (1, 2, 3, 63, 64, 65, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK, 2 * BLOCK + 1, 3 * BLOCK + 7)
# crossed sparsely: every frame count and both row counts, and the four corners
SHAPES = [(ROWS_SET[i % 2], T) for i, T in enumerate(T_SET)] + [(3, T_SET[0]), (1, T_SET[-1])]
MANY_SHORT = (300, 37)
REACHES = [(0, 0, 0, 0), (1, 0, 4, 4), (3, 1, 5, 5), (256, 256, 256, 256), (0, 256, 256, 0)]
DEFAULT = dict(pre_max=3, post_max=1, pre_avg=5, post_avg=5, delta=0.07, wait=3, normalise=True)
WAITS_LONG = (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 3, MAX_FRAMES)
DELTAS = (-0.1, 0.0, 0.07)


def quantised(T, seed=0, rows=1):
    """Noise on four levels: ties abound, about a third of the frames are candidates at the reaches (3, 1, 5, 5) with delta 0.07."""
    return np.random.default_rng(seed).integers(0, 4, (rows, T)).astype(f32)


def smooth(T, seed=0, rows=1):
    """Smooth noise: about one candidate in twenty frames at the reaches (3, 1, 5, 5)."""
    w = np.random.default_rng(seed).standard_normal((rows, T + 8))
    k = np.hanning(11)[1:-1]
    return np.stack([np.convolve(r, k, "valid") for r in w]).astype(f32)


def impulses(T, every=6):
    x = np.zeros(T, f32)
    x[::every] = 1
    return x
