"""Restatement of include/jsgx.h sections 10 and 11 in numpy: path enhancement of a plane by a tap list, one vectorised float32 fmaf per
tap over the plane (rhythm_ref.fma32), and the time-lag conversions.  Also the float64 scipy route the definition is measured against,
and the test planes."""
import numpy as np

from rhythm_ref import fma32


def unpack(tap_at):
    """(di, dj) of the packed offsets: two signed 16-bit halves, di high."""
    at = np.asarray(tap_at, dtype=np.int32)
    return (at >> 16).astype(np.int64), (at & 0xffff).astype(np.uint16).view(np.int16).astype(np.int64)


def pack(di, dj):
    return ((np.asarray(di, np.int64) << 16) | (np.asarray(dj, np.int64) & 0xffff)).astype(np.uint32).view(np.int32)


def taps_of_table(K, filter_first=None):
    """The tap list of a dense table, as the builder emits it: the non-zero entries in row-major order, di = h // 2 - a, dj = w // 2 - b,
    float32 weights."""
    K = np.asarray(K)
    h, w = K.shape
    a, b = np.nonzero(K)
    return K[a, b].astype(np.float32), pack(h // 2 - a, w // 2 - b)


def path_enhance32(R, tap_w, tap_at, filter_first, reach_i, reach_j, clip=True):
    """out [N][M] float32 of the definition: per filter the chain acc = fmaf(w_t, Rz[i + di][j + dj], acc) from +0 in list order (a tap
    beyond the reach is skipped, filter_first clamped into 0..n_taps), np.maximum across the filters in ascending order, the clip."""
    R = np.asarray(R, dtype=np.float32)
    N, M = R.shape
    di, dj = unpack(tap_at)
    w = np.asarray(tap_w, dtype=np.float32)
    T = len(w)
    first = np.clip(np.asarray(filter_first, dtype=np.int64), 0, T)
    ri, rj = int(reach_i), int(reach_j)
    Rz = np.zeros((N + 2 * ri, M + 2 * rj), np.float32)
    Rz[ri:ri + N, rj:rj + M] = R
    best = None
    for f in range(len(first) - 1):
        acc = np.zeros((N, M), np.float32)
        for t in range(first[f], first[f + 1]):
            if abs(di[t]) > ri or abs(dj[t]) > rj:
                continue
            acc = fma32(np.broadcast_to(w[t], (N, M)), Rz[ri + di[t]:ri + di[t] + N, rj + dj[t]:rj + dj[t] + M], acc)
        if best is None:
            best = acc
        else:
            with np.errstate(invalid="ignore"):
                best = np.where((acc > best) | np.isnan(acc), acc, best)
    if clip:
        with np.errstate(invalid="ignore"):
            best = np.where(best < 0, np.float32(0), best)
    return best.astype(np.float32)


def tables_of_taps(tap_w, tap_at, filter_first):
    """The dense float64 tables (odd extents, centred) of a tap list, for scipy.ndimage.convolve: K[h // 2 - di][w // 2 - dj] = w."""
    di, dj = unpack(tap_at)
    w = np.asarray(tap_w, dtype=np.float64)
    out = []
    for f in range(len(filter_first) - 1):
        s = slice(int(filter_first[f]), int(filter_first[f + 1]))
        ri = int(np.abs(di[s]).max()) if s.stop > s.start else 0
        rj = int(np.abs(dj[s]).max()) if s.stop > s.start else 0
        K = np.zeros((2 * ri + 1, 2 * rj + 1))
        np.add.at(K, (ri - di[s], rj - dj[s]), w[s])
        out.append(K)
    return out


def path_enhance64(R, tap_w, tap_at, filter_first, clip=True):
    """The scipy route in float64 from the same float32 taps: ndimage.convolve(mode="constant") per filter, np.maximum, the clip."""
    import scipy.ndimage
    R64 = np.asarray(R, dtype=np.float64)
    best = None
    for K in tables_of_taps(tap_w, tap_at, filter_first):
        acc = scipy.ndimage.convolve(R64, K, mode="constant", cval=0.0)
        best = acc if best is None else np.maximum(best, acc)
    return np.clip(best, 0, None) if clip else best


def to_lag(R, pad=True, axis=1):
    """Section 11, to lag: axis 1: lag[l][j] = Rz[(l + j) mod L][j]; axis 0: lag[i][l] = Rz[i][(l + i) mod L]."""
    R = np.asarray(R)
    N = R.shape[0]
    L = 2 * N if pad else N
    if axis == 0:
        return to_lag(R.T, pad, 1).T.copy()
    Rz = np.zeros((L, N), R.dtype)
    Rz[:N] = R
    l, j = np.arange(L)[:, None], np.arange(N)[None, :]
    return Rz[(l + j) % L, j]


def from_lag(lag, axis=1):
    """Section 11, from lag: axis 1: R[i][j] = lag[(i - j) mod L][j]; axis 0: R[i][j] = lag[i][(j - i) mod L]."""
    lag = np.asarray(lag)
    if axis == 0:
        return from_lag(lag.T, 1).T.copy()
    L, N = lag.shape
    i, j = np.arange(N)[:, None], np.arange(N)[None, :]
    return lag[(i - j) % L, j]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool((na == nb).all()) and bool((a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def affinity_plane(N, M, seed):
    """An affinity-like plane: floats in [0, 1], three quarters of them zero, with broken diagonals on top."""
    rng = np.random.default_rng(1000 + seed)
    R = rng.random((N, M)).astype(np.float32) * (rng.random((N, M)) < 0.25)
    for k in range(-(N - 1), M, 7):
        d = np.arange(max(0, -k), min(N, M - k))
        keep = rng.random(d.size) < 0.7
        R[d[keep], d[keep] + k] = rng.random(int(keep.sum())).astype(np.float32)
    return R.astype(np.float32)


def integer_plane(N, M, seed):
    """Small integers 0..3, half of them zero."""
    rng = np.random.default_rng(2000 + seed)
    return (rng.integers(0, 4, (N, M)) * (rng.random((N, M)) < 0.5)).astype(np.float32)


def distinct_plane(rows, cols, seed):
    """A plane of distinct values, none of them zero, for the permutations."""
    rng = np.random.default_rng(3000 + seed)
    return (rng.permutation(rows * cols).reshape(rows, cols) + 1).astype(np.float32) * np.float32(0.5)
