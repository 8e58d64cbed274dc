"""Sections 15 and 16 of include/jsgx.h restated in float32 numpy, operation by operation: the segments of a list of boundaries, the four
aggregates over them and the time-delay embedding.  Every result is compared with the GPU's as int32 bits.  Also the shapes and the
segment lengths the GPU test runs, derived from the header's thresholds."""
import numpy as np

MEAN, MIN, MAX, MEDIAN = 0, 1, 2, 3
AGGREGATES = {"mean": MEAN, "min": MIN, "max": MAX, "median": MEDIAN}
CHUNK, WAVE_MAX, STAGE = 256, 64, 256          # JSGX_SYNC_CHUNK, JSGX_SYNC_WAVE_MAX, JSGX_SYNC_STAGE
NAN_BITS = 0x7FC00000
CONSTANT, EDGE = 0, 1

# what the GPU test runs
N_SET = (1, 63, 64, 65, 257, 1025)
F_SET = (1, 63, 64, 65, 130)
THRESHOLDS = tuple(sorted({CHUNK, WAVE_MAX, STAGE}))
# every listed length, and one each side of every threshold between two forms of the kernel
LENGTHS = tuple(sorted({1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 512, 513} | {t + d for t in THRESHOLDS for d in (0, 1)}))
WHOLE = 1025          # one segment that is the whole of N = 1025


def key(v):
    """HPSS's hp_key on float32 values: uint32 whose order is the order of the floats, -0 below +0."""
    b = np.asarray(v, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def segments(bounds, n_bounds, n_frames, pad, max_bounds=None):
    """(n_segments, u) of one pair: n_segments is -1 for a refused pair (u None), else the whole count and u the frames u[0] < ... < u[U-1]
    (empty where U < 2: nothing is written then)."""
    max_bounds = len(bounds) if max_bounds is None else max_bounds
    if n_bounds < 0:
        return -1, None
    m = min(int(n_bounds), int(max_bounds))
    b = np.asarray(bounds[:m], np.int64)
    if (b[1:] < b[:-1]).any():
        return -1, None
    c = np.minimum(np.maximum(b, 0), n_frames)
    s = list(c)
    if pad:
        s = [0] + s + [n_frames]
    u = [v for i, v in enumerate(s) if i == 0 or v != s[i - 1]]
    if len(u) < 2:
        return 0, np.zeros(0, np.int32)
    return len(u) - 1, np.asarray(u, np.int32)


def mean_chunked(X):
    """X float32 [cnt][F] -> [F]: partial chains over chunks of CHUNK frames, the chain of the partials, one correctly rounded divide."""
    X = np.asarray(X, np.float32)
    cnt, F = X.shape
    tot = np.zeros(F, np.float32)
    for a in range(0, cnt, CHUNK):
        part = np.zeros(F, np.float32)
        for t in range(a, min(a + CHUNK, cnt)):
            part = part + X[t]
        tot = tot + part
    with np.errstate(all="ignore"):
        return tot / np.float32(cnt)


def mean_single_chain(X):
    """The order the contract does NOT use: one ascending chain over the whole segment."""
    X = np.asarray(X, np.float32)
    acc = np.zeros(X.shape[1], np.float32)
    for t in range(X.shape[0]):
        acc = acc + X[t]
    return acc / np.float32(X.shape[0])


def aggregate(X, agg):
    """One segment X float32 [cnt][F] -> uint32 bits [F]."""
    X = np.asarray(X, np.float32)
    cnt = X.shape[0]
    nan = np.isnan(X).any(axis=0)
    with np.errstate(all="ignore"):
        if agg == MEAN:
            out = mean_chunked(X)
            nan = np.isnan(out)
        elif agg == MIN:
            out = unkey(key(X).min(axis=0))
        elif agg == MAX:
            out = unkey(key(X).max(axis=0))
        else:
            v = unkey(np.sort(key(X), axis=0))
            out = v[(cnt - 1) // 2] if cnt % 2 else np.float32(0.5) * (v[cnt // 2 - 1] + v[cnt // 2])
            nan = nan | np.isnan(out)          # -inf + inf
    bits = np.array(out, np.float32).view(np.uint32).copy()
    bits[nan] = NAN_BITS
    return bits


def sync(X, bounds, n_bounds, agg, pad, max_segments, max_bounds=None):
    """One pair: X float32 [N][F] -> (n_segments, u as written (at most max_segments + 1 entries), out bits uint32 [rows written][F])."""
    X = np.asarray(X, np.float32)
    n, u = segments(bounds, n_bounds, X.shape[0], pad, max_bounds)
    if n <= 0:
        return n, np.zeros(0, np.int32), np.zeros((0, X.shape[1]), np.uint32)
    rows = min(n, max_segments)
    out = np.stack([aggregate(X[u[o]:u[o + 1]], agg) for o in range(rows)])
    return n, u[:rows + 1], out


def stack_memory(X, n_steps, delay, mode, fill_bits=0):
    """X [N][F] (any 32-bit dtype, taken as bits) -> uint32 [N][n_steps * F]."""
    B = np.ascontiguousarray(X).view(np.uint32)
    N, F = B.shape
    out = np.empty((N, n_steps * F), np.uint32)
    t = np.arange(N, dtype=np.int64)
    for s in range(n_steps):
        src = t - s * delay
        inside = (src >= 0) & (src < N)
        rows = B[np.clip(src, 0, N - 1)]
        if mode == CONSTANT:
            rows = np.where(inside[:, None], rows, np.uint32(fill_bits))
        out[:, s * F:(s + 1) * F] = rows
    return out


def bounds_of_lengths(lengths):
    """Boundaries (without 0 and the end) and N of a plane cut into segments of these lengths."""
    edges = np.cumsum(np.asarray(lengths, np.int64))
    return edges[:-1].astype(np.int32), int(edges[-1])
