"""The pairwise cost and dynamic time warping (include/jsgx.h sections 2 and 3): the float32 restatement in the library's stated
operations, a cell-by-cell float32 loop, and a plain float64 DTW written independently.  numpy only; tests/test_dtw_ref.py checks this
module on the CPU, tests/test_gpu_dtw.py compares the GPU against it bit for bit.

The restatement: the cost operation by operation with k ascending (the float32 fmaf is beat_ref.fma32, exact); the recurrence vectorised
over cell anti-diagonals (the cells of one anti-diagonal depend only on the two before it), 1000 x 1000 in about a second; the backtrace
recomputing the forward choice.
"""
import numpy as np

from beat_ref import fma32

F32 = np.float32
METRICS = {"sqeuclidean": 0, "euclidean": 1, "cosine": 2}
STEPS = ((1, 1), (0, 1), (1, 0))          # (di, dj) of k = 0, 1, 2
INF = F32(np.inf)


def cost32(X, Y, metric="euclidean"):
    """c(i, j) of section 2 for X [N, K] and Y [M, K], float32 [N, M]."""
    X, Y = np.asarray(X, F32), np.asarray(Y, F32)
    N, K = X.shape
    M = Y.shape[0]
    with np.errstate(all="ignore"):
        if metric in ("sqeuclidean", "euclidean"):
            acc = np.zeros((N, M), F32)
            for k in range(K):
                d = X[:, k, None] - Y[None, :, k]
                acc = fma32(d, d, acc)
            return acc if metric == "sqeuclidean" else np.sqrt(acc)
        assert metric == "cosine"
        dot, nx, ny = np.zeros((N, M), F32), np.zeros(N, F32), np.zeros(M, F32)
        for k in range(K):
            dot = fma32(np.broadcast_to(X[:, k, None], (N, M)), np.broadcast_to(Y[None, :, k], (N, M)), dot)
            nx = fma32(X[:, k], X[:, k], nx)
            ny = fma32(Y[:, k], Y[:, k], ny)
        den = np.sqrt(nx)[:, None] * np.sqrt(ny)[None, :]
        return np.where(den == 0, F32(1.0), F32(1.0) - dot / np.where(den == 0, F32(1.0), den)).astype(F32)


def inside_band(N, M, band):
    """The cells inside the band of section 3 (all of them for band 0), exact integers."""
    if band == 0:
        return np.ones((N, M), bool)
    i, j = np.arange(N, dtype=np.int64)[:, None], np.arange(M, dtype=np.int64)[None, :]
    return np.abs(j * (N - 1) - i * (M - 1)) <= band * max(N - 1, 1)


def _weights(weights_mul, weights_add):
    wm = np.asarray((1, 1, 1) if weights_mul is None else weights_mul, F32)
    wa = np.asarray((0, 0, 0) if weights_add is None else weights_add, F32)
    return wm, wa


def dtw32(C, weights_mul=None, weights_add=None, subseq=False, band=0):
    """D of section 3, float32 [N, M], anti-diagonal by anti-diagonal."""
    C = np.asarray(C, F32)
    N, M = C.shape
    wm, wa = _weights(weights_mul, weights_add)
    inside = inside_band(N, M, band)
    with np.errstate(all="ignore"):
        e = [(wm[k] * C) + wa[k] for k in range(3)]
        P = np.full((N + 1, M + 1), INF, F32)          # P[i + 1][j + 1] = D[i][j]; row and column 0: outside the matrix
        for d in range(N + M - 1):
            i = np.arange(max(0, d - (M - 1)), min(N - 1, d) + 1)
            j = d - i
            v0, v1, v2 = P[i, j] + e[0][i, j], P[i + 1, j] + e[1][i, j], P[i, j + 1] + e[2][i, j]
            best = v0
            best = np.where(v1 < best, v1, best)
            best = np.where(v2 < best, v2, best)
            best = np.where(inside[i, j], best, INF)
            best = np.where((i == 0) & ((j == 0) | bool(subseq)), C[i, j], best)
            P[i + 1, j + 1] = best
    return P[1:, 1:].copy()


def dtw32_loop(C, weights_mul=None, weights_add=None, subseq=False, band=0):
    """The same D cell by cell with numpy float32 scalars: the text of the header, line by line."""
    C = np.asarray(C, F32)
    N, M = C.shape
    wm, wa = _weights(weights_mul, weights_add)
    D = np.empty((N, M), F32)
    get = lambda i, j: D[i, j] if i >= 0 and j >= 0 else INF
    with np.errstate(all="ignore"):
        for i in range(N):
            for j in range(M):
                if i == 0 and (j == 0 or subseq):
                    D[i, j] = C[i, j]
                elif band and abs(j * (N - 1) - i * (M - 1)) > band * max(N - 1, 1):
                    D[i, j] = INF
                else:
                    best = None
                    for k, (di, dj) in enumerate(STEPS):
                        v = F32(get(i - di, j - dj) + F32(F32(wm[k] * C[i, j]) + wa[k]))
                        if best is None or v < best:
                            best = v
                    D[i, j] = best
    return D


def backtrace32(D, C, weights_mul=None, weights_add=None, subseq=False):
    """(path int32 [L, 2] ascending or None where there is none, total or None) of section 3 from D and C."""
    D, C = np.asarray(D, F32), np.asarray(C, F32)
    N, M = D.shape
    wm, wa = _weights(weights_mul, weights_add)
    i, j = N - 1, M - 1
    if subseq:
        if np.isnan(D[N - 1]).any():
            return None, None
        j = int(np.argmin(D[N - 1]))            # the first of the minimal ones
    total = D[i, j]
    get = lambda a, b: D[a, b] if a >= 0 and b >= 0 else INF
    path = []
    with np.errstate(all="ignore"):
        while True:
            if np.isnan(D[i, j]) or D[i, j] == INF:
                return None, None
            path.append((i, j))
            if i == 0 and (subseq or j == 0):
                break
            best, step = None, 0
            for k, (di, dj) in enumerate(STEPS):
                v = F32(get(i - di, j - dj) + F32(F32(wm[k] * C[i, j]) + wa[k]))
                if best is None or v < best:
                    best, step = v, k
            i, j = i - STEPS[step][0], j - STEPS[step][1]
            if i < 0 or j < 0:
                return None, None
    return np.asarray(path[::-1], np.int32).reshape(-1, 2), total


def dtw64(C, weights_mul=None, weights_add=None, subseq=False, band=0):
    """A plain float64 DTW, written independently: (D, total, path ascending or None)."""
    C = np.asarray(C, np.float64)
    N, M = C.shape
    wm = [1.0, 1.0, 1.0] if weights_mul is None else [float(w) for w in weights_mul]
    wa = [0.0, 0.0, 0.0] if weights_add is None else [float(w) for w in weights_add]
    D = np.full((N, M), np.inf)
    choice = np.full((N, M), -1, np.int8)
    for i in range(N):
        for j in range(M):
            if i == 0 and (j == 0 or subseq):
                D[i, j] = C[i, j]
                continue
            if band and abs(j * (N - 1) - i * (M - 1)) > band * max(N - 1, 1):
                continue
            cands = []
            if i > 0 and j > 0:
                cands.append((D[i - 1, j - 1] + wm[0] * C[i, j] + wa[0], 0))
            if j > 0:
                cands.append((D[i, j - 1] + wm[1] * C[i, j] + wa[1], 1))
            if i > 0:
                cands.append((D[i - 1, j] + wm[2] * C[i, j] + wa[2], 2))
            D[i, j], choice[i, j] = min(cands)
    i, j = N - 1, (int(np.argmin(D[N - 1])) if subseq else M - 1)
    total = D[i, j]
    if not np.isfinite(total):
        return D, total, None
    path = [(i, j)]
    while not (i == 0 and (subseq or j == 0)):
        di, dj = STEPS[choice[i, j]]
        i, j = i - di, j - dj
        path.append((i, j))
    return D, total, np.asarray(path[::-1], np.int32)


def same_bits(a, b):
    """NaN positions equal, all other bits equal."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---------------------------------------------------------------------------------------------------- the inputs the tests share
def integer_costs(N, M, seed):
    """Costs 0..3 with a -0 among them: about a quarter of the cells tie."""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 4, (N, M)).astype(F32)
    C[rng.integers(0, N), rng.integers(0, M)] = F32(-0.0)
    return C


def float_costs(N, M, seed):
    return np.random.default_rng(seed).random((N, M), F32)


# ---------------------------------------------------------------------------------------------------- the cost against float64
def float64_cost(X, Y, metric):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    try:
        from scipy.spatial.distance import cdist
        return cdist(X, Y, metric)
    except ImportError:
        if metric == "cosine":
            return 1.0 - (X @ Y.T) / (np.linalg.norm(X, axis=1)[:, None] * np.linalg.norm(Y, axis=1)[None, :])
        sq = ((X[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
        return sq if metric == "sqeuclidean" else np.sqrt(sq)


def cost_data(kind, N, M, K, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, K)).astype(F32)
    Y = rng.standard_normal((M, K)).astype(F32)
    if kind == "positive":
        X, Y = np.abs(X), np.abs(Y)
    elif kind == "near-duplicate":
        Y = (X[rng.integers(0, N, M)] * F32(1 + 2.0 ** -12)).astype(F32)
    return X, Y


def cost_errors(metric, kind, K, N=24, M=20, seed=0):
    """(the worst error in units of 2^-24: relative for the Euclidean metrics, absolute for cosine; the bound in the same units)."""
    X, Y = cost_data(kind, N, M, K, seed)
    got = cost32(X, Y, metric).astype(np.float64)
    want = float64_cost(X, Y, metric)
    if metric == "cosine":
        return float(np.abs(got - want).max()) / 2.0 ** -24, K + 5
    nz = want != 0
    assert (got[~nz] == 0).all()
    return float((np.abs(got - want)[nz] / want[nz]).max()) / 2.0 ** -24, K + 3
