"""The k nearest frames, the recurrence plane and the neighbour aggregation (include/jsgx.h sections 6 to 8): the float32 restatement in
the library's stated operations, a brute-force transcription of the definition, and the inputs the tests share.  numpy only;
tests/test_knn_ref.py checks this module on the CPU, tests/test_gpu_knn.py compares the GPU against it bit for bit.

The restatement: the costs are dtw_ref.cost32 (section 2, operation by operation); the selection is np.lexsort on (j, c) over the
candidates (the float comparison: -0 == +0); the affinity is beat_ref.exp32 (jsgx_exp operation by operation); the aggregation adds in
ascending r with beat_ref.fma32 where the header writes fmaf.
"""
import numpy as np

from beat_ref import exp32, fma32
from dtw_ref import cost32, same_bits  # noqa: F401

F32 = np.float32
INF = F32(np.inf)
MAX_K = 256
MODES = {"connectivity": 0, "distance": 1, "affinity": 2}


def default_k(n, width=0):
    """librosa's 2 * ceil(sqrt(n - 2 width + 1)), clamped to 1..256."""
    t = n - 2 * width + 1
    return max(1, min(MAX_K, 2 * int(np.ceil(np.sqrt(t))))) if t > 0 else 1


def select32(C, k, width=0, col0=0):
    """(index int32 [N, k], dist float32 [N, k]) of the cost plane C [N, M'] whose column 0 is frame col0 of y: the definition of section 6."""
    C = np.asarray(C, F32)
    N, M = C.shape
    index, dist = np.full((N, k), -1, np.int32), np.full((N, k), INF, F32)
    j = np.arange(col0, col0 + M)
    for i in range(N):
        cand = np.flatnonzero((np.abs(i - j) >= width) & ~np.isnan(C[i]))
        order = cand[np.lexsort((cand, C[i, cand]))][:k]
        index[i, :order.size] = j[order]
        dist[i, :order.size] = C[i, order]
    return index, dist


def knn32(X, Y, k, width=0, metric="euclidean"):
    return select32(cost32(X, Y, metric), k, width)


def select_brute(C, k, width=0):
    """The same by the text of the header, one candidate at a time: an insertion into a sorted list with the key (c, j)."""
    C = np.asarray(C, F32)
    N, M = C.shape
    index, dist = np.full((N, k), -1, np.int32), np.full((N, k), INF, F32)
    for i in range(N):
        best = []
        for j in range(M):
            c = C[i, j]
            if abs(i - j) < width or c != c:
                continue
            at = len(best)
            while at > 0 and (c < best[at - 1][0]):       # j ascends: an equal cost stays behind
                at -= 1
            best.insert(at, (c, j))
            del best[k:]
        for r, (c, j) in enumerate(best):
            index[i, r], dist[i, r] = j, c
    return index, dist


def merge_lists(parts, k):
    """The lists of consecutive column ranges, in ascending order of the ranges, merged as "knn_merge" does: the k smallest of their union
    by (c, j)."""
    index = np.concatenate([p[0] for p in parts], axis=1)
    dist = np.concatenate([p[1] for p in parts], axis=1)
    N = index.shape[0]
    out_i, out_d = np.full((N, k), -1, np.int32), np.full((N, k), INF, F32)
    for i in range(N):
        cand = np.flatnonzero(index[i] >= 0)
        order = cand[np.lexsort((index[i, cand], dist[i, cand]))][:k]
        out_i[i, :order.size], out_d[i, :order.size] = index[i, order], dist[i, order]
    return out_i, out_d


def split_select32(C, k, width, S):
    """select32 by S column ranges of whole tiles of 64, as the kernel cuts them: tiles floor(s T / S) .. floor((s + 1) T / S) - 1."""
    M = C.shape[1]
    T = -(-M // 64)
    S = min(S, T)
    parts = []
    for s in range(S):
        a, b = 64 * (s * T // S), min(M, 64 * ((s + 1) * T // S))
        parts.append(select32(C[:, a:b], k, width, col0=a))
    return merge_lists(parts, k)


def affinity32(d, bw):
    """jsgx_exp(-fl(d / bw)); NaN where !(bw > 0) or d is a NaN."""
    d, bw = np.asarray(d, F32), F32(bw)
    with np.errstate(all="ignore"):
        bad = ~(bw > 0) | np.isnan(d)
        x = -(np.where(bad, F32(0), d) / (bw if bw > 0 else F32(1)))
        return np.where(bad, F32(np.nan), exp32(x.astype(F32))).astype(F32)


def recurrence32(index, dist, M, mode="connectivity", sym=False, diag=False, bw=None):
    """The plane [N, M] of section 7 from the lists of one pair."""
    N, k = index.shape
    out = np.zeros((N, M), F32)
    member = np.zeros((N, M), bool)
    rows = np.repeat(np.arange(N), k)
    ok = (index.ravel() >= 0) & (index.ravel() < M)
    member[rows[ok], index.ravel()[ok]] = True
    if mode == "connectivity":
        value = np.ones((N, k), F32)
    elif mode == "distance":
        value = np.asarray(dist, F32)
    else:
        value = affinity32(dist, bw)
    link = member & member.T if sym else member
    for i in range(N):
        for r in range(k):
            j = index[i, r]
            if 0 <= j < M and link[i, j]:
                out[i, j] = value[i, r]
    if diag:
        d = np.arange(min(N, M))
        out[d, d] = F32(0.0 if mode == "distance" else 1.0)
    return out


def bandwidth32(dist):
    """librosa's med_k_scalar as the Python layer states it: of the finite dist[i][k-1] sorted ascending, 0.5f * (v[(c-1)//2] + v[c//2])."""
    last = np.asarray(dist, F32)[:, -1]
    v = np.sort(last[np.isfinite(last)])
    c = v.size
    if c == 0:
        return INF
    return F32(F32(0.5) * F32(v[(c - 1) // 2] + v[c // 2]))


def nn_filter32(S, index, weights=None):
    """Section 8 for one pair: S [N, F], index [N, k], weights [N, k] or None."""
    S = np.asarray(S, F32)
    N, F = S.shape
    k = index.shape[1]
    acc, den, cnt = np.zeros((N, F), F32), np.zeros((N, 1), F32), np.zeros((N, 1), np.int64)
    with np.errstate(all="ignore"):
        for r in range(k):
            j = index[:, r]
            ok = ((j >= 0) & (j < N))[:, None]
            v = S[np.where(ok[:, 0], j, 0)]
            if weights is None:
                acc = np.where(ok, acc + v, acc)
            else:
                w = np.asarray(weights, F32)[:, r, None]
                acc = np.where(ok, fma32(np.broadcast_to(w, v.shape), v, acc), acc)
                den = np.where(ok, den + w, den)
            cnt += ok
        if weights is None:
            den = cnt.astype(F32)
        own = (cnt == 0) | (den == 0)
        return np.where(own, S, acc / np.where(own, F32(1), den)).astype(F32)


# ---------------------------------------------------------------------------------------------------- the inputs the tests share
def frames(kind, N, M, K, seed):
    """(X [N, K], Y [M, K]) float32 of one kind:
    integers     small integer features with duplicate frames: massive ties, the tie rule decides most entries
    floats       standard normal
    approaching  column j + 1 always nearer to every x than column j: every tile inserts, the merge's worst case
    receding     column j + 1 always farther: nothing inserts once the lists are full
    nan_y        floats with a NaN frame in y, which is never selected
    nan_x        floats with a NaN frame in x: that row has no candidate
    inf          floats with a +inf feature in one frame of y: a cost of +inf (or a NaN under cosine) like any other
    zero         floats with a zero vector in x and in y (cosine: the cost 1)"""
    rng = np.random.default_rng(seed)
    if kind == "integers":
        return rng.integers(0, 3, (N, K)).astype(F32), rng.integers(0, 3, (M, K)).astype(F32)
    if kind in ("approaching", "receding"):
        X = (rng.random((N, K)) * 0.25).astype(F32)
        far = (np.arange(M, 0, -1) if kind == "approaching" else np.arange(1, M + 1)).astype(F32)
        Y = np.zeros((M, K), F32)
        Y[:, 0] = far + F32(1.0)
        return X, Y
    X, Y = rng.standard_normal((N, K)).astype(F32), rng.standard_normal((M, K)).astype(F32)
    if kind == "nan_y":
        Y[M // 2, K // 2] = np.nan
    elif kind == "nan_x":
        X[N // 2, 0] = np.nan
    elif kind == "inf":
        Y[M // 3, K - 1] = np.inf
    elif kind == "zero":
        X[N // 2] = 0
        Y[M // 2] = 0
    else:
        assert kind == "floats"
    return X, Y


KINDS = ("integers", "floats", "approaching", "receding", "nan_y", "nan_x", "inf", "zero")
