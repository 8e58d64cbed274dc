"""Recurrence quantification alignment (include/jsgx.h section 9): the float32 restatement in the library's stated operations row by row,
the header's text cell by cell, the backtrace that recomputes the forward choice, and an independent brute force over every chain of
allowed steps.  numpy only; tests/test_rqa_ref.py checks this module on the CPU, tests/test_gpu_rqa.py compares the GPU against it bit
for bit.

The restatement: every predecessor of a cell lies in an earlier row, so a row is one vector operation on the two rows above it.
"""
import numpy as np

from dtw_ref import same_bits  # noqa: F401  (the comparison the GPU tests use)

F32 = np.float32
STEPS = ((1, 1), (1, 2), (2, 1))          # (di, dj) of k = 0, 1, 2


def _select(best, kk, v, k, where=True):
    """if (v > best) { best = v; kk = k; }: strict, so the lowest k wins ties and a NaN never replaces best."""
    take = (v > best) & where
    return np.where(take, v, best), np.where(take, np.int8(k), kk)


def rqa32(R, gap_onset=1.0, gap_extend=1.0, knight=True):
    """(S float32 [N, M], step int8 [N, M]) of section 9, row by row."""
    R = np.asarray(R, F32)
    N, M = R.shape
    link = R > 0
    pen = np.where(link, F32(gap_onset), F32(gap_extend)).astype(F32)          # what a step FROM this cell into a gap costs
    S = np.empty((N, M), F32)
    step = np.empty((N, M), np.int8)
    S[0], S[:, 0] = R[0], R[:, 0]
    step[0], step[:, 0] = np.where(link[0], -2, -1), np.where(link[:, 0], -2, -1)
    with np.errstate(all="ignore"):
        for i in range(1, N):
            if M < 2:
                break
            lk, r = link[i, 1:], R[i, 1:]
            a = S[i - 1, :-1]
            best = np.where(lk, a, a - pen[i - 1, :-1]).astype(F32)             # k = 0: (i-1, j-1), every j >= 1
            kk = np.zeros(M - 1, np.int8)
            if knight and M > 2:                                                # k = 1: (i-1, j-2), j >= 2
                b = S[i - 1, :-2]
                v1 = np.where(lk[1:], b, b - pen[i - 1, :-2]).astype(F32)
                best[1:], kk[1:] = _select(best[1:], kk[1:], v1, 1)
            if knight and i >= 2:                                               # k = 2: (i-2, j-1)
                c = S[i - 2, :-1]
                v2 = np.where(lk, c, c - pen[i - 2, :-1]).astype(F32)
                best, kk = _select(best, kk, v2, 2)
            keep = best > 0
            S[i, 1:] = np.where(lk, best + r, np.where(keep, best, F32(0)))
            step[i, 1:] = np.where(lk | keep, kk, np.int8(-1))
    return S, step


def _cell(S, R, i, j, on, ex, knight):
    """(S, step) of an inner cell from S and R of its predecessors: the header's text."""
    link = R[i, j] > 0
    best, kstar = None, -1
    for k, (di, dj) in enumerate(STEPS[:3 if knight else 1]):
        pi, pj = i - di, j - dj
        if pi < 0 or pj < 0:
            continue
        v = S[pi, pj] if link else F32(S[pi, pj] - (on if R[pi, pj] > 0 else ex))
        if best is None or v > best:
            best, kstar = v, k
    if link:
        return F32(best + R[i, j]), kstar
    return (best, kstar) if best > 0 else (F32(0), -1)


def rqa32_loop(R, gap_onset=1.0, gap_extend=1.0, knight=True):
    """The same (S, step) cell by cell with numpy float32 scalars."""
    R = np.asarray(R, F32)
    N, M = R.shape
    on, ex = F32(gap_onset), F32(gap_extend)
    S = np.empty((N, M), F32)
    step = np.empty((N, M), np.int8)
    with np.errstate(all="ignore"):
        for i in range(N):
            for j in range(M):
                if i == 0 or j == 0:
                    S[i, j], step[i, j] = R[i, j], (-2 if R[i, j] > 0 else -1)
                else:
                    S[i, j], step[i, j] = _cell(S, R, i, j, on, ex, knight)
    return S, step


def end_cell(S):
    """(i, j) of the largest S > 0, the lowest i and then the lowest j among equal ones; None where no S > 0."""
    ok = S > 0
    if not ok.any():
        return None
    flat = int(np.argmax(np.where(ok, S, F32(-np.inf))))          # numpy's flat argmax: the first of the maximal ones
    return flat // S.shape[1], flat % S.shape[1]


def backtrace32(S, R, gap_onset=1.0, gap_extend=1.0, knight=True):
    """(path int32 [L, 2] ascending, end (i, j), total) of section 9 from S and R, the step of every cell recomputed; no S > 0:
    (an empty path, (-1, -1), +0)."""
    S, R = np.asarray(S, F32), np.asarray(R, F32)
    on, ex = F32(gap_onset), F32(gap_extend)
    end = end_cell(S)
    if end is None:
        return np.zeros((0, 2), np.int32), (-1, -1), F32(0)
    i, j = end
    path = []
    with np.errstate(all="ignore"):
        while True:
            if i == 0 or j == 0:
                step = -2 if R[i, j] > 0 else -1
            else:
                step = _cell(S, R, i, j, on, ex, knight)[1]
            if step == -1:
                break
            path.append((i, j))
            if step == -2:
                break
            i, j = i - STEPS[step][0], j - STEPS[step][1]
    return np.asarray(path[::-1], np.int32).reshape(-1, 2), end, S[end]


def rqa_chains(R, gap_onset=1.0, gap_extend=1.0, knight=True):
    """The largest score of any chain that ends at each cell, by enumeration.  Every inner cell has the candidate k = 0, so every chain
    starts at a border cell; a chain is folded as s = R[c0], then per cell: a link adds R, a gap gives max(0, s - pen) with pen by the
    cell it comes from.  The fold is monotone in s, so the maximum over chains is what the recurrence keeps.  For planes without NaN."""
    R = np.asarray(R, F32)
    N, M = R.shape
    on, ex = F32(gap_onset), F32(gap_extend)
    out = np.full((N, M), -np.inf, F32)
    steps = STEPS[:3 if knight else 1]

    def walk(i, j, s):
        if s > out[i, j]:
            out[i, j] = s
        for di, dj in steps:
            ni, nj = i + di, j + dj
            if ni < N and nj < M:
                if R[ni, nj] > 0:
                    t = F32(s + R[ni, nj])
                else:
                    t = F32(s - (on if R[i, j] > 0 else ex))
                    t = t if t > 0 else F32(0)
                walk(ni, nj, t)

    for i in range(N):
        for j in range(M):
            if i == 0 or j == 0:
                walk(i, j, R[i, j])
    return out


# ---------------------------------------------------------------------------------------------------- the planes the tests share
def integer_links(N, M, seed):
    """About 35 % links with the values 1..3: many ties, and every operation exact with dyadic penalties."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((N, M)) < 0.35, rng.integers(1, 4, (N, M)), 0).astype(F32)


def float_links(N, M, seed):
    """About 35 % links with affinities in (0, 1]."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((N, M)) < 0.35, 1.0 - rng.random((N, M)), 0.0).astype(F32)
