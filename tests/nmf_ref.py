"""numpy restatement of include/jsgx.h section 12 (non-negative matrix factorisation by multiplicative updates, Frobenius loss): the
float32 form, operation by operation on rhythm_ref.fma32, whose bits the GPU must give; the float64 form, which is scikit-learn's
solver="mu"; the seeded inputs the tests share.  The chunk lengths come from capix (the header's constants), never from a literal."""
import functools

import numpy as np

from rhythm_ref import fma32

from jadespectrogram_amd import capix

CHUNK_K, CHUNK_T = capix.NMF_CHUNK_K, capix.NMF_CHUNK_T
EPSILON = np.float32(capix.NMF_EPSILON)
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------- inputs
def plane(T, K, seed):
    """random ** 4: the exponents spread over many binades, so the order of a sum shows in its bits."""
    return (np.random.default_rng(seed).random((T, K)) ** 4).astype(np.float32)


def start(T, K, r, seed):
    """(A [T][r], C [r][K]): positive, spread like the plane."""
    rng = np.random.default_rng(seed + 1000)
    return (rng.random((T, r)) ** 3 + 0.01).astype(np.float32), (rng.random((r, K)) ** 3 + 0.01).astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(T, K, r, seed=0):
    """(V, A0, C0) of a shape, built once and shared read-only."""
    V = plane(T, K, seed)
    A, C = start(T, K, r, seed)
    for x in (V, A, C):
        x.setflags(write=False)
    return V, A, C


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------- float32, the contract
def chunked_dot32(X, Y, chunk=None, reverse=False):
    """out[m][n] = the chunked sum over i of X[m][i] * Y[n][i]: a fmaf chain from +0 over each chunk, i ascending (descending with
    `reverse`, which is no part of the definition: the probe's control), the chunks' results added in ascending order.  chunk None: one chain."""
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    n = X.shape[1]
    chunk = chunk or max(n, 1)
    total = None
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        acc = np.zeros((X.shape[0], Y.shape[0]), np.float32)
        for i in (range(hi - 1, lo - 1, -1) if reverse else range(lo, hi)):
            acc = fma32(X[:, i:i + 1], Y[None, :, i], acc)
        total = acc if total is None else (total + acc).astype(np.float32)
    return total


def _ratio32(old, num, den):
    with np.errstate(all="ignore"):
        dz = np.where(den != 0, den, EPSILON).astype(np.float32)
        return (old * (num / dz).astype(np.float32)).astype(np.float32)


def update_a32(V, A, C, reverse=False):
    N = chunked_dot32(V, C, CHUNK_K, reverse)
    G = chunked_dot32(C, C, CHUNK_K, reverse)
    D = chunked_dot32(A, G.T)                   # D[t][c] = chain over c' of A[t][c'] * G[c'][c]
    return _ratio32(np.asarray(A, np.float32), N, D)


def update_c32(V, A, C):
    At, Vt = np.ascontiguousarray(np.asarray(A, np.float32).T), np.ascontiguousarray(np.asarray(V, np.float32).T)
    N2 = chunked_dot32(At, Vt, CHUNK_T)
    G2 = chunked_dot32(At, At, CHUNK_T)
    D2 = chunked_dot32(G2, np.asarray(C, np.float32).T)       # D2[c][k] = chain over c' of G2[c][c'] * C[c'][k]
    return _ratio32(np.asarray(C, np.float32), N2, D2)


def nmf32(V, A, C, n_iter, update_components=True):
    """(A, C) after n_iter iterations, as the header states them."""
    A, C = np.array(A, np.float32), np.array(C, np.float32)
    for _ in range(n_iter):
        A = update_a32(V, A, C)
        if update_components:
            C = update_c32(V, A, C)
    return A, C


# ---------------------------------------------------------------------------------------------------- float64, scikit-learn's form
def _ratio64(old, num, den):
    den = den.copy()
    den[den == 0] = float(EPSILON)
    return old * (num / den)


def update_a64(V, A, C):
    return _ratio64(A, V @ C.T, A @ (C @ C.T))


def update_c64(V, A, C):
    return _ratio64(C, A.T @ V, (A.T @ A) @ C)


def nmf64(V, A, C, n_iter, update_components=True, losses=None):
    V, A, C = (np.array(x, np.float64) for x in (V, A, C))
    for _ in range(n_iter):
        A = update_a64(V, A, C)
        if update_components:
            C = update_c64(V, A, C)
        if losses is not None:
            losses.append(float(np.linalg.norm(V - A @ C)))
    return A, C


def constant_start(V, r):
    """The activations scikit-learn's transform (update_H=False) starts from."""
    return np.sqrt(np.asarray(V, np.float64).mean() / r)


def update_bound(n, chunk, r):
    """The relative error of one float32 update against the exact one on the same inputs, every term non-negative: a chunked sum of n
    terms carries at most L = min(n, chunk) + ceil(n / chunk) roundings (the chain, then the adds), twice for the numerator and the Gram
    matrix, r more for the D chain, and three for the divide, the multiply and the rounding of the result: g u / (1 - g u), g = 2 L + r + 3."""
    L = min(n, chunk) + -(-n // chunk)
    g = (2 * L + r + 3) * U
    return g / (1 - g)
