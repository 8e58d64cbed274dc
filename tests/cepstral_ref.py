"""Cepstral coefficients and delta features (include/jsg.h section 2k): the definitions evaluated in float64, the float32 restatements
in the library's stated orders, the two per-element bounds, the table formulas, the shared planes.  numpy only;
tests/test_cepstral_ref.py checks this module on the CPU, tests/test_gpu_cepstral.py compares the GPU against it.

The restatements: the projection, one accumulator per coefficient and acc = fmaf(D[m][b], S[t][b], acc) for b ascending; delta, one
per element and acc = fmaf(w[j], X[frame j][m], acc) for j ascending.  The float32 fmaf is the exact emulation of tests/rhythm_ref.py.
"""
import functools
import math

import numpy as np

from rhythm_ref import U, fma32

INTERP, NEAREST = 0, 1


# ---------------------------------------------------------------------------------------------------- projection
def project64(S, D):
    """S [..., T, B], D [M, B] float32 -> (C64 [..., T, M], bound [..., T, M]): the sum in float64 of the exact products of the float32
    operands, and (B + 2) u sum |D| |S|."""
    S, D = np.asarray(S, np.float32).astype(np.float64), np.asarray(D, np.float32).astype(np.float64)
    B = S.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        return S @ D.T, (B + 2) * U * (np.abs(S) @ np.abs(D).T)


def project32(S, D):
    """The float32 restatement: [..., T, M] float32."""
    S, D = np.asarray(S, np.float32), np.asarray(D, np.float32)
    acc = np.zeros(S.shape[:-1] + (D.shape[0],), np.float32)
    for b in range(S.shape[-1]):
        acc = fma32(D[:, b], S[..., b:b + 1], acc)
    return acc


# ---------------------------------------------------------------------------------------------------- delta
def window_frames(T, width, mode):
    """[T][width] frame indices of the window of every frame."""
    h = width // 2
    t = np.arange(T)[:, None]
    j = np.arange(width)[None, :]
    if mode == INTERP:
        assert T >= width
        return np.clip(t - h, 0, T - width) + j
    return np.clip(t - h + j, 0, T - 1)


def delta64(X, w, mode):
    """X [..., T, M], w [Wd] float32 -> (Y64, bound), both [..., T, M]: bound = (Wd + 2) u sum |w| |X|."""
    X, w = np.asarray(X, np.float32).astype(np.float64), np.asarray(w, np.float32).astype(np.float64)
    idx = window_frames(X.shape[-2], w.size, mode)
    with np.errstate(invalid="ignore", over="ignore"):
        G = X[..., idx, :]                          # [..., T, Wd, M]
        return np.einsum("...tjm,j->...tm", G, w), (w.size + 2) * U * np.einsum("...tjm,j->...tm", np.abs(G), np.abs(w))


def delta32(X, w, mode):
    """The float32 restatement: [..., T, M] float32."""
    X, w = np.asarray(X, np.float32), np.asarray(w, np.float32)
    idx = window_frames(X.shape[-2], w.size, mode)
    acc = np.zeros(X.shape, np.float32)
    for j in range(w.size):
        acc = fma32(w[j:j + 1], X[..., idx[:, j], :], acc)
    return acc


# ---------------------------------------------------------------------------------------------------- tables
def lifter64(M, lifter):
    m = np.arange(M, dtype=np.float64)
    return np.ones(M) if lifter == 0 else 1.0 + (lifter / 2.0) * np.sin(np.pi * (m + 1) / lifter)


def dct_table64(B, M, norm="ortho", lifter=0.0, inverse=False):
    """The table formulas of section 2k in float64: forward [M][B], inverse [B][M]."""
    m = np.arange(M)[:, None]
    b = np.arange(B)[None, :]
    k = (m * (2 * b + 1)) % (4 * B)                 # integers
    c = np.cos(np.pi * k / (2.0 * B))
    s = np.ones((M, 1))
    if norm == "ortho":
        s = np.where(m == 0, math.sqrt(1.0 / (4 * B)), math.sqrt(1.0 / (2 * B)))
    L = lifter64(M, lifter)[:, None]
    if not inverse:
        return 2 * c * s * L
    if norm == "ortho":
        return (2 * c * s / L).T
    return (np.where(m == 0, 1.0, 2 * c) / (2.0 * B) / L).T


def delta_weights64(width, order):
    """order! x row `order` of the pseudo-inverse of the Vandermonde matrix of j - h (columns 1, x, x^2, ...)."""
    x = np.arange(width, dtype=np.float64) - width // 2
    return math.factorial(order) * np.linalg.pinv(np.vander(x, order + 1, increasing=True))[order]


# ---------------------------------------------------------------------------------------------------- shared planes
@functools.lru_cache(maxsize=None)
def planes(R=3, T=200, B=257):
    """[R][T][B] float32 dB-like planes (noise around -40 dB, a slow rise, a few loud frames).  Read-only."""
    rng = np.random.default_rng(20261020)
    S = -40.0 + 12.0 * rng.standard_normal((R, T, B))
    S[1] += 0.1 * np.arange(T)[:, None]
    S[2, ::11] += 30.0
    S = S.astype(np.float32)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def tables(M, B, seed=0):
    """A dense [M][B] float32 table: the orthonormal DCT where M <= B (seed 0), else noise.  Read-only."""
    if seed == 0 and M <= B:
        D = dct_table64(B, M).astype(np.float32)
    else:
        D = (np.random.default_rng(seed + 1000 * M + B).standard_normal((M, B)) / math.sqrt(B)).astype(np.float32)
    D.setflags(write=False)
    return D


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def same_but_nan(a, b):
    """same(), with a NaN of any sign and payload equal to any other NaN."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and same(np.nan_to_num(a, posinf=3e38, neginf=-3e38), np.nan_to_num(b, posinf=3e38, neginf=-3e38)) \
        and np.array_equal(np.isinf(a), np.isinf(b))
