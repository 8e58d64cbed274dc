"""Harmonic-percussive separation (include/jsg.h section 2f): the float32 numpy restatement that the library matches bit for bit,
librosa's definition on float64 magnitudes, and the seeded inputs the tests share.  A helper, no tests."""
import functools

import numpy as np

U = 2.0 ** -24          # the unit round-off of float32


def refl(i, L: int):
    """scipy's "reflect" at any distance past the edge: (d c b a | a b c d | d c b a)."""
    m = np.mod(np.asarray(i, dtype=np.int64), 2 * L)
    return np.where(m < L, m, 2 * L - 1 - m)


def _median(P: np.ndarray, W: int, axis: int) -> np.ndarray:
    """The (h+1)-th smallest of the W reflected neighbours along `axis`, h = (W-1)/2: a selection, no arithmetic."""
    assert W % 2 == 1 and W >= 1
    h = (W - 1) // 2
    L = P.shape[axis]
    idx = refl(np.arange(L)[:, None] + np.arange(-h, h + 1)[None, :], L)        # [L][W]
    if axis == 0:
        return np.sort(P[idx], axis=1)[:, h, :]                                  # P[idx]: [T][W][K]
    return np.sort(P[:, idx], axis=2)[:, :, h]                                   # P[:, idx]: [T][K][W]


def power(X: np.ndarray) -> np.ndarray:
    """re*re + im*im in float32, each operation rounded (complex input), or the input itself (real power)."""
    X = np.asarray(X)
    if np.iscomplexobj(X):
        X = X.astype(np.complex64)
        re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
        return (re * re).astype(np.float32) + (im * im).astype(np.float32)
    return X.astype(np.float32)


def mirror(X, W_t: int, W_f: int, m_h: float = 1.0, m_p: float = 1.0):
    """The definition of section 2f in float32, every operation rounded separately: X [T][K] complex64, or float32 power ->
    (mask_h, mask_p, out_h, out_p, H, C); the outputs have the input's kind."""
    f32 = np.float32
    X = np.asarray(X)
    P = power(X)
    with np.errstate(all="ignore"):
        H, C = _median(P, W_t, 0), _median(P, W_f, 1)
        g_h, g_p = f32(m_h) * f32(m_h), f32(m_p) * f32(m_p)
        D_h = H + (g_h * C).astype(f32)
        D_p = C + (g_p * H).astype(f32)
        M_h = np.where(D_h > 0, H / np.where(D_h > 0, D_h, f32(1)), f32(0)).astype(f32)
        M_p = np.where(D_p > 0, C / np.where(D_p > 0, D_p, f32(1)), f32(0)).astype(f32)
        if np.iscomplexobj(X):
            Xc = X.astype(np.complex64)
            re, im = Xc.real, Xc.imag
            out_h, out_p = np.empty_like(Xc), np.empty_like(Xc)
            out_h.real, out_h.imag = M_h * re, M_h * im
            out_p.real, out_p.imag = M_p * re, M_p * im
        else:
            out_h, out_p = (M_h * P).astype(f32), (M_p * P).astype(f32)
    return M_h, M_p, out_h, out_p, H, C


def reference64(X, W_t: int, W_f: int, m_h: float = 1.0, m_p: float = 1.0):
    """librosa.decompose.hpss(|X|, kernel_size=(W_f, W_t), power=2, margin=(m_h, m_p), mask=True) in float64 on magnitudes, with a
    mask of 0 where its denominator is 0: X [T][K] -> (mask_h, mask_p)."""
    X = np.asarray(X)
    S = np.abs(X.astype(np.complex128)) if np.iscomplexobj(X) else np.sqrt(X.astype(np.float64))
    harm, perc = _median(S, W_t, 0), _median(S, W_f, 1)

    def soft(a, b):
        a2, b2 = a * a, b * b
        d = a2 + b2
        return np.where(d > 0, a2 / np.where(d > 0, d, 1.0), 0.0)

    return soft(harm, perc * float(m_h)), soft(perc, harm * float(m_p))


@functools.lru_cache(maxsize=32)
def make_input(T: int, K: int, seed: int = 0) -> np.ndarray:
    """complex64 [T][K]: complex normal values times 10^U(-6, 3), so that powers and their products stay normal floats.  Read-only:
    the tests share it."""
    rng = np.random.default_rng(seed + 1000003 * T + 7919 * K)
    z = rng.standard_normal((T, K)) + 1j * rng.standard_normal((T, K))
    X = (z * 10.0 ** rng.uniform(-6.0, 3.0, (T, K))).astype(np.complex64)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=8)
def tie_input(T: int, K: int, seed: int = 0) -> np.ndarray:
    """complex64 [T][K] with parts drawn from {0, 1, 2, 3} (many equal powers), and a block of zeros in the middle large enough to
    hold whole-zero windows of 31 either way."""
    rng = np.random.default_rng(seed + 15485863 + 1000003 * T + 7919 * K)
    X = (rng.integers(0, 4, (T, K)) + 1j * rng.integers(0, 4, (T, K))).astype(np.complex64)
    X[T // 2 - min(24, T // 2):T // 2 + 24, K // 2 - min(24, K // 2):K // 2 + 24] = 0
    X.setflags(write=False)
    return X


# (T, K, W_t, W_f) of the bit-for-bit GPU checks and of the accuracy report
GEOMETRIES = [(96, 257, 31, 31), (70, 65, 63, 63), (5, 3, 31, 63), (1, 1, 1, 1), (1, 513, 31, 31), (130, 1, 31, 31), (67, 129, 3, 5),
              (200, 130, 17, 9), (40, 63, 31, 31), (40, 64, 31, 31), (40, 65, 31, 31)]


def geometry_id(g) -> str:
    return "T{}-K{}-Wt{}-Wf{}".format(*g)
