"""tests/cepstral_ref.py checked on the CPU: the float32 restatements against the float64 definitions under the two bounds, the window
of a delta frame in both edge modes, and the table and weight formulas against scipy (where it imports) and numpy.linalg.pinv."""
import math

import numpy as np
import pytest

import cepstral_ref as cr


@pytest.mark.parametrize("B,M", [(1, 1), (3, 2), (33, 13), (128, 20), (257, 20), (20, 128)])
def test_projection_restatement_stays_within_the_bound(B, M):
    S = cr.planes()[:2, :40, :B]
    D = cr.tables(M, B)
    C64, bound = cr.project64(S, D)
    C32 = cr.project32(S, D)
    assert C32.dtype == np.float32 and C32.shape == (2, 40, M)
    assert (np.abs(C32.astype(np.float64) - C64) <= bound).all()
    # b really ascends: the chain of one element by hand
    acc = np.float32(0)
    for b in range(B):
        acc = cr.fma32(D[M - 1, b:b + 1], S[1, 7, b:b + 1], acc)[0]
    assert cr.same(np.array(acc), np.array(C32[1, 7, M - 1]))


def test_projection_nan_stays_in_its_frame():
    S = np.array(cr.planes()[0, :10, :8])
    D = np.array(cr.tables(3, 8))
    D[1, 5] = 0                                     # a zero in the table does not stop a NaN
    clean = cr.project32(S, D)
    S[4, 5] = np.nan
    S[6, 0] = np.inf
    got = cr.project32(S, D)
    assert np.isnan(got[4]).all() and not np.isnan(np.delete(got, 4, axis=0)).any()
    assert cr.same(np.delete(got, [4, 6], axis=0), np.delete(clean, [4, 6], axis=0))
    assert (np.isinf(got[6]) | np.isnan(got[6])).all()


@pytest.mark.parametrize("mode", [cr.INTERP, cr.NEAREST])
def test_window_frames(mode):
    idx = cr.window_frames(12, 5, mode)
    assert idx.shape == (12, 5) and idx.min() == 0 and idx.max() == 11
    assert (idx[2:10] == np.arange(2, 10)[:, None] - 2 + np.arange(5)).all()        # the interior: centred
    if mode == cr.INTERP:
        assert (idx[:3] == np.arange(5)).all() and (idx[9:] == np.arange(7, 12)).all()
    else:
        assert list(idx[0]) == [0, 0, 0, 1, 2] and list(idx[11]) == [9, 10, 11, 11, 11]
    assert (cr.window_frames(1, 3, cr.NEAREST) == 0).all()


@pytest.mark.parametrize("width,order", [(3, 1), (5, 2), (9, 1), (9, 2), (255, 1), (255, 3)])
@pytest.mark.parametrize("mode", [cr.INTERP, cr.NEAREST])
def test_delta_restatement_stays_within_the_bound(width, order, mode):
    X = cr.planes()[:2, :, :13]
    X = X if width < 200 else np.concatenate([X, X], axis=1)[:, :width + 1]
    w = cr.delta_weights64(width, order).astype(np.float32)
    Y64, bound = cr.delta64(X, w, mode)
    Y32 = cr.delta32(X, w, mode)
    assert Y32.dtype == np.float32 and Y32.shape == X.shape
    assert (np.abs(Y32.astype(np.float64) - Y64) <= bound).all()


def test_delta_of_a_line_is_its_slope():
    t = np.arange(40, dtype=np.float64)
    X = (3.0 + 0.25 * t[:, None] * np.arange(1, 4)[None, :]).astype(np.float32)
    w1, w2 = cr.delta_weights64(9, 1).astype(np.float32), cr.delta_weights64(9, 2).astype(np.float32)
    Y, bound = cr.delta64(X, w1, cr.INTERP)
    assert (np.abs(Y - 0.25 * np.arange(1, 4)) <= bound + 1e-6).all()               # the weights are rounded to float32: 1e-6 covers it
    Y2, bound2 = cr.delta64(X, w2, cr.INTERP)
    assert (np.abs(Y2) <= bound2 + 1e-5).all()
    assert np.allclose(cr.delta_weights64(9, 1), (np.arange(9) - 4) / 60.0, rtol=0, atol=1e-15)


def test_dct_tables_against_scipy():
    fft = pytest.importorskip("scipy.fft")
    B, M = 128, 20
    eye = np.eye(B)
    for norm in ("ortho", None):
        full = fft.dct(eye, type=2, norm=norm, axis=0)             # [k][b]: column b is the DCT of e_b
        assert np.abs(cr.dct_table64(B, M, norm or "none") - full[:M]).max() <= 2e-15 * max(1.0, np.abs(full).max())
        inv = fft.idct(np.eye(M), type=2, norm=norm, n=B, axis=0)  # [b][m]: column m is the zero-padded inverse of e_m
        assert np.abs(cr.dct_table64(B, M, norm or "none", inverse=True) - inv).max() <= 2e-15
    L = cr.lifter64(M, 22.0)
    assert np.allclose(cr.dct_table64(B, M, "ortho", 22.0), fft.dct(eye, type=2, norm="ortho", axis=0)[:M] * L[:, None], rtol=0, atol=1e-13)
    assert np.allclose(cr.dct_table64(B, M, "ortho", 22.0, inverse=True), fft.idct(np.eye(M) / L[:, None], type=2, norm="ortho", n=B, axis=0), rtol=0, atol=1e-13)


def test_dct_tables_without_scipy():
    """The same facts from numpy alone: the rows of the orthonormal table are orthonormal, the inverse undoes the forward for M = B, and
    the unnormalised table is the textbook sum."""
    for B in (1, 2, 7, 64):
        D = cr.dct_table64(B, B)
        assert np.abs(D @ D.T - np.eye(B)).max() <= 1e-13
        for norm in ("ortho", "none"):
            for lifter in (0.0, 22.0):
                assert np.abs(cr.dct_table64(B, B, norm, lifter, inverse=True) @ cr.dct_table64(B, B, norm, lifter) - np.eye(B)).max() <= 1e-12
        m, b = np.arange(B)[:, None], np.arange(B)[None, :]
        assert np.abs(cr.dct_table64(B, B, "none") - 2 * np.cos(np.pi * m * (2 * b + 1) / (2 * B))).max() <= 1e-12


@pytest.mark.parametrize("width,order", [(9, 1), (9, 2), (5, 2), (3, 1), (255, 3)])
def test_delta_weights_against_savgol(width, order):
    signal = pytest.importorskip("scipy.signal")
    want = signal.savgol_coeffs(width, order, deriv=order, use="dot")
    assert np.abs(cr.delta_weights64(width, order) - want).max() <= 1e-12 * np.abs(want).max() + 1e-15
    x = np.random.default_rng(5).standard_normal((width + 3, 2))
    for mode, name in ((cr.INTERP, "interp"), (cr.NEAREST, "nearest")):
        idx = cr.window_frames(x.shape[0], width, mode)
        got = np.einsum("tjm,j->tm", x[idx, :], cr.delta_weights64(width, order))
        assert np.abs(got - signal.savgol_filter(x, width, order, deriv=order, axis=0, mode=name)).max() <= 1e-9 * np.abs(want).max() * width


def test_delta_weights_fit_polynomials():
    """Without scipy: the weights take x^order to order! and every lower power to 0, and are (anti)symmetric."""
    for width, order in ((3, 1), (3, 2), (5, 2), (9, 1), (9, 4), (255, 3)):
        w = cr.delta_weights64(width, order)
        x = np.arange(width, dtype=np.float64) - width // 2
        for p in range(order + 1):
            want = math.factorial(order) if p == order else 0.0
            assert abs(w @ x ** p - want) <= 1e-9, (width, order, p)
        assert np.allclose(w, (-1) ** order * w[::-1], rtol=0, atol=1e-12 * np.abs(w).max())
