"""The float32 restatement of harmonic-percussive separation (tests/hpss_ref.py) against librosa's definition in float64, its medians
against scipy, and the properties of the masks.  CPU only: the GPU tests compare the library with this restatement bit for bit."""
import numpy as np
import pytest
import scipy.ndimage

import hpss_ref as hr

GEOMS = [(96, 257, 31, 31), (70, 65, 63, 63), (5, 3, 31, 63), (67, 129, 3, 5), (200, 130, 17, 9)]


@pytest.mark.parametrize("g", GEOMS, ids=hr.geometry_id)
@pytest.mark.parametrize("margins", [(1.0, 1.0), (2.0, 1.0), (1.0, 3.5)], ids=str)
def test_mirror_masks_stay_within_4u_of_float64(g, margins):
    """Power carries 2u, g*C 2u more and the sum u, so a mask moves by at most M(1-M) 6u <= 1.5u; one u for the sum and u/2 for the
    divide bring it to about 3u.  The bound is 4u."""
    T, K, W_t, W_f = g
    X = hr.make_input(T, K)
    M_h, M_p = hr.mirror(X, W_t, W_f, *margins)[:2]
    R_h, R_p = hr.reference64(X, W_t, W_f, *margins)
    e = max(np.abs(M_h.astype(np.float64) - R_h).max(), np.abs(M_p.astype(np.float64) - R_p).max())
    print(f"{hr.geometry_id(g)} margins {margins}: worst mask error {e / hr.U:.3f} u")
    assert e <= 4 * hr.U


@pytest.mark.parametrize("g", hr.GEOMETRIES, ids=hr.geometry_id)
def test_mirror_medians_equal_scipy(g):
    """scipy.ndimage.median_filter(mode="reflect") where the half window is at most the axis length (scipy reflects once)."""
    T, K, W_t, W_f = g
    P = hr.power(hr.make_input(T, K))
    H, C = hr.mirror(P, W_t, W_f)[4:]
    if (W_t - 1) // 2 <= T:
        assert np.array_equal(H, scipy.ndimage.median_filter(P, size=(W_t, 1), mode="reflect"))
    if (W_f - 1) // 2 <= K:
        assert np.array_equal(C, scipy.ndimage.median_filter(P, size=(1, W_f), mode="reflect"))


def test_refl_is_the_definition():
    assert hr.refl(np.arange(-9, 12), 4).tolist() == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3]
    assert hr.refl(np.arange(-3, 4), 1).tolist() == [0] * 7
    for L in (1, 2, 3, 5, 64):       # the symmetric extension, period 2L
        ext = np.concatenate([np.arange(L), np.arange(L)[::-1]])
        i = np.arange(-4 * L - 3, 4 * L + 3)
        assert np.array_equal(hr.refl(i, L), ext[np.mod(i, 2 * L)])


@pytest.mark.parametrize("g", GEOMS, ids=hr.geometry_id)
def test_masks_sum_to_one_at_margin_one(g):
    T, K, W_t, W_f = g
    for X, has_zero_windows in ((hr.make_input(T, K), False), (hr.tie_input(T, K), True)):
        M_h, M_p, _, _, H, C = hr.mirror(X, W_t, W_f)
        live = (H + C) > 0
        assert (np.abs(M_h.astype(np.float64) + M_p.astype(np.float64) - 1.0)[live] <= 2.0 ** -23).all()
        assert (M_h[~live] == 0).all() and (M_p[~live] == 0).all()
        assert (~live).any() == has_zero_windows          # the tie input's zero block holds windows whose medians are both zero


@pytest.mark.parametrize("W_t,W_f", [(31, 31), (1, 3), (63, 5), (3, 63)])
def test_a_horizontal_line_is_harmonic(W_t, W_f):
    """One bin constant over all frames, everything else zero: M_h = 1 and M_p = 0 exactly on the line."""
    X = np.zeros((50, 40), np.complex64)
    X[:, 17] = 3.0 - 4.0j
    M_h, M_p, out_h, out_p = hr.mirror(X, W_t, W_f)[:4]
    assert (M_h[:, 17] == 1).all() and (M_p[:, 17] == 0).all()
    assert np.array_equal(out_h, X) and (out_p == 0).all()


@pytest.mark.parametrize("W_t,W_f", [(31, 31), (3, 1), (63, 5), (3, 63)])
def test_a_vertical_line_is_percussive(W_t, W_f):
    """One frame constant over all bins, everything else zero: M_p = 1 and M_h = 0 exactly on the line."""
    X = np.zeros((50, 40), np.complex64)
    X[23, :] = -0.5 + 2.0j
    M_h, M_p, out_h, out_p = hr.mirror(X, W_t, W_f)[:4]
    assert (M_p[23, :] == 1).all() and (M_h[23, :] == 0).all()
    assert np.array_equal(out_p, X) and (out_h == 0).all()


def test_real_power_input_gives_the_same_masks():
    X = hr.make_input(67, 129)
    c = hr.mirror(X, 17, 9, 2.0, 1.0)
    r = hr.mirror(hr.power(X), 17, 9, 2.0, 1.0)
    assert np.array_equal(c[0], r[0]) and np.array_equal(c[1], r[1])
    assert np.array_equal(r[2], r[0] * hr.power(X)) and r[2].dtype == np.float32
