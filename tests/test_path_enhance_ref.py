"""The restatement of include/jsgx.h sections 10 and 11 (tests/path_enhance_ref.py) against scipy and against a transcription of librosa's
roll loops, and the filter-bank builder of libjsgx.so (Python's diagonal_filter and jsgx_diagonal_filter_build) against the scipy
construction that librosa.segment.path_enhance runs.  CPU only.

Six of these cases (test_exact_on_integers_with_dyadic_weights and test_lag_against_the_roll_loops) check the numpy restatement alone,
against scipy and the roll loops, and so pass without the library's new entry points: they are what makes the reference of the GPU tests
independent of the code under test.  Every other case needs the new names."""
import os

import numpy as np
import pytest
import scipy.ndimage

import path_enhance_ref as pr

SLOPES = 2.0 ** np.linspace(-1.0, 1.0, 7)          # librosa's defaults: max_ratio 2, min_ratio 1 / 2, seven filters


def hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1))


def scipy_filter(n, slope, zero_mean=False):
    """librosa.filters.diagonal_filter, written out."""
    win = np.diag(hann(n))
    if not np.isclose(slope, 1.0):
        win = scipy.ndimage.rotate(win, 45.0 - np.arctan(slope) * 180.0 / np.pi, order=5, prefilter=False)
    np.clip(win, 0, None, out=win)
    win /= win.sum()
    if zero_mean:
        win -= win.mean()
    return win


@pytest.fixture(scope="module")
def jsgmod(jsg):
    from jadespectrogram_amd import _build
    if not os.path.exists(jsg.capix.LIB_PATH):
        _build.build_lib()
    jsg.capix.lib()
    return jsg


@pytest.mark.parametrize("n", [3, 7, 31, 51])
def test_diagonal_filter_and_the_builder_against_scipy(jsgmod, n):
    """Shapes equal; every entry within 2^-40 of the table's largest (the restatement measured 3.4e-16; a wrong border rule is seven
    orders above the bound).  The builder's taps are the float32 of the same tables, row-major, zeros dropped."""
    jsg = jsgmod
    worst = 0.0
    tap_w, tap_at, first, ri, rj = jsg.path_enhance_filters(n)
    assert len(first) == 8 and first[0] == 0 and first[-1] == len(tap_w) == len(tap_at) and (np.diff(first) > 0).all()
    reach = [0, 0]
    for f, slope in enumerate(SLOPES):
        want = scipy_filter(n, slope)
        got = jsg.diagonal_filter("hann", n, slope=slope)
        assert got.shape == want.shape, (n, slope, got.shape, want.shape)
        err = np.abs(got - want).max() / want.max()
        print(f"n {n} slope {slope:.4f} shape {want.shape} max |diff| / max {err:.3e}")
        assert err <= 2.0 ** -40, (n, slope, err)
        worst = max(worst, err)
        # the builder: the same table as taps
        w32 = got.astype(np.float32)
        keep = (got != 0) & (np.abs(w32) >= np.finfo(np.float32).tiny)
        a, b = np.nonzero(keep)
        s = slice(first[f], first[f + 1])
        assert np.array_equal(tap_w[s], w32[a, b]) and np.array_equal(tap_at[s], pr.pack(got.shape[0] // 2 - a, got.shape[1] // 2 - b)), (n, slope)
        reach = [max(reach[0], int(np.abs(got.shape[0] // 2 - a).max())), max(reach[1], int(np.abs(got.shape[1] // 2 - b).max()))]
        # and against scipy's table directly: the taps lie where scipy's entries are not negligible, with its values
        dense = np.zeros(want.shape)
        dense[a, b] = tap_w[s]
        assert np.abs(dense - want).max() <= 2.0 ** -23 * want.max()
    assert [ri, rj] == reach
    # zero_mean: the dense table, against scipy
    zm = scipy_filter(n, SLOPES[1], zero_mean=True)
    got = jsg.diagonal_filter(hann(n), n, slope=SLOPES[1], zero_mean=True)
    assert got.shape == zm.shape and np.abs(got - zm).max() <= 2.0 ** -40 * np.abs(zm).max()
    print(f"n {n}: largest difference {worst:.3e} of the table's largest entry")


def test_the_builder_trims_and_refuses(jsgmod):
    jsg = jsgmod
    full = jsg.path_enhance_filters(31)
    cut = jsg.path_enhance_filters(31, drop_below=1e-3)
    assert len(cut[0]) < len(full[0]) and cut[3] <= full[3]
    di, dj = pr.unpack(full[1])
    for f in range(7):
        s = slice(full[2][f], full[2][f + 1])
        big = np.abs(full[0][s]) >= np.float64(1e-3) * np.float64(np.abs(full[0][s]).max())
        c = slice(cut[2][f], cut[2][f + 1])
        assert np.array_equal(cut[0][c], full[0][s][big]) and np.array_equal(cut[1][c], full[1][s][big])
    one = jsg.path_enhance_filters(7, n_filters=1, max_ratio=1.0, min_ratio=1.0)
    assert len(one[0]) == 5 and one[3] == one[4] == 2 and np.array_equal(one[1], pr.pack([2, 1, 0, -1, -2], [2, 1, 0, -1, -2]))       # hann's end samples are 0
    dense = jsg.path_enhance_filters(7, zero_mean=True)
    assert len(dense[0]) > 7 * 40
    for kw, text in ((dict(n=2), "n must be in 3..101"), (dict(n=102), "n must be in 3..101"), (dict(n=7, max_ratio=-1.0, min_ratio=1.0), "max_ratio must be finite and > 0"),
                     (dict(n=7, min_ratio=3.0), "min_ratio above max_ratio"), (dict(n=7, n_filters=33), "n_filters must be in 1..32"),
                     (dict(n=7, drop_below=1.0), r"drop_below must be in \[0, 1\)"), (dict(n=101, max_ratio=50.0), "the bank reaches further than 64")):
        with pytest.raises(jsg.JsgError, match=text):
            jsg.path_enhance_filters(**kw)
    # n = 101 at slope 2 is a 128 x 128 table, centre 64; its outermost rows and columns are zero, so the taps reach 63
    assert jsg.path_enhance_filters(101)[3:] == (63, 63) and jsg.diagonal_filter("hann", 101, slope=2.0).shape == (128, 128)


@pytest.mark.parametrize("n", [7, 31])
def test_the_chain_against_scipy_in_float64(jsgmod, n):
    """Non-negative plane and weights: every fmaf chain of T taps is within T u / (1 - T u) relative of the exact sum, u = 2^-24; scipy's
    float64 sum of the same float32 taps stands for the exact sum (its own error, T 2^-53, is nine orders below).  A weight near the
    smallest normal float32 times a cell below 1 is subnormal, where a rounding errs by up to 2^-149 absolutely: T 2^-149 is added."""
    tap_w, tap_at, first, ri, rj = jsgmod.path_enhance_filters(n)
    R = pr.affinity_plane(45, 52, n)
    got = pr.path_enhance32(R, tap_w, tap_at, first, ri, rj)
    want = pr.path_enhance64(R, tap_w, tap_at, first)
    T = int(np.diff(first).max())
    u = 2.0 ** -24
    bound = T * u / (1 - T * u)
    err = np.abs(got.astype(np.float64) - want)
    # the maximum of chains each within the bound of its exact sum is within the bound of the maximum of the exact sums
    assert (err <= bound * want * (1 + 2.0 ** -40) + T * 2.0 ** -149).all(), (float((err / np.maximum(want, 1e-300)).max()), bound)
    print(f"n {n}: largest relative difference {float((err[want > 0] / want[want > 0]).max()):.3e}, bound {bound:.3e}")


def test_exact_on_integers_with_dyadic_weights():
    rng = np.random.default_rng(5)
    R = pr.integer_plane(23, 29, 1)
    R[3, 4] = -2.0
    Ks = [rng.integers(-4, 5, (5, 4)) / 8.0, rng.integers(0, 3, (2, 7)) / 4.0, np.zeros((3, 3))]
    Ks[0][2, 2] = 0.5
    w, at, first = [], [], [0]
    for K in Ks:
        kw, ka = pr.taps_of_table(K)
        w.append(kw), at.append(ka), first.append(first[-1] + len(kw))
    w, at = np.concatenate(w), np.concatenate(at)
    assert first[-1] == first[-2]          # the all-zero table is a filter without taps: acc = +0
    for clip in (True, False):
        got = pr.path_enhance32(R, w, at, first, 3, 4, clip)
        accs = [scipy.ndimage.convolve(R.astype(np.float64), K, mode="constant") for K in Ks]
        want = np.maximum(np.maximum(accs[0], accs[1]), accs[2])
        want = np.clip(want, 0, None) if clip else want
        assert np.array_equal(got.astype(np.float64), want) and not np.signbit(got[got == 0]).any()
    # a tap beyond the reach is skipped: a reach of 1 keeps only the taps within it
    di, dj = pr.unpack(at)
    near = (np.abs(di) <= 1) & (np.abs(dj) <= 1)
    cum = np.concatenate([[0], np.cumsum(near)])
    assert pr.same_bits(pr.path_enhance32(R, w, at, first, 1, 1), pr.path_enhance32(R, w[near], at[near], cum[first], 1, 1))
    # np.maximum: a NaN wins and stays, also through the clip
    Rn = np.array(R)
    Rn[10, 10] = np.nan
    got = pr.path_enhance32(Rn, w, at, first, 3, 4)
    assert np.isnan(got[10, 10]) and 0 < np.isnan(got).sum() <= 5 * 4 + 2 * 7


def librosa_to_lag(rec, pad, axis):
    """librosa.segment.recurrence_to_lag for a dense array, transcribed."""
    axis = np.abs(axis)
    t = rec.shape[axis]
    if pad:
        padding = [(0, 0), (0, 0)]
        padding[1 - axis] = (0, t)
        lag = np.pad(rec, padding, mode="constant")
    else:
        lag = rec.copy()
    idx = [slice(None)] * 2
    for i in range(1, t):
        idx[axis] = i
        lag[tuple(idx)] = np.roll(lag[tuple(idx)], -i)
    return lag


def librosa_from_lag(lag, axis):
    axis = np.abs(axis)
    t = lag.shape[axis]
    rec = lag.copy()
    idx = [slice(None)] * 2
    for i in range(1, t):
        idx[axis] = i
        rec[tuple(idx)] = np.roll(rec[tuple(idx)], i)
    return rec[:t, :t]


@pytest.mark.parametrize("N", [1, 2, 5, 64, 65])
def test_lag_against_the_roll_loops(N):
    R = pr.distinct_plane(N, N, N)
    for pad in (False, True):
        for axis in (0, 1):
            lag = pr.to_lag(R, pad, axis)
            assert np.array_equal(lag, librosa_to_lag(R, pad, axis)) and (axis == 0 or np.array_equal(lag, librosa_to_lag(R, pad, -1)))
            back = pr.from_lag(lag, axis)
            assert np.array_equal(back, librosa_from_lag(lag, axis)) and pr.same_bits(back, R)
            L = 2 * N if pad else N
            assert lag.shape == ((L, N) if axis == 1 else (N, L)) and (np.sort(lag[lag != 0]) == np.sort(R.ravel())).all() and (lag == 0).sum() == (L - N) * N
