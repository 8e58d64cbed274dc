"""The float32 restatement of the spectral shape descriptors (tests/spectral_ref.py, include/jsg.h section 2l) against float64 on
signals with known answers: one-hot frames, flat spectra, a symmetric pair, the stated bounds on random non-negative planes, a tie in
the rolloff comparison built from small integers, and the all-zero, NaN and infinity rules.  CPU only."""
import math

import numpy as np
import pytest

import spectral_ref as sr
from spectral_ref import U

KS = (1, 2, 3, 31, 32, 33, 64, 65, 100, 129, 257, 1025)


@pytest.mark.parametrize("K", KS)
def test_one_hot_frames(K):
    """All the energy (a power of two, so every product and quotient is exact) in bin k0: the centroid is f[k0] to the bit, the spread
    +0, the rolloff bin k0 for any percentage, the crest K to two roundings."""
    k0s = sorted({0, K // 3, K // 2, K - 1})
    S = np.zeros((len(k0s), K), np.float32)
    S[np.arange(len(k0s)), k0s] = 4.0
    f = sr.freqs(K)
    for roll in (1.0, 0.85, 1e-30):
        got = sr.shape32(S, f, roll)
        assert sr.same(got["energy"], np.full(len(k0s), 4.0, np.float32))
        assert sr.same(got["centroid"], f[k0s])
        assert sr.same(got["spread"], np.zeros(len(k0s), np.float32))                  # +0, not -0
        assert np.array_equal(got["rolloff_bin"], np.array(k0s, np.int32)) and sr.same(got["rolloff"], f[k0s])
        assert (np.abs(got["crest"].astype(np.float64) - K) <= 2 * U * K).all()


@pytest.mark.parametrize("K,roll,bin_", [(100, 0.85, 84), (64, 0.5, 31), (1000, 0.85, 849), (33, 1.0, 32), (7, 0.3, 2), (1, 0.85, 0), (257, 0.5, 128)])
def test_flat_spectra(K, roll, bin_):
    """Every bin 3.0 (the sums are small integers times 3: exact): the centroid is the mean of f, the rolloff bin ceil(p K) - 1, and
    flatness_db is 0 up to the rounding of the K-term sum of jsg_exact_db(3) (E / K is exactly 3, so both logarithms are the same
    number): at most (n + 2) u |db(3)|, n = ceil(K / W) + log2 W."""
    assert bin_ == math.ceil(round(roll * K, 9)) - 1
    S = np.full((2, K), 3.0, np.float32)
    f = sr.freqs(K, 10.0)                           # integers: N1 is exact below 2^24
    got = sr.shape32(S, f, roll)
    assert sr.same(got["energy"], np.full(2, 3.0 * K, np.float32))
    assert (np.abs(got["centroid"].astype(np.float64) - f.astype(np.float64).mean()) <= sr.bounds(K)["centroid"] * f.mean() + 0).all()
    # (in float64 the float32 0.85 = 0.85000002 times 300 lies above 255; in float32 the product rounds to 255, the decimal's value)
    assert np.array_equal(got["rolloff_bin"], np.full(2, bin_, np.int32))
    W = sr.lanes(K)
    n = -(-K // W) + W.bit_length() - 1
    db3 = float(sr.exact_db(np.float32(3.0)))
    assert (np.abs(got["flatness_db"]) <= (n + 2) * U * abs(db3)).all()
    assert (np.abs(got["crest"].astype(np.float64) - 1.0) <= 2 * U).all()


def test_a_symmetric_pair():
    """Two equal bins a and b on an integer frequency grid: every step is exact, so the centroid is the midpoint and the spread half the
    distance, to the bit; the rolloff falls on a for p <= 1/2 and on b above."""
    for K, a, b in ((8, 1, 5), (65, 0, 64), (257, 63, 193), (1025, 100, 900)):
        S = np.zeros((1, K), np.float32)
        S[0, [a, b]] = 1.0
        f = sr.freqs(K, 10.0)
        got = sr.shape32(S, f, 0.5)
        assert got["centroid"][0] == 5.0 * (a + b) and got["spread"][0] == 5.0 * (b - a) and got["energy"][0] == 2.0
        assert got["rolloff_bin"][0] == a and got["crest"][0] == np.float32(1.0) / (np.float32(2.0) / np.float32(K))
        assert sr.shape32(S, f, 0.75)["rolloff_bin"][0] == b


@pytest.mark.parametrize("K", KS + (4097,))
def test_the_bounds_hold_on_random_planes(K):
    S = sr.planes(3, 20, K)
    f = sr.freqs(K)
    got, want, bound = sr.shape32(S, f), sr.shape64(S, f), sr.bounds(K)
    for name in ("energy", "N1", "centroid"):
        err = np.abs(got[name].astype(np.float64) - want[name])
        assert (err <= bound[name] * np.abs(want[name])).all(), (name, (err / np.maximum(np.abs(want[name]), 1e-300)).max() / bound[name])
    # the rolloff bin differs from float64's only where a cum value lies within rounding of the threshold
    differ = got["rolloff_bin"] != want["rolloff_bin"]
    assert differ.mean() <= 0.05


def test_a_tie_goes_to_the_lowest_bin():
    """Small integers, every sum exact: cum reaches thr exactly at bin 1 and stays there over a plateau of zeros."""
    S = np.array([[1, 1, 0, 0, 2, 0], [0, 0, 3, 0, 0, 3], [2, 0, 0, 0, 0, 2]], np.float32)
    f = np.array([50, 40, 30, 20, 10, 0], np.float32)              # descending: the bin is searched, not the frequency
    got = sr.shape32(S, f, 0.5)
    assert got["rolloff_bin"].tolist() == [1, 2, 0] and got["rolloff"].tolist() == [40.0, 30.0, 50.0]
    # the same across a chunk boundary: 64 ones, a plateau of zeros over bins 64..99, then 64 more
    S = np.zeros((1, 164), np.float32)
    S[0, :64] = 1
    S[0, 100:] = 1
    assert sr.shape32(S, sr.freqs(164), 0.5)["rolloff_bin"][0] == 63
    assert sr.shape32(S, sr.freqs(164), np.float32(65) / np.float32(128))["rolloff_bin"][0] == 100


def test_all_zero_nan_and_infinity():
    K = 70
    S = np.array(sr.planes(1, 6, K)[0])
    f = sr.freqs(K)
    clean = sr.shape32(S, f)
    S[2] = 0
    got = sr.shape32(S, f)
    for name in ("centroid", "spread", "crest", "energy"):
        assert got[name][2] == 0 and not np.signbit(got[name][2])
    assert got["rolloff_bin"][2] == 0 and got["rolloff"][2] == f[0]
    # flatness_db of silence: the mean of K equal logarithms minus that logarithm
    assert abs(got["flatness_db"][2]) <= (2 + 6 + 2) * U * 110.0
    for k0 in (0, K // 2, K - 1):
        T = np.array(S)
        T[4, k0] = np.nan
        got = sr.shape32(T, f)
        for name in sr.FLOATS:
            assert np.isnan(got[name][4]), (name, k0)
        assert got["rolloff_bin"][4] == -1
        rest = [0, 1, 3, 5]
        assert not sr.same_outputs({n: v[rest] for n, v in got.items()}, {n: v[rest] for n, v in clean.items()})
    T = np.array(S)
    T[1, 9] = np.inf
    got = sr.shape32(T, f)
    assert np.isposinf(got["energy"][1]) and np.isnan(got["centroid"][1]) and got["rolloff_bin"][1] == 9 and got["rolloff"][1] == f[9]
    assert np.isnan(got["crest"][1]) and np.isnan(got["flatness_db"][1])          # inf / inf, inf - inf
    assert not sr.same_outputs({n: v[[0, 3]] for n, v in got.items()}, {n: v[[0, 3]] for n, v in clean.items()})


def test_the_plan_table():
    assert sr.plan(1) == ("spectral_regs1", 1, 8) and sr.plan(33) == ("spectral_regs1", 64, 8) and sr.plan(20) == ("spectral_regs1", 32, 8)
    assert [sr.plan(n // 2 + 1)[0] for n in (512, 1024, 2048, 4096, 8192)] == ["spectral_regs9", "spectral_regs9", "spectral_regs17", "spectral_regs33", "spectral_regs65"]
    assert sr.plan(4160)[0] == "spectral_regs65" and sr.plan(4161) == ("spectral_stream", 64, 1) and sr.plan(128)[0] == "spectral_regs2"
