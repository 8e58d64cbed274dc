"""tests/rhythm_ref.py checked on the CPU: the float32 restatements against the float64 definitions under the cap, the float64
autocorrelation against numpy.correlate, the onset definition on hand-made planes, and the tempo of the decided impulse trains."""
import numpy as np
import pytest

import rhythm_ref as rr


def test_fma32_is_exact_on_cases_that_round_twice():
    a = np.array([1.0 + 2.0 ** -12, 3.0, 1e-20, -1.0], np.float32)
    b = np.array([1.0 + 2.0 ** -12, 1.0 / 3.0, 1e-20, 1.0], np.float32)
    c = np.array([2.0 ** -24, -1.0, 1.0, 1.0], np.float32)
    got = rr.fma32(a, b, c)
    from fractions import Fraction
    for i in range(4):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = np.float32(float(exact))          # float(Fraction) rounds once to float64; these cases are far from a float32 tie there
        assert got[i] == near, i


@pytest.mark.parametrize("Wn,lags,hop", [(2, 2, 1), (8, 4, 3), (64, 64, 1), (65, 32, 65), (384, 384, 7)])
@pytest.mark.parametrize("normalise", [0, 1])
def test_restatement_stays_within_the_cap(Wn, lags, hop, normalise):
    o = rr.envelopes()[:, :3 * Wn]
    n = rr.frames(o.shape[1], hop)
    ref = rr.tempogram(o, rr.hann(Wn), lags, hop, n, normalise)
    assert ref["tg32"].dtype == np.float32 and ref["tg32"].shape == (5, n, lags)
    assert (np.abs(ref["tg32"].astype(np.float64) - ref["tg64"]) <= ref["cap"]).all(), rr.cap_units(ref["tg32"], ref)
    assert (ref["tg32"][3] == 0).all() and not np.signbit(ref["tg32"][3]).any()        # silence: +0 everywhere
    if normalise:
        live = ref["tg64"][..., 0] != 0
        assert (ref["tg32"][..., 0][live] == 1).all()


def test_float64_autocorrelation_is_numpy_correlate():
    Wn = 50
    o = rr.envelopes()[1, :120]
    w = rr.hann(Wn)
    n = rr.frames(120, 10)
    y = rr.windowed(o, w, 10, n)
    A, _ = rr.autocorr64(y, Wn)
    for i in (0, 3, n - 1):
        full = np.correlate(y[0, i].astype(np.float64), y[0, i].astype(np.float64), mode="full")
        assert np.allclose(A[0, i], full[Wn - 1:], rtol=1e-13, atol=1e-300)
    # frame 0 is centred on sample 0: its first Wn / 2 samples lie before the row and are +0, the others are products
    assert (y[0, 0, :Wn // 2] == 0).all() and np.array_equal(y[0, 0, Wn // 2:], o[:Wn - Wn // 2] * w[Wn // 2:])


def test_onset_definition_on_hand_made_planes():
    # a step in every band at frame 3
    S = np.zeros((6, 4), np.float32)
    S[3:] = 2.0
    assert np.array_equal(rr.onset64(S), [0, 0, 0, 2, 0, 0]) and np.array_equal(rr.onset32(S), np.float32([0, 0, 0, 2, 0, 0]))
    assert np.array_equal(rr.onset64(S, lag=2), [0, 0, 0, 2, 2, 0])
    # t < lag is +0 and a lag past the plane gives all zeros
    assert np.array_equal(rr.onset64(S, lag=6), np.zeros(6)) and np.array_equal(rr.onset32(S, lag=7), np.zeros(6, np.float32))
    # the maximum filter is clipped at both band edges: m = 3 covers b - 1 .. b + 1, m = 4 covers b - 2 .. b + 1
    prev = np.float32([5, 0, 0, 0, 9])
    S = np.stack([prev, np.float32([6, 6, 6, 6, 10])])
    assert np.array_equal(rr.onset64(S, m=1)[1] * 5, 1 + 6 + 6 + 6 + 1)
    assert np.array_equal(rr.onset64(S, m=3)[1] * 5, 1 + 1 + 6 + 0 + 1)             # ref = 5 5 0 9 9
    assert np.array_equal(rr.onset64(S, m=4)[1] * 5, 1 + 1 + 1 + 0 + 1)             # ref = 5 5 5 9 9
    assert np.array_equal(rr.onset32(S, m=4)[1], np.float32(4) / np.float32(5))
    # a decrease contributes nothing, a NaN goes through to exactly the frames t and t + lag
    S = np.array(rr.planes()[0, :10, :5])
    S[4, 2] = np.nan
    for lag in (1, 3):
        for o in (rr.onset64(S, lag=lag, m=3), rr.onset32(S, lag=lag, m=3)):
            assert np.array_equal(np.flatnonzero(np.isnan(o)), [4, 4 + lag])


@pytest.mark.parametrize("B", [1, 2, 33, 64, 65, 200])
def test_onset_restatement_against_float64(B):
    S = rr.planes()[:, :, :B]
    for lag, m in ((1, 1), (2, 3), (3, 4)):
        o64, o32 = rr.onset64(S, lag, m), rr.onset32(S, lag, m)
        # every term is non-negative: (B / W + log2 W + 2) roundings at most
        assert (np.abs(o32 - o64) <= (B / 64 + 9) * rr.U * o64).all()


@pytest.mark.parametrize("Wn,T,period,margin", rr.DECIDED)
def test_tempo_of_the_decided_impulse_trains(Wn, T, period, margin):
    o = rr.impulse_train(T, period)
    ref = rr.tempogram(o, rr.hann(Wn), Wn, 1, T, 1)
    prior = rr.prior64(Wn)
    lag, bpm, got, _ = rr.tempo64(ref["tg64"][0], prior)
    assert lag == period and bpm == 60.0 * rr.FRAME_RATE / period
    assert got >= 1.5 and abs(got / margin - 1) <= 0.06, got            # decided, and the margin of the table
    lag32, bpm32, g32 = rr.tempo32(ref["tg32"][0], prior.astype(np.float32))
    assert lag32 == period and bpm32 == np.float32(np.float32(60.0) * np.float32(rr.FRAME_RATE)) / np.float32(period)
    assert np.abs(g32 - ref["tg64"][0].mean(axis=0)).max() <= 1e-4


def test_tempo_ties_and_nan():
    prior = np.float32([0, 1, 1, 1, 0.5])
    tg = np.zeros((70, 5), np.float32)
    tg[:, 2] = tg[:, 3] = 0.25
    assert rr.tempo32(tg, prior)[0] == 2                                 # the lowest lag on a tie
    tg[69, 0] = np.nan
    assert rr.tempo32(tg, prior)[0] == 2                                 # lag 0 is not looked at
    tg[5, 4] = np.nan
    lag, bpm, g = rr.tempo32(tg, prior)
    assert lag == -1 and np.isnan(bpm) and np.isnan(g[4]) and g[2] == np.float32(0.25)
