"""The float32 restatement of the beat tracker (tests/beat_ref.py, include/jsgx.h section 1) against the plain float64 version on known
answers, the stated tie rules, the first-beat rule, the end rule, and the bound of the exp routine.  CPU only, numpy only."""
import numpy as np
import pytest

import beat_ref as br

PERIODS = (4, 7, 16, 33, 100)


@pytest.mark.parametrize("smooth,normalise", [(False, False), (True, True)])
@pytest.mark.parametrize("P", PERIODS)
def test_impulse_train_gives_the_impulses(P, smooth, normalise):
    T = 8 * P + 1
    o = br.impulse_train(T, P)
    want = np.arange(0, T, P)
    got = br.beat32(o, P, smooth=smooth, normalise=normalise)
    assert got["n"] == want.size and (got["beats"] == want).all()
    assert (br.beat64(o, P, smooth=smooth, normalise=normalise) == want).all()


@pytest.mark.parametrize("P", PERIODS)
def test_a_missing_impulse_still_gets_its_beat(P):
    T = 8 * P + 1
    o = br.impulse_train(T, P, missing=(4,))
    assert o[4 * P] == 0 and o.sum() == 8
    want = np.arange(0, T, P)
    for smooth, normalise in ((False, False), (True, True)):
        assert (br.beat32(o, P, smooth=smooth, normalise=normalise)["beats"] == want).all()
        assert (br.beat64(o, P, smooth=smooth, normalise=normalise) == want).all()


@pytest.mark.parametrize("P,T", [(4, 30), (7, 7), (7, 3), (33, 100), (100, 401), (1, 5), (2, 9)])
def test_zero_and_constant_rows_follow_the_tie_rules(P, T):
    # all zero: every candidate is pen[tau] + 0, the largest is -0 + 0 = +0 at tau = P alone; C = +0; t0 = 0; e = max(0, T - P), the lowest t
    for normalise in (False, True):
        got = br.beat32(np.zeros(T, np.float32), P, smooth=True, normalise=normalise)
        e = max(0, T - P)
        want = np.arange(e % P, e + 1, P)
        assert (got["C"] == 0).all() and not np.signbit(got["C"]).any() and (got["s"] == 0).all()
        assert got["n"] == want.size and (got["beats"] == want).all()
    # a constant row without smoothing: sd = 0 (the lane sums of equal values 0.75 are exact here), so s = o; C never decreases, so the end is
    # the last frame unless C is flat over the last period, and the first link that leaves the row ends the chain
    got = br.beat32(np.full(T, 0.75, np.float32), P, smooth=False, normalise=True)
    assert (got["s"] == np.float32(0.75)).all() and (np.diff(got["C"]) >= 0).all()
    assert (got["C"][:(P + 1) // 2] == np.float32(0.75)).all()          # nothing to look back at: pen[P] + 0
    e0 = max(0, T - P)
    assert got["beats"][-1] == e0 + int(np.argmax(got["C"][e0:])) and got["beats"][0] < 2 * P
    assert (br.beat64(np.full(T, 0.75), P, smooth=False, normalise=True) == got["beats"]).all()


def test_first_beat_rule():
    # frames in front of the first one that reaches 1 % of the maximum link nowhere: t0 = 23, so the chain stops at 13 although 13 - P = 3 lies
    # in the row and holds a (quiet) impulse too; with 2 % at 13 instead t0 = 13 and the chain goes on to 3
    P, T = 10, 64
    o = np.zeros(T, np.float32)
    o[3] = o[13] = 0.005
    o[23::P] = 1.0
    got = br.beat32(o, P, smooth=False, normalise=False)
    assert (got["beats"] == np.arange(13, T, P)).all()
    assert (br.beat64(o, P, smooth=False, normalise=False) == got["beats"]).all()
    # ... and C is not changed by the rule: C[13] holds both quiet impulses
    assert got["C"][3] == np.float32(0.005) and got["C"][13] == np.float32(0.005) + np.float32(0.005)
    o[13] = 0.02
    assert (br.beat32(o, P, smooth=False, normalise=False)["beats"] == np.arange(3, T, P)).all()
    # a row that never reaches the threshold (max < 0: th = 0.01 max > every s): only the end frame is a beat
    neg = br.beat32(np.full(20, -1.0, np.float32), 5, smooth=False, normalise=False)
    assert neg["n"] == 1 and 15 <= neg["beats"][0] < 20


def test_end_rule():
    # the chain ends on the best C of the LAST period, the lowest t on ties: a louder beat earlier does not move the end
    P, T = 8, 70
    o = br.impulse_train(T, P).copy()
    o[16] = 5.0
    got = br.beat32(o, P, smooth=False, normalise=False)
    assert got["beats"][-1] == 64 and (got["beats"] == np.arange(0, T, P)).all()
    e0 = T - P
    assert got["C"][e0:].argmax() + e0 == 64
    # T <= P: the window is the whole row
    short = br.beat32(np.array([0, 0, 1, 0, 1], np.float32), 16, smooth=False, normalise=False)
    assert short["n"] == 1 and short["beats"][0] == 2


def test_restatement_agrees_with_float64_on_noisy_trains():
    rng = np.random.default_rng(5)
    for P in (7, 16, 33):
        T = 12 * P + 5
        o = (br.impulse_train(T, P, start=P // 2) + 0.05 * np.abs(rng.standard_normal(T))).astype(np.float32)
        got = br.beat32(o, P)["beats"]
        assert (got == br.beat64(o, P)).all()
        assert (np.diff(got) == P).all() and got[0] % P == P // 2


def test_bad_period_and_nan():
    o = np.ones(10, np.float32)
    assert br.beat32(o, 0)["n"] == -1 and br.beat32(o, -1)["n"] == -1 and br.beat32(o, 1025)["n"] == -1 and br.beat32(o, 1024)["n"] >= 1
    o[4] = np.nan
    assert br.beat32(o, 4)["n"] == -1


def test_forms():
    assert br.form(1) == (1, 64, 1) and br.form(2) == (1, 64, 1) and br.form(7) == (4, 64, 4) and br.form(47) == (24, 16, 16)
    assert br.form(510) == (255, 2, 128) and br.form(511) == (256, 1, 256) and br.form(1024) == (512, 1, 256)
    for P in range(1, 1025):
        a, G, F = br.form(P)
        assert 1 <= F <= a and F * G <= 256 and 2 * P + F <= 4096 - 256


def test_exp_routine_bound():
    """jsgx_exp against exp in double over every (P, k) with P <= 1024: the bound the header states (JSGX_EXP_REL_BOUND) where x >= -87; +0
    below, where exp(x) itself is below 1.7e-38."""
    worst, count, below, n_below = br.exp_accuracy()
    print(f"jsgx_exp: worst relative error {worst:.3e} over {count} points; {n_below} points below -87, the largest exp there {below:.3e}")
    assert count > 200000 and n_below > 200000
    assert worst <= br.EXP_REL_BOUND
    assert below < 1.7e-38
    assert br.exp32(np.float32([0.0]))[0] == 1.0 and br.exp32(np.float32([-87.0]))[0] > 0 and br.exp32(np.float32([-87.00001]))[0] == 0
