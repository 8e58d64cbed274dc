"""tests/yin_ref.py checked on the CPU: the float32 restatement against the float64 evaluation under cap (b), its lags on decided
frames, how many frames are decided, the pitch of the tone and of the pulse train, silence, the exact fused multiply-add, and the
selection rule on hand-made d' vectors."""
import numpy as np
import pytest

import yin_ref as yr

T = yr.frames(yr.L, yr.W, yr.TAU_MAX, yr.HOP)


def test_shapes():
    assert T == 40 and yr.signals().shape == (6, yr.L) and yr.shared()["dp64"].shape == (6, T, yr.TAU_MAX + 1)
    assert yr.frames(455, 256, 200, 64) == 0 and yr.frames(456, 256, 200, 64) == 1 and yr.frames(519, 256, 200, 64) == 1 and yr.frames(520, 256, 200, 64) == 2
    assert yr.order(5) == [0, 1, 2, 3, 4] and yr.order(130)[:6] == [0, 64, 128, 1, 65, 129] and sorted(yr.order(1000)) == list(range(1000))
    assert yr.order(1000)[:9] == [0, 64, 128, 192, 256, 320, 384, 448, 1] and yr.order(1000)[512:515] == [512, 576, 640]


def test_restatement_under_the_cap_and_on_the_float64_lag():
    ref = yr.shared()
    units = yr.cap_units(ref["dp32"], ref)
    print("restatement error in units of cap (b):", dict(zip(yr.NAMES, units)))
    assert (np.abs(ref["dp32"].astype(np.float64) - ref["dp64"]) <= ref["cap"]).all()
    ok = ref["decided"]
    assert (ref["tau32"][ok] == ref["tau64"][ok]).all()
    rel = np.abs(ref["f032"][ok].astype(np.float64) - ref["f064"][ok]) / ref["f064"][ok]
    print("restatement f0 error on decided frames, relative:", rel.max())
    assert rel.max() <= 1e-4


def test_most_frames_are_decided():
    ref = yr.shared()
    for name in yr.MOSTLY_DECIDED:
        undecided = int((~ref["decided"][yr.NAMES.index(name)]).sum())
        print(name, "undecided frames:", undecided, "of", T)
        assert undecided <= T // 10, name


def test_pitch_of_the_tone_and_the_pulse_train():
    ref = yr.shared()
    tone, pulses = ref["f064"][yr.NAMES.index("tone")], ref["f064"][yr.NAMES.index("pulses")]
    assert (np.abs(tone / 220.0 - 1.0) <= 0.005).all() and (np.abs(pulses / (yr.SR / yr.PULSE_PERIOD) - 1.0) <= 0.005).all()
    i = yr.NAMES.index("tone")
    assert (ref["aper64"][i] < yr.THRESHOLD).all() and (ref["aper64"][yr.NAMES.index("noise")] > yr.THRESHOLD).all()
    late = ref["f064"][yr.NAMES.index("onset")][-10:]
    assert (np.abs(late / 330.0 - 1.0) <= 0.005).all()


def test_silence():
    ref = yr.shared()
    i = yr.NAMES.index("silence")
    for tag, ft in (("64", np.float64), ("32", np.float32)):
        assert (ref["dp" + tag][i] == 1).all() and (ref["tau" + tag][i] == yr.TAU_MIN).all()
        assert (ref["f0" + tag][i] == ft(np.float32(yr.SR)) / ft(yr.TAU_MIN)).all() and (ref["aper" + tag][i] == 1).all()
    # the frames of the onset signal that lie before the onset are silent too
    j = yr.NAMES.index("onset")
    quiet = np.arange(T) * yr.HOP + yr.W + yr.TAU_MAX <= 1500
    assert quiet.sum() >= 10 and (ref["dp32"][j][quiet] == 1).all() and (ref["f032"][j][quiet] == np.float32(1000)).all()


def test_fma_square_is_exact():
    rng = np.random.default_rng(3)
    e = (rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000)).astype(np.float32)
    acc = np.abs(rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000)).astype(np.float32)
    got = yr.fma_square(e, acc)
    want = np.array([np.float32(np.longdouble(a) + np.longdouble(v) * np.longdouble(v)) for v, a in zip(e, acc)])       # 64-bit mantissa: exact, rounded once
    if np.finfo(np.longdouble).nmant >= 63:
        assert np.array_equal(got, want)
    # a tie that a float64 sum rounded to nearest gets wrong: 1 + 2^-24 + 2^-60 lies above the midpoint
    one, tiny = np.float32(1), np.float32(2.0 ** -12)
    assert yr.fma_square(np.array([tiny]), np.array([one]))[0] == np.float32(1)                                          # exactly the midpoint: to even
    e2 = np.array([np.float32(2.0 ** -12 * (1 + 2.0 ** -23))])
    assert yr.fma_square(e2, np.array([one]))[0] == np.float32(1 + 2.0 ** -23)


def dp_of(values, dtype=np.float32):
    return np.array(values, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_selection_rule(dtype):
    sel = lambda v, lo, hi, thr=0.1: yr.select(dp_of(v, dtype), lo, hi, thr, 100.0)
    # a dip below the threshold, walked to its bottom, though a deeper one follows further on
    v = [1, 1, 0.5, 0.09, 0.05, 0.07, 0.5, 0.01, 0.5]
    tau, s, f0, aper = sel(v, 2, 8)
    assert tau == 4 and aper == dtype(0.05)
    a, b, c = dtype(0.09), dtype(0.05), dtype(0.07)
    want = (dtype(0.5) * (a - c)) / ((a - b) + (c - b))
    assert s == want and f0 == dtype(100.0) / (dtype(4) + want) and type(f0) is dtype
    # the threshold is strict (0.25 is not below 0.25)
    assert sel([1, 1, 0.5, 0.25, 0.5, 0.125, 0.5], 1, 6, 0.25)[0] == 5
    # a walk that ends at tau_max: no parabola there
    tau, s, f0, aper = sel([1, 1, 0.5, 0.09, 0.05, 0.04], 1, 5)
    assert tau == 5 and s == 0 and f0 == dtype(20) and aper == dtype(0.04)
    # nothing below the threshold: the minimum, the lowest lag on ties; lags below tau_min do not count
    tau, s, f0, aper = sel([1, 0.9, 0.5, 0.7, 0.5, 0.8], 1, 5)
    assert tau == 2 and aper == dtype(0.5)
    assert sel([1, 0.2, 0.9, 0.5, 0.7, 0.5, 0.8], 2, 6)[0] == 3
    # tau_min == tau_max
    tau, s, f0, aper = sel([1, 0.5, 0.01, 0.5], 3, 3)
    assert tau == 3 and s == 0 and f0 == dtype(100.0) / dtype(3) and aper == dtype(0.5)
    # den == 0 (a flat triple) and den < 0 (the first lag below the threshold is a local maximum and no step follows)
    tau, s, _, _ = sel([1, 0.5, 0.05, 0.05, 0.05, 0.5], 3, 5)
    assert tau == 3 and s == 0
    tau, s, f0, _ = sel([1, 0.5, 0.75, 0.75, 0.25], 2, 3, 0.875)
    assert tau == 2 and s == 0 and f0 == dtype(50)
    # |s| > 1 is dropped: the fallback lands on the edge of the range with a lower value below tau_min
    out = dp_of([1, 0.2, 0.5, 0.9, 0.95], dtype)
    tau, s, f0, _ = yr.select(out, 2, 4, 0.1, 100.0)
    a, b, c = out[1], out[2], out[3]
    assert tau == 2 and (a - b) + (c - b) > 0 and abs((dtype(0.5) * (a - c)) / ((a - b) + (c - b))) > 1 and s == 0 and f0 == dtype(50)
    # a NaN inside the range makes the frame NaN; one outside does not
    nan = dp_of([1, np.nan, 0.5, 0.05, 0.5], dtype)
    assert yr.select(nan, 2, 4, 0.1, 100.0)[0] == 3 and np.isfinite(yr.select(nan, 2, 4, 0.1, 100.0)[2])
    assert np.isnan(yr.select(nan, 1, 4, 0.1, 100.0)[2]) and np.isnan(yr.select(nan, 1, 4, 0.1, 100.0)[3])


def test_decided_is_a_property_of_the_gaps():
    w = 256
    dp = np.array([1, 1, 0.5, 0.09, 0.05, 0.07, 0.5, 0.01, 0.5])
    assert yr.decided(dp, yr.cap(dp, w), 2, 8, 0.1)
    close = dp.copy()
    close[3] = 0.1 - 1e-7                       # within its cap of the threshold
    assert not yr.decided(close, yr.cap(close, w), 2, 8, 0.1)
    flat = dp.copy()
    flat[5] = 0.05 + 1e-7                       # the end of the walk hangs on less than the cap
    assert not yr.decided(flat, yr.cap(flat, w), 2, 8, 0.1)
    high = np.array([1, 0.9, 0.5, 0.7, 0.5 + 1e-7, 0.8])
    assert not yr.decided(high, yr.cap(high, w), 1, 5, 0.1)
    high[4] = 0.6
    assert yr.decided(high, yr.cap(high, w), 1, 5, 0.1)
