"""tests/peak_ref.py, the restatement of include/jsgx.h section 14 that the GPU results are compared with: the vectorised candidates
against the frame-by-frame loop of the header, the known answers the header lists, the blocked decomposition of the wait rule (the
tables, the carry, the i-th pick) against the serial rule, and back() against a serial search.  CPU only."""
import numpy as np
import pytest

import peak_ref as pr

f32 = np.float32


def test_vectorised_candidates_equal_the_serial_loop():
    rng = np.random.default_rng(1)
    share = []
    for trial in range(3000):
        T = int(rng.integers(1, 80))
        x = rng.integers(0, 4, T).astype(f32) if trial % 3 else rng.standard_normal(T).astype(f32)
        reaches = [int(v) for v in rng.integers(0, 7, 4)]
        delta = float(rng.choice([-0.1, 0.0, 0.07, 0.3]))
        normalise = bool(trial & 1)
        a, b = pr.candidates(x, *reaches, delta, normalise), pr.candidates_serial(x, *reaches, delta, normalise)
        assert (a == b).all(), (trial, x, reaches, delta, normalise)
        share.append(a.mean())
    assert 0.1 < np.mean(share) < 0.9
    # reaches beyond the row, and the largest
    x = pr.quantised(300, 5)[0]
    for reaches in ((256, 256, 256, 256), (0, 256, 256, 0), (300, 0, 0, 300)):
        assert (pr.candidates(x, *reaches, 0.0, True) == pr.candidates_serial(x, *reaches, 0.0, True)).all()


def test_a_row_with_a_nan_or_an_infinity_is_refused():
    x = pr.quantised(50, 2)[0]
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[17] = bad
        assert pr.candidates(y, 1, 1, 2, 2, 0.0, True) is None and pr.peak_pick32(y, 1, 1, 2, 2, 0.0, 1)[0] == -1
        assert pr.peak_pick32(x, 1, 1, 2, 2, 0.0, 1, energy=y)[0] == -1 and pr.peak_pick32(x, 1, 1, 2, 2, 0.0, 1, energy=x)[0] >= 0


@pytest.mark.parametrize("T", [1, 5, 37, 64, 100])
@pytest.mark.parametrize("w", [0, 1, 4, 36, 37, 1000])
def test_known_answer_zero_row(T, w):
    for normalise in (False, True):
        for delta in (0.0, -0.1):
            n, peaks, _, c = pr.peak_pick32(np.zeros(T), 2, 1, 3, 3, delta, w, normalise)
            assert c.all() and peaks == list(range(0, T, w + 1)) and n == -(-T // (w + 1))
        assert pr.peak_pick32(np.zeros(T), 2, 1, 3, 3, 0.07, w, normalise)[0] == 0
    assert pr.peak_pick32(np.full(T, 3.5), 2, 1, 3, 3, 0.07, w, True)[0] == 0          # a constant row, normalised: y = +0


@pytest.mark.parametrize("wait", [0, 1, 2, 4, 5, 6, 11, 12])
def test_known_answer_impulse_train(wait):
    for T in (64, 65, 301):
        n, peaks, _, c = pr.peak_pick32(pr.impulses(T), 1, 1, 2, 2, 0.07, wait, True)
        assert list(np.flatnonzero(c)) == list(range(0, T, 6))
        assert peaks == list(range(0, T, 6 * -(-(wait + 1) // 6))) and n == len(peaks)
    five, six = (pr.peak_pick32(pr.impulses(64), 1, 1, 2, 2, 0.07, w, True)[1] for w in (5, 6))
    assert five[:3] == [0, 6, 12] and six[:3] == [0, 12, 24]          # the off-by-one of the rule


def test_known_answer_one_frame():
    for v in (0.0, 1.0, -2.5, 1e30, 3.0e7):
        for delta in (-0.1, 0.0, 0.07, 1.0):
            assert pr.peak_pick32([v], 3, 1, 5, 5, delta, 0, True)[0] == int(0 >= delta)
            assert pr.peak_pick32([v], 3, 1, 5, 5, delta, 0, False)[0] == int(f32(v) >= f32(f32(v) + f32(delta)))
    assert pr.peak_pick32([3.0e7], 0, 0, 0, 0, 1.0, 0, False)[0] == 1 and pr.peak_pick32([2.0 ** 30], 0, 0, 0, 0, 1.0, 0, False)[0] == 1          # delta absorbed
    assert pr.peak_pick32([1.0], 0, 0, 0, 0, 0.07, 0, True, energy=[5.0])[2] == []


@pytest.mark.parametrize("B", [1, 4, 7, 16])
def test_blocked_decomposition_equals_the_serial_rule(B):
    rng = np.random.default_rng(B)
    for trial in range(800):
        T = int(rng.integers(1, 90))
        c = rng.random(T) < rng.choice([0.05, 0.3, 0.9, 1.0])
        wait = int(rng.choice([0, 1, 2, 3, 5, B - 1, B, B + 1, 2 * B + 3, 3 * B, 5 * B + 1, T, 1 << 24]))
        assert pr.blocked(c, wait, B) == pr.greedy(c, wait), (trial, T, wait, c)


def test_blocked_decomposition_at_the_block_of_the_library():
    B = pr.BLOCK
    for seed, wait in enumerate((0, 1, 3, 30, B - 1, B, B + 1, 2 * B + 3)):
        x = pr.quantised(3 * B + 7, seed)[0]
        c = pr.candidates(x, 3, 1, 5, 5, 0.07, True)
        assert 0.2 < c.mean() < 0.5          # about a third of the frames
        assert pr.blocked(c, wait, B) == pr.greedy(c, wait)
    c = pr.candidates(pr.smooth(4000, 1)[0], 3, 1, 5, 5, 0.07, True)
    assert 1 / 40 < c.mean() < 1 / 10          # about one frame in twenty


def test_back_equals_a_serial_search():
    rng = np.random.default_rng(3)
    for trial in range(500):
        T = int(rng.integers(1, 60))
        e = rng.integers(0, 3, T).astype(f32) if trial % 2 else rng.standard_normal(T).astype(f32)
        peaks = sorted(int(p) for p in rng.integers(0, T, int(rng.integers(0, 10))))
        got = pr.back(peaks, e)
        assert got == pr.back_serial(peaks, e) and got == sorted(got) and all(b <= p for b, p in zip(got, peaks))
    m = pr.minima(np.array([3, 1, 1, 2, 0, 0, 0], f32))
    assert list(m) == [True, False, True, False, False, False, False]          # the right end of a flat run; frame T-1 never is; frame 0 always
    assert list(pr.minima(np.array([1.0], f32))) == [True] and list(pr.minima(np.array([2.0, 1.0], f32))) == [True, False]
    assert pr.back([1, 2, 3, 3, 6], np.array([3, 1, 1, 2, 0, 0, 0], f32)) == [0, 2, 2, 2, 2]          # duplicates are kept


def test_max_peaks_keeps_the_earliest():
    x = pr.quantised(200, 4)[0]
    n, peaks, b, _ = pr.peak_pick32(x, 3, 1, 5, 5, 0.07, 3, True, energy=x)
    assert n > 6
    n2, cut, cut_b, _ = pr.peak_pick32(x, 3, 1, 5, 5, 0.07, 3, True, energy=x, max_peaks=5)
    assert n2 == n and cut == peaks[:5] and cut_b == b[:5]


def test_the_shape_list():
    assert {s[0] for s in pr.SHAPES} == set(pr.ROWS_SET) and {s[1] for s in pr.SHAPES} == set(pr.T_SET)
    for corner in ((pr.ROWS_SET[0], pr.T_SET[0]), (pr.ROWS_SET[1], pr.T_SET[0]), (pr.ROWS_SET[0], pr.T_SET[-1]), (pr.ROWS_SET[1], pr.T_SET[-1])):
        assert corner in pr.SHAPES
