"""The restatement of Viterbi decoding (tests/viterbi_ref.py, include/jsgx.h section 4) against what does not share its code: brute-force
enumeration of all S^T paths in float64, the band form against the dense form, the header's error bound against float64, and the
header's known answers.  CPU only."""
import itertools

import numpy as np
import pytest

import viterbi_ref as vr

U = 2.0 ** -24


def brute_force(b, p0, A):
    """(the best total, the optimal path that is smallest when compared from its last state backwards) over all S^T paths, in float64."""
    T, S = b.shape
    b, p0, A = (x.astype(np.float64) for x in (b, p0, A))
    paths = np.array(list(itertools.product(range(S), repeat=T)), dtype=np.int64)        # [S^T][T]
    with np.errstate(invalid="ignore"):
        total = p0[paths[:, 0]] + b[0, paths[:, 0]]
        for t in range(1, T):
            total = total + A[paths[:, t - 1], paths[:, t]]
            total = total + b[t, paths[:, t]]
    best = total.max()
    optimal = paths[total == best]
    order = np.lexsort(tuple(optimal[:, t] for t in range(T)))      # the last key is the primary one: frame T-1 first, then backwards
    return best, optimal[order[0]]


def test_against_brute_force_on_eighths():
    """S in 1..4, T in 1..6 over 300 seeds: logp equal in every case; the path equal in every case whose optimum is finite (with an
    optimum of -inf every path is optimal and the tie rule's path is not the reversed-lexicographic least: psi is chosen among equal
    -inf, not among optimal prefixes)."""
    finite = 0
    for seed in range(300):
        S, T = 1 + seed % 4, 1 + (seed // 4) % 6
        b, p0, A = vr.inputs("eighths", T, S, 1000 + seed)
        V, psi, states, logp = vr.viterbi32(b, p0, A)
        best, path = brute_force(b, p0, A)
        assert float(logp) == best, (seed, S, T, logp, best)
        assert (psi[1:] >= 0).all() and (psi < S).all()
        if np.isfinite(best):
            finite += 1
            assert (states == path).all(), (seed, S, T, states, path)
    assert finite >= 150, finite


@pytest.mark.parametrize("kind", ["eighths", "floats"])
def test_band_form_equals_dense_form_on_the_bands_matrix(kind):
    """The band table against the same matrix in the dense form with -inf outside the band: V and logp bit for bit.  psi, and with it
    the states, are compared where the choice is among finite values: where every source of a destination is -inf the band form takes
    its own lowest source, max(0, j - W), and the dense form state 0, as the header's tie rule has it for each set of sources."""
    for seed, (S, W, T) in enumerate([(1, 0, 5), (5, 0, 9), (5, 4, 9), (9, 2, 30), (40, 64, 12), (33, 3, 25), (64, 7, 20)]):
        b, p0, band = vr.inputs(kind, T, S, 50 + seed, band_half=W)
        V, psi, states, logp = vr.viterbi32(b, p0, band, band_half=W)
        dense = vr.band_as_dense(band, W)
        Vd, psid, statesd, logpd = vr.viterbi32(b, p0, dense)
        assert vr.same_bits(V, Vd) and vr.same_bits(logp, logpd)
        chosen_finite = np.zeros(V.shape, bool)
        chosen_finite[1:] = np.isfinite(V[np.arange(T - 1)[:, None], psi[1:]] + dense[psi[1:], np.arange(S)[None, :]])      # w(i*)
        assert (psi[chosen_finite] == psid[chosen_finite]).all()
        if np.isfinite(logp):
            assert (states == statesd).all()
        if kind == "floats":
            assert np.isfinite(logp) and chosen_finite[1:].all()
        lo = np.maximum(0, np.arange(S) - W)
        assert (psi[1:] >= lo).all() and (psi[1:] <= np.minimum(S - 1, np.arange(S) + W)).all()


@pytest.mark.parametrize("T", [1, 2, 17, 256, 1024, 4096])
def test_error_bound_of_the_header(T):
    """Non-positive floats at S = 8: logp against the same recurrence in float64 is inside the relative (2T + 2) u that the header derives
    (2T - 1 roundings, the second-order part below 3 u up to T = 4096)."""
    S = 8
    for seed in range(4):
        b, p0, A = vr.inputs("floats", T, S, 7000 + 10 * seed + T)
        logp = float(vr.viterbi32(b, p0, A)[3])
        V = p0.astype(np.float64) + b[0].astype(np.float64)
        A64 = A.astype(np.float64)
        for t in range(1, T):
            V = (V[:, None] + A64).max(axis=0) + b[t].astype(np.float64)
        exact = V.max()
        err = abs(logp - exact) / abs(exact)
        print(f"T={T} seed={seed} relative error {err / U:.3f} u, bound {2 * T + 2} u")
        assert err <= (2 * T + 2) * U, (T, seed, err / U)


def test_known_answers():
    z = lambda *shape: np.zeros(shape, np.float32)
    # all-zero inputs: states all 0, logp +0, V +0 everywhere
    for S, T, W in ((1, 1, None), (5, 7, None), (6, 9, 2), (4, 3, 64)):
        V, psi, states, logp = vr.viterbi32(z(T, S), z(S), z(S, S) if W is None else z(2 * W + 1, S), band_half=W)
        assert (states == 0).all() and logp.view(np.uint32) == 0 and (V.view(np.uint32) == 0).all()
        assert (psi[1:] == (0 if W is None else np.maximum(0, np.arange(S) - W))).all()
    # a band with W = 0 and a finite diagonal keeps the states constant at the end state
    b, p0, band = vr.inputs("floats", 40, 9, 3, band_half=0)
    V, psi, states, logp = vr.viterbi32(b, p0, band, band_half=0)
    totals = p0 + b.astype(np.float64).sum(axis=0) + 39 * band[0].astype(np.float64)
    assert (states == states[-1]).all() and states[-1] == int(np.argmax(totals)) and np.isfinite(logp)
    # an all -inf frame: logp = -inf, and the path as the tie rule has it (dense: the lowest source of everything, state 0)
    b, p0, A = vr.inputs("floats", 12, 5, 4)
    b[6] = -np.inf
    V, psi, states, logp = vr.viterbi32(b, p0, A)
    assert logp == -np.inf and np.isinf(V[6:]).all() and np.isfinite(V[:6]).all() and (psi[7:] == 0).all()
    assert (states[6:] == 0).all() and states[5] == psi[6][0] == int(np.argmax(V[5] + A[:, 0]))
    # a NaN emission at (t, s): V[t][s] is the NaN, the state is -inf for frame t + 1 and nothing else is touched
    b, p0, A = vr.inputs("floats", 12, 5, 5)
    clean = vr.viterbi32(b, p0, A)
    bn = b.copy()
    bn[4, 2] = np.nan
    masked = b.copy()
    masked[4, 2] = -np.inf
    V, psi, states, logp = vr.viterbi32(bn, p0, A)
    Vm, psim, statesm, logpm = vr.viterbi32(masked, p0, A)
    assert np.isnan(V[4, 2]) and np.isnan(V).sum() == 1 and vr.same_bits(V[:4], clean[0][:4])
    Vm[4, 2] = np.nan
    assert vr.same_bits(V, Vm) and (psi == psim).all() and (states == statesm).all() and vr.same_bits(logp, logpm) and np.isfinite(logp)
    assert (psi[5] != 2).all()
    # ... and as the last frame's state it counts as -inf at the end
    bn = b.copy()
    bn[11, clean[2][11]] = np.nan
    V, psi, states, logp = vr.viterbi32(bn, p0, A)
    assert states[11] != clean[2][11] and np.isfinite(logp)


def test_same_bits_and_makers():
    a = np.array([0.0, -0.0, np.nan, 1.0], np.float32)
    assert vr.same_bits(a, a.copy()) and not vr.same_bits(a, np.array([-0.0, -0.0, np.nan, 1.0], np.float32))
    assert not vr.same_bits(a, np.array([0.0, -0.0, 2.0, 1.0], np.float32)) and not vr.same_bits(a, a[:3])
    x = vr.eighths((200, 50), 1)
    assert 0.2 < np.isinf(x).mean() < 0.3 and ((x[np.isfinite(x)] * 8) % 1 == 0).all() and x[np.isfinite(x)].min() >= -3 and x.max() <= 0
    y = vr.floats((200, 50), 1)
    assert len(np.unique(y)) > 9900 and y.max() <= 0 and y.min() > -4
    band = vr.inputs("floats", 3, 6, 0, band_half=2)[2]
    assert (band[0, :2] == np.float32(1e30)).all() and (band[4, -2:] == np.float32(1e30)).all() and (band[2] <= 0).all()
