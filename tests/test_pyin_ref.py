"""The restatement of include/jsgx.h section 5 (tests/pyin_ref.py) against independent readings, on the CPU: the factored decoder against
brute force over all paths and against the dense restatement of section 4 where every sum is exact; logp and the observation against
float64 inside the header's derived bounds; L against numpy; the known answers of the observation."""
import itertools

import numpy as np
import pytest

import pyin_ref as pr
import viterbi_ref as vr

U = 2.0 ** -24


def brute_force(b, p0, lw, off, sw):
    """The best path by enumeration, with the pair rule read as "the lexicographically lowest state sequence from the end backwards"."""
    A = pr.dense_of(lw, off, sw, dtype=np.float64)
    T, S = b.shape
    best, best_path = -np.inf, None
    for path in itertools.product(range(S), repeat=T):
        lp = float(p0[path[0]]) + float(b[0][path[0]])
        for t in range(1, T):
            lp += A[path[t - 1], path[t]] + float(b[t][path[t]])
        if lp > best:
            best, best_path = lp, path
    return best, best_path


@pytest.mark.parametrize("P, W, T", [(1, 0, 4), (2, 0, 4), (2, 1, 4), (3, 1, 3), (3, 2, 3), (3, 5, 2), (1, 3, 1)])
def test_the_decoder_equals_brute_force(P, W, T):
    """Random floats: no ties, so the best path is unique and the sum along it is within a few u of the exact one."""
    for seed in range(4):
        b, p0, lw, off, sw = pr.decode_inputs("floats", T, P, W, 10 * P + seed)
        V, psi, states, logp = pr.decode32(b, p0, lw, off, sw)
        best, path = brute_force(b, p0, lw, off, sw)
        assert tuple(states) == path, (P, W, T, seed)
        assert abs(float(logp) - best) <= (4 * T + 2) * U * abs(best)


@pytest.mark.parametrize("P, W", [(1, 0), (2, 1), (5, 0), (5, 2), (7, 9), (16, 3), (33, 8), (40, 50)])
def test_the_decoder_equals_the_dense_restatement_on_exact_sums(P, W):
    """Multiples of 1/8 in a small range: every sum is exact, so the two association orders give the same V, and the tie rules (the
    lowest p, then u = 0; the lowest state u P + p) must pick the same source.  A tenth of the emissions are -inf; a destination all of
    whose sources are -inf is where psi differs by the header (V is -inf there either way), so psi is compared at the others."""
    for seed in range(3):
        T = 23
        b, p0, lw, off, sw = pr.decode_inputs("eighths", T, P, W, 100 + 7 * P + seed, dead=0.1)
        V, psi, states, logp = pr.decode32(b, p0, lw, off, sw)
        A = pr.dense_of(lw, off, sw)
        dV, dpsi, dstates, dlogp = vr.viterbi32(b, p0, A)
        reachable = np.isfinite((V[:-1, :, None] + A[None]).max(axis=1))        # [t-1][j]: some source of j at frame t is above -inf
        assert reachable.mean() > 0.5 and np.isfinite(logp)       # a path above -inf never goes through a destination without a live source
        assert vr.same_bits(V, dV) and (psi[1:] == dpsi[1:])[reachable].all() and (states == dstates).all() and vr.same_bits(logp, dlogp)
        assert len(np.unique(states)) > 1 or P == 1


@pytest.mark.parametrize("P, W, T", [(5, 2, 50), (33, 8, 300), (601, 50, 64), (64, 128, 100)])
def test_logp_inside_the_derived_bound_of_float64(P, W, T):
    b, p0, lw, off, sw = pr.decode_inputs("floats", T, P, W, P + T)
    V, psi, states, logp = pr.decode32(b, p0, lw, off, sw)
    want = pr.decode64(b, p0, lw, off, sw)
    err = abs(float(logp) - want) / abs(want)
    print(f"P={P} W={W} T={T}: logp relative error {err / U:.2f} u, bound {(4 * T + 2)} u")
    assert err <= (4 * T + 2) * U
    assert (np.abs(np.diff(states % P)) <= W).all()


def test_all_zero_inputs_give_the_known_answer():
    P, W, T = 9, 2, 6
    z = lambda n: np.zeros(n, np.float32)
    V, psi, states, logp = pr.decode32(np.zeros((T, 2 * P), np.float32), z(2 * P), z(2 * W + 1), z(P), z(4))
    assert (V.view(np.uint32) == 0).all() and (states == 0).all() and logp.view(np.uint32) == 0
    assert (psi[1:] == np.tile(np.maximum(0, np.arange(P) - W), 2)[None, :]).all()


def test_the_logarithm_routine():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.random(200000).astype(np.float32), np.float32(2.0) ** -rng.integers(0, 150, 2000).astype(np.float32) * rng.random(2000).astype(np.float32),
                        np.array([1.0, 0.5, 2.0 ** -126, 2.0 ** -149, 2.0 ** -127, np.nextafter(np.float32(1), np.float32(0))], np.float32)])
    x = x[x > 0]
    got = pr.log32(x).astype(np.float64)
    want = np.log(x.astype(np.float64))
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"L: worst |L(x) - ln x| / max(1, |ln x|) over {x.size} samples: {err.max():.3e}")
    assert err.max() <= 1.0e-7                                  # JSGX_LOG_ABS_BOUND
    assert pr.log32(np.float32(1)).view(np.uint32) == 0 and pr.log32(np.float32(0)) == -np.inf and np.isnan(pr.log32(np.float32(-1)))
    assert np.isnan(pr.log32(np.float32(np.nan))) and pr.log32(np.float32(np.inf)) == np.inf


def test_the_observation_inside_the_derived_bound_of_float64():
    """Frames without bin collisions.  The float32 tables are the float64 ones rounded once (three roundings on top of the header's 13):
    17 u to first order; the second-order part is below 17^2 u^2 < 0.0001 u, so 18 u is asserted."""
    from scipy import stats
    rng = np.random.default_rng(11)
    sr, fmin, bps, P, N, lam, ntp = 22050.0, 65.40639132514966, 10, 601, 100, 2.0, 0.01
    tau_min, tau_max = 10, 338
    prior = np.diff(stats.beta.cdf(np.linspace(0, 1, N + 1), 2, 18)).astype(np.float32)
    decay, norm = pr.boltzmann_tables(lam, pr.max_troughs(tau_min, tau_max))
    edges, freqs = pr.bins_tables(sr, fmin, bps, P)
    checked, worst = 0, 0.0
    for i in range(40):
        h = pr.frame_of(rng, tau_max, int(rng.integers(1, 6)), 1.2)
        emit, obs, voiced = pr.observe32(h, tau_min, tau_max, prior, decay, norm, edges, ntp)
        lags = pr.troughs_of(h, tau_min, tau_max)
        bins32 = [pr.bin_of(pr.period32(h, tau), edges, P) for tau in lags]
        obs64, voiced64, bins64, lags64 = pr.observe64(h, tau_min, tau_max, N, (2, 18), lam, sr, fmin, bps, P, ntp)
        assert lags64 == lags, (i, lags, lags64)                      # the two readings of the trough rule agree
        if len(set(bins32)) != len(bins32) or bins32 != bins64:       # a collision, or a period within rounding of a bin edge
            continue
        checked += 1
        live = obs64 > 0
        assert ((obs > 0) == live).all()
        err = np.abs(obs[live].astype(np.float64) - obs64[live]) / obs64[live]
        worst = max(worst, err.max())
        assert err.max() <= 18 * U, (i, err.max() / U)
        assert abs(float(voiced) - voiced64) <= (18 + P // 64 + 7) * U * voiced64
        with np.errstate(divide="ignore"):
            want = np.log(obs.astype(np.float64))
        assert (np.abs(emit[:P][live] - want[live]) <= 1.0e-7 * np.maximum(1, np.abs(want[live]))).all() and np.isneginf(emit[:P][~live]).all()
    print(f"observation: {checked} frames without collisions, worst relative error of obs {worst / U:.2f} u")
    assert checked >= 20


def test_known_answers_of_the_observation():
    P, N = 7, 10
    prior = np.full(N, 0.1, np.float32)
    decay, norm = pr.boltzmann_tables(2.0, 10)
    edges, _ = pr.bins_tables(100.0, 5.0, 1, P)
    silent = np.ones(21, np.float32)
    emit, obs, voiced = pr.observe32(silent, 2, 20, prior, decay, norm, edges, 0.01)
    assert (obs.view(np.uint32) == 0).all() and voiced.view(np.uint32) == 0 and np.isneginf(emit[:P]).all()
    assert pr.same_bits(emit[P:], np.full(P, pr.log32(np.float32(1) / np.float32(P))))
    high = np.full(21, 3.0, np.float32)
    high[9] = 1.5                     # the only trough, at or above 1
    emit, obs, voiced = pr.observe32(high, 2, 20, prior, decay, norm, edges, 0.01)
    want = np.float32(np.float32(0.01) * pr.lane_sum(prior))
    b = pr.bin_of(pr.period32(high, 9), edges, P)
    assert obs[b] == want and np.count_nonzero(obs) == 1 and voiced == want
    nan = silent.copy()
    nan[5] = np.nan
    emit, obs, voiced = pr.observe32(nan, 2, 20, prior, decay, norm, edges, 0.01)
    assert np.isnan(voiced) and (obs == 0).all() and np.isneginf(emit[:P]).all() and pr.same_bits(emit[P:], np.full(P, pr.log32(np.float32(1) / np.float32(P))))
    nan[5], nan[1] = 1.0, np.nan      # outside tau_min..tau_max: not looked at
    assert pr.observe32(nan, 2, 20, prior, decay, norm, edges, 0.01)[2] == 0
