"""tests/dtw_ref.py on the CPU (include/jsgx.h sections 2 and 3): the vectorised restatement against the cell-by-cell float32 loop to
the bit, the header's known answers, the cost against float64 within the derived bounds, and the total against an independent float64
DTW within 3 (N + M) 2^-24."""
import numpy as np
import pytest

import dtw_ref as dr

U = 2.0 ** -24
WEIGHTS = [(None, None), ((1, 1.5, 0.75), (0, 0.25, 0.5))]


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (6, 1), (5, 9), (13, 4), (17, 17)])
@pytest.mark.parametrize("costs", [dr.integer_costs, dr.float_costs])
def test_restatement_equals_the_cell_loop(shape, costs):
    C = costs(*shape, seed=shape[0] * 100 + shape[1])
    for wm, wa in WEIGHTS:
        for subseq, band in ((False, 0), (True, 0), (False, 1), (False, 3)):
            D = dr.dtw32(C, wm, wa, subseq, band)
            assert dr.same_bits(D, dr.dtw32_loop(C, wm, wa, subseq, band)), (shape, wm, subseq, band)


def test_nan_and_signed_zero_rules():
    C = dr.integer_costs(9, 11, 3)
    C[4, 5] = np.nan
    assert dr.same_bits(dr.dtw32(C), dr.dtw32_loop(C))
    D = dr.dtw32(C)
    assert np.isnan(D[4, 5]) and not np.isnan(D[:4]).any() and not np.isnan(D[:, :5]).any()
    # a NaN v_0 stays (every later comparison is false); a NaN v_1 or v_2 never replaces best
    assert np.isnan(D[5, 6]) and not np.isnan(D[3, 6])
    # 1 * (-0) + 0 = +0: the operations are kept as written
    Z = np.full((2, 2), -0.0, np.float32)
    D = dr.dtw32(Z)
    assert np.signbit(D[0, 0]) and not np.signbit(D[0, 1]) and not np.signbit(D[1, 1])
    # subseq with a NaN in the last row: no path
    C = dr.float_costs(5, 8, 1)
    C[4, 2] = np.nan
    D = dr.dtw32(C, subseq=True)
    assert dr.backtrace32(D, C, subseq=True) == (None, None)


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (4, 1), (6, 6), (5, 9), (9, 4)])
def test_all_zero_cost_runs_on_the_diagonal_then_along_the_edge(shape):
    N, M = shape
    C = np.zeros(shape, np.float32)
    D = dr.dtw32(C)
    assert not D.any() and not np.signbit(D).any()
    path, total = dr.backtrace32(D, C)
    k = min(N, M) - 1
    want = [(N - 1 - q, M - 1 - q) for q in range(k + 1)]
    i, j = want[-1]
    want += [(i - q, j) for q in range(1, i + 1)] + [(i, j - q) for q in range(1, j + 1)]
    assert path.tolist() == [list(c) for c in want[::-1]] and total == 0


@pytest.mark.parametrize("shape, band, connected", [((65, 200), 1, False), ((65, 200), 2, True), ((10, 100), 4, False), ((10, 100), 5, True)])
def test_a_band_narrower_than_the_slope_has_no_path(shape, band, connected):
    C = dr.float_costs(*shape, seed=band)
    D = dr.dtw32(C, band=band)
    path, total = dr.backtrace32(D, C)
    assert (path is not None) == connected == bool(np.isfinite(D[-1, -1]))
    assert np.isinf(D[~dr.inside_band(*shape, band)]).all()
    if connected:
        assert path[0].tolist() == [0, 0] and path[-1].tolist() == [shape[0] - 1, shape[1] - 1] and dr.inside_band(*shape, band)[path[:, 0], path[:, 1]].all()
        _, total64, path64 = dr.dtw64(C, band=band)
        assert abs(float(total) - total64) <= 3 * sum(shape) * U * total64


@pytest.mark.parametrize("K", [1, 12, 128, 1024])
@pytest.mark.parametrize("kind", ["normal", "positive", "near-duplicate"])
@pytest.mark.parametrize("metric", list(dr.METRICS))
def test_cost_against_float64_within_the_derived_bound(metric, kind, K):
    """include/jsgx.h derives relative (K + 3) 2^-24 for the two Euclidean metrics and absolute (K + 5) 2^-24 for cosine; the worst found
    over these cases is recorded in profiles/dtw_accuracy.md."""
    worst, bound = dr.cost_errors(metric, kind, K)
    print(f"{metric} {kind} K={K}: worst {worst:.2f} u, bound {bound} u")
    assert worst <= bound


def test_cosine_of_a_zero_vector_is_one():
    X = np.zeros((2, 5), np.float32)
    X[1] = 1
    c = dr.cost32(X, X, "cosine")
    assert c[0, 0] == 1 and c[0, 1] == 1 and c[1, 0] == 1 and abs(c[1, 1]) <= 6 * U


@pytest.mark.parametrize("shape", [(40, 40), (30, 77), (90, 25)])
@pytest.mark.parametrize("subseq", [False, True])
def test_total_against_the_float64_dtw(shape, subseq):
    """Non-negative costs and weights: min is monotone and every sum is of non-negative terms, so the relative error of total is at most
    3 (N + M) 2^-24."""
    N, M = shape
    for seed, (wm, wa) in enumerate(WEIGHTS):
        X, Y = dr.cost_data("normal", N, M, 12, seed)
        C = dr.cost32(X, Y, "euclidean")
        D = dr.dtw32(C, wm, wa, subseq)
        path, total = dr.backtrace32(D, C, wm, wa, subseq)
        D64, total64, path64 = dr.dtw64(C, wm, wa, subseq)
        err = abs(float(total) - total64) / total64
        print(f"{shape} subseq={subseq}: {err / U:.2f} u against {3 * (N + M)} u")
        assert err <= 3 * (N + M) * U
        assert path[-1, 0] == N - 1 and path[0, 0] == 0 and (subseq or (path[0, 1] == 0 and path[-1, 1] == M - 1))
        assert (np.diff(path, axis=0) >= 0).all() and (np.diff(path, axis=0).max(axis=1) == 1).all()


def test_the_vectorised_loop_is_fast_enough():
    C = dr.float_costs(1000, 1000, 0)
    import time
    t = time.perf_counter()
    D = dr.dtw32(C)
    assert time.perf_counter() - t < 10 and np.isfinite(D[-1, -1])
