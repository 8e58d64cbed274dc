"""tests/rqa_ref.py against itself and against the known answers of include/jsgx.h section 9: the row-by-row restatement equals the
cell-by-cell text bit for bit; both equal an independent brute force over every chain of allowed steps on small planes whose arithmetic
is exact; the all-zero plane, the identity and the identity with a gap of two; the path's bounds.  CPU only."""
import numpy as np
import pytest

import rqa_ref as rr

PENALTIES = [(1.0, 1.0), (0.5, 0.25), (0.0, 0.0)]


@pytest.mark.parametrize("knight", [False, True])
@pytest.mark.parametrize("kind", ["integer_links", "float_links"])
def test_rows_equal_the_cell_by_cell_text(kind, knight):
    for seed, (N, M) in enumerate([(1, 1), (1, 7), (7, 1), (2, 2), (3, 9), (9, 3), (24, 31), (40, 17)]):
        R = getattr(rr, kind)(N, M, seed)
        if N * M > 20:          # special values: a NaN, a negative and a -0 cell, one of them on the border
            R[N // 2, M // 2], R[0, M - 1], R[N - 1, 1] = np.nan, -1.5, -0.0
        for on, ex in PENALTIES:
            S, step = rr.rqa32(R, on, ex, knight)
            S2, step2 = rr.rqa32_loop(R, on, ex, knight)
            assert rr.same_bits(S, S2) and np.array_equal(step, step2), (kind, N, M, on, ex)
            assert S.dtype == np.float32 and step.dtype == np.int8 and set(np.unique(step)) <= ({-2, -1, 0, 1, 2} if knight else {-2, -1, 0})
            assert (step[1:, 1:] != -2).all() and (step[0] < 0).all() and (step[:, 0] < 0).all()


@pytest.mark.parametrize("knight", [False, True])
def test_rows_equal_the_brute_force_over_chains(knight):
    """Planes over {0, 1, 2} with dyadic penalties: every operation is exact, so the maximum over all chains is S in every bit."""
    rng = np.random.default_rng(5)
    shapes = [(N, M) for N in range(1, 7) for M in range(1, 7)]
    for n, (N, M) in enumerate(shapes * 3):
        R = rng.integers(0, 3, (N, M)).astype(np.float32)
        on, ex = [(1.0, 1.0), (0.5, 0.25), (0.0, 0.0), (0.25, 1.5), (2.0, 0.5)][n % 5]
        S, _ = rr.rqa32(R, on, ex, knight)
        assert np.array_equal(S, rr.rqa_chains(R, on, ex, knight)), (N, M, on, ex, R)
        assert (S >= 0).all() and not np.signbit(S).any()


def test_known_answers_of_the_header():
    # an all-zero plane
    S, step = rr.rqa32(np.zeros((9, 13), np.float32))
    assert (S == 0).all() and not np.signbit(S).any() and (step == -1).all()
    path, end, total = rr.backtrace32(S, np.zeros((9, 13), np.float32))
    assert len(path) == 0 and end == (-1, -1) and total == 0 and not np.signbit(total)
    N, g, on, ex = 70, 2, 0.5, 0.25
    for knight in (False, True):
        # the identity: the main diagonal, total N, a unique end cell
        I = np.eye(N, dtype=np.float32)
        S, step = rr.rqa32(I, on, ex, knight)
        path, end, total = rr.backtrace32(S, I, on, ex, knight)
        assert total == N and end == (N - 1, N - 1) and (S == total).sum() == 1 and path.tolist() == [[i, i] for i in range(N)]
        assert step[0, 0] == -2 and (np.diag(step)[1:] == 0).all()
    # the identity with two cells cleared: a gap of two, crossed on the diagonal without knight moves ...
    G = np.eye(N, dtype=np.float32)
    G[g, g] = G[g + 1, g + 1] = 0
    S, _ = rr.rqa32(G, on, ex, False)
    path, end, total = rr.backtrace32(S, G, on, ex, False)
    assert total == N - 2 - on - ex == 67.25 and end == (N - 1, N - 1) and path.tolist() == [[i, i] for i in range(N)]
    assert S[g, g] > 0 and S[g + 1, g + 1] > 0
    # ... and bridged by one knight move with them
    S, step = rr.rqa32(G, on, ex, True)
    path, end, total = rr.backtrace32(S, G, on, ex, True)
    assert total == 67.5 and len(path) == 69 and end == (N - 1, N - 1) and (step[path[:, 0], path[:, 1]] > 0).any()


@pytest.mark.parametrize("knight", [False, True])
@pytest.mark.parametrize("kind", ["integer_links", "float_links"])
def test_paths_are_bounded_and_positive(kind, knight):
    for seed, (N, M) in enumerate([(1, 5), (5, 1), (2, 70), (33, 20), (40, 41)]):
        R = getattr(rr, kind)(N, M, 100 + seed)
        for on, ex in PENALTIES:
            S, step = rr.rqa32(R, on, ex, knight)
            path, end, total = rr.backtrace32(S, R, on, ex, knight)
            assert 1 <= len(path) <= min(N, M) and tuple(path[-1]) == end and total == S[end] == S.max()
            assert (S[path[:, 0], path[:, 1]] > 0).all()
            assert (np.diff(path[:, 0]) >= 1).all() and (np.diff(path[:, 1]) >= 1).all()
            # the recomputed steps are the forward ones, and the path follows them
            moves = [rr.STEPS[k] for k in step[path[1:, 0], path[1:, 1]]]
            assert np.array_equal(np.diff(path, axis=0), np.asarray(moves, np.int32).reshape(-1, 2))
            first = step[path[0, 0], path[0, 1]]
            assert first == -2 or step[path[0, 0] - rr.STEPS[first][0], path[0, 1] - rr.STEPS[first][1]] == -1
