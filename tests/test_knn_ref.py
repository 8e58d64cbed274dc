"""tests/knn_ref.py on the CPU (include/jsgx.h sections 6 to 8): the restated selection against a brute-force transcription of the
definition; the lists in full order against scikit-learn's brute-force NearestNeighbors in float64 after the same band removal; the
symmetry of the mutual plane; the invariance under a column split; the affinity routine against exp in double; the aggregation and the
bandwidth rule against plain float64."""
import numpy as np
import pytest

import beat_ref as br
import knn_ref as kr

SKLEARN_CASES = [(300, 12, 10, 3, 0), (257, 20, 34, 1, 1), (130, 5, 8, 0, 2)]        # N, K, k, width, seed


@pytest.mark.parametrize("metric", ["sqeuclidean", "euclidean", "cosine"])
@pytest.mark.parametrize("kind", kr.KINDS)
def test_the_restatement_is_the_definition(kind, metric):
    """np.lexsort on (j, c) over the candidates against an explicit loop per row that inserts one candidate at a time."""
    for N, M, k, width in ((40, 70, 9, 1), (70, 40, 50, 3), (5, 5, 8, 0), (6, 6, 2, 9)):
        X, Y = kr.frames(kind, N, M, 4, 11)
        C = kr.cost32(X, Y, metric)
        got, want = kr.select32(C, k, width), kr.select_brute(C, k, width)
        assert np.array_equal(got[0], want[0]) and kr.same_bits(got[1], want[1]), (kind, metric, N, M)
        cnt = (got[0] >= 0).sum(axis=1)
        cands = ((np.abs(np.arange(N)[:, None] - np.arange(M)[None, :]) >= width) & ~np.isnan(C)).sum(axis=1)
        assert (cnt == np.minimum(k, cands)).all() and (got[0][got[0] < 0] == -1).all() and np.isinf(got[1][got[0] < 0]).all()
        # the lists are sorted by (c, j), and what follows the list is no nearer
        for i in range(N):
            keys = [(got[1][i, r], got[0][i, r]) for r in range(cnt[i])]
            assert keys == sorted(keys)


def test_ties_and_signed_zeros():
    """-0 == +0: the lower j goes first whatever the sign; the bits of the stored cost are the cell's own."""
    C = np.array([[0.0, -0.0, 1.0, -0.0, 0.0, np.inf, np.nan, np.inf]], np.float32)
    index, dist = kr.select32(C, 8)
    assert index.tolist() == [[0, 1, 3, 4, 2, 5, 7, -1]]
    assert kr.same_bits(dist, np.array([[0.0, -0.0, -0.0, 0.0, 1.0, np.inf, np.inf, np.inf]], np.float32))


@pytest.mark.parametrize("N, K, k, width, seed", SKLEARN_CASES)
def test_the_lists_are_those_of_scikit_learn_in_full_order(N, K, k, width, seed):
    """librosa's route: the k + 2 width nearest of every frame from NearestNeighbors(algorithm="brute") in float64, the band dropped, the
    nearest k kept.  Every row, every position."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    X = np.random.default_rng(seed).standard_normal((N, K)).astype(np.float32)
    index, dist = kr.knn32(X, X, k, width, "euclidean")
    knn = neighbors.NearestNeighbors(n_neighbors=min(N, k + 2 * width), algorithm="brute").fit(X.astype(np.float64))
    d64, j64 = knn.kneighbors(X.astype(np.float64))
    for i in range(N):
        keep = np.abs(j64[i] - i) >= width
        assert np.array_equal(j64[i][keep][:k], index[i]), i
        assert np.allclose(d64[i][keep][:k], dist[i], rtol=(K + 3) * 2.0 ** -24, atol=1e-6), i       # atol: a frame against itself is ~1e-8 by the expanded form, not 0
    # the gap between the k-th and the next distance is far above the error of the float32 chain, so the order is not an accident
    C = kr.cost32(X, X).astype(np.float64)
    C[np.abs(np.arange(N)[:, None] - np.arange(N)[None, :]) < width] = np.inf
    C.sort(axis=1)
    assert ((C[:, k] - C[:, k - 1]) / C[:, k]).min() > 5 * (K + 3) * 2.0 ** -24


def test_the_mutual_plane_is_symmetric():
    for kind in ("integers", "floats"):
        X = kr.frames(kind, 90, 90, 6, 3)[0]
        C = kr.cost32(X, X)
        assert kr.same_bits(C, C.T)                                  # the costs of x against itself are bitwise symmetric
        index, dist = kr.select32(C, 9, 1)
        for mode in kr.MODES:
            one = kr.recurrence32(index, dist, 90, mode, False, False, kr.bandwidth32(dist))
            both = kr.recurrence32(index, dist, 90, mode, True, False, kr.bandwidth32(dist))
            assert kr.same_bits(both, both.T) and not kr.same_bits(one, one.T)
            assert ((both != 0) == ((one != 0) & (one.T != 0))).all() or mode == "distance"      # minimum(rec, rec.T) on the links
            assert kr.same_bits(both[both != 0], one[both != 0])
        conn = kr.recurrence32(index, dist, 90, "connectivity", True, True)
        assert (np.diag(conn) == 1).all() and (np.diag(kr.recurrence32(index, dist, 90, "distance", False, True)) == 0).all()


def test_invariance_under_a_column_split():
    for kind in kr.KINDS:
        X, Y = kr.frames(kind, 30, 330, 5, 5)
        C = kr.cost32(X, Y)
        for k in (1, 7, 70):
            want = kr.select32(C, k, 2)
            for S in (1, 2, 3, 4, 5, 6, 16):
                got = kr.split_select32(C, k, 2, S)
                assert np.array_equal(got[0], want[0]) and kr.same_bits(got[1], want[1]), (kind, k, S)


def test_the_affinity_routine_inside_its_bound():
    """jsgx_exp on a strided sample of every float32 in [-87, 0] and on the edges, against exp in double: JSGX_EXP_REL_BOUND, which holds
    over the whole range (profiles/knn_accuracy.md: every float32 of the range was measured)."""
    lo, hi = np.float32(-87.0).view(np.uint32), np.float32(-0.0).view(np.uint32)
    bits = np.concatenate([np.arange(hi, lo + 1, 4093, dtype=np.uint64), [lo, lo - 1, hi, hi + 1, hi + 2]]).astype(np.uint32)
    x = np.concatenate([bits.view(np.float32), np.float32([0.0, -1.0, -0.5 * np.log(2), -np.log(2), -86.99999, -5.89112377, -1e-30, -1e-45])])      # -5.89...: the worst of the whole range
    assert x.min() == -87.0 and x.max() == 0.0 and x.size > 270000
    got = br.exp32(x).astype(np.float64)
    rel = np.abs(got - np.exp(x.astype(np.float64))) / np.exp(x.astype(np.float64))
    print("jsgx_exp on the sample of [-87, 0]: worst relative error", rel.max(), "at", x[rel.argmax()])
    assert rel.max() <= br.EXP_REL_BOUND
    assert br.exp32(np.float32([-87.00001, -1e30, -np.inf])).tolist() == [0.0, 0.0, 0.0]
    # the affinity of the plane: the argument is -fl(d / bw)
    d = np.float32([0.0, 0.5, 1.0, 3.0, np.inf, np.nan])
    got = kr.affinity32(d, 0.75)
    assert got[0] == 1 and got[4] == 0 and np.isnan(got[5])
    assert np.allclose(got[1:4], np.exp(-d[1:4].astype(np.float64) / 0.75), rtol=3 * 2.0 ** -24 + br.EXP_REL_BOUND * 1.01, atol=0)
    for bad in (0.0, -1.0, np.nan):
        assert np.isnan(kr.affinity32(d, bad)).all()


def test_the_aggregation_and_the_bandwidth():
    rng = np.random.default_rng(8)
    N, F, k = 50, 13, 6
    S = rng.standard_normal((N, F)).astype(np.float32)
    index = rng.integers(0, N, (N, k)).astype(np.int32)
    index[3] = -1
    index[4, 2:] = -1
    W = rng.random((N, k)).astype(np.float32)
    W[5] = [1, -1, 2, -2, 0, 0]
    mean = kr.nn_filter32(S, index)
    weighted = kr.nn_filter32(S, index, W)
    u = 2.0 ** -24
    for i in range(N):
        js = index[i][index[i] >= 0]
        if js.size == 0:
            assert kr.same_bits(mean[i], S[i]) and kr.same_bits(weighted[i], S[i])
            continue
        want = S[js].astype(np.float64).mean(axis=0)
        assert np.abs(mean[i] - want).max() <= (k + 1) * u * np.abs(S[js]).sum(axis=0).max()
        w = W[i][index[i] >= 0].astype(np.float64)
        if i == 5:
            assert kr.same_bits(weighted[i], S[i])                   # the weights sum to zero
        else:
            want = (w[:, None] * S[js]).sum(axis=0) / w.sum()
            assert np.abs(weighted[i] - want).max() <= (2 * k + 2) * u * (np.abs(w[:, None] * S[js]).sum(axis=0) / w.sum()).max()
    assert kr.same_bits(mean[4], ((S[index[4, 0]] + S[index[4, 1]]) / np.float32(2)))
    # the bandwidth: the median of the finite k-th distances, the mean of the two middle ones for an even count
    dist = np.sort(rng.random((9, 4)).astype(np.float32), axis=1)
    assert kr.bandwidth32(dist) == np.float32(np.median(dist[:, -1]))
    dist[2, -1] = np.inf
    v = np.sort(dist[np.isfinite(dist[:, -1]), -1])
    assert kr.bandwidth32(dist) == np.float32(0.5) * (v[3] + v[4]) and np.isclose(kr.bandwidth32(dist), np.median(v))
    assert kr.default_k(300, 3) == 2 * 18 and kr.default_k(10 ** 6) == 256 and kr.default_k(4, 5) == 1
