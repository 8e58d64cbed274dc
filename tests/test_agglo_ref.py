"""tests/agglo_ref.py, the restatement of include/jsgx.h section 17: its float64 form against scikit-learn's AgglomerativeClustering (Ward
linkage on a chain) on every shape the GPU test runs, its float32 form against the float64 one on the same planes, with the gap between
the best and the second-best cost of every step asserted (so no plane decides a step inside the rounding); the tree of k = 1 read at k';
subsegment against calls a stretch; the constant plane; the refusals.  CPU only."""
import numpy as np
import pytest

import agglo_ref as ar

IDS = [f"{N}x{F}-{kind}{seed}" for N, F, kind, seed in ar.PLANES]


def starts_of_labels(labels):
    return np.concatenate(([0], 1 + np.flatnonzero(np.diff(labels) != 0))).astype(np.int32)


@pytest.fixture(scope="module")
def trees():
    """The whole tree of every plane, once: float64 (starts, order, gap) and float32 (starts, order, height, gap)."""
    return {case: (ar.cluster64(ar.plane(*case), 1), ar.cluster32(ar.plane(*case), 1)) for case in
            ((N, F, seed, kind) for N, F, kind, seed in ar.PLANES)}


def test_the_planes_cover_the_shapes():
    assert {(N, F) for N, F, _, _ in ar.PLANES} == {(N, F) for N, F, _ in ar.SHAPES if N > 1}
    assert {N for N, _, _ in ar.SHAPES} == set(ar.N_SET) and {F for _, F, _ in ar.SHAPES} == set(ar.F_SET) and {P for _, _, P in ar.SHAPES} == set(ar.PAIRS_SET)
    assert set(ar.N_SET) == {1, 2, 3, 63, 64, 65, 257, 1025} and set(ar.F_SET) == {1, 63, 64, 65, 130} and ar.k_set(9) == (1, 2, 7, 9, 12)


@pytest.mark.parametrize("N, F, kind, seed", ar.PLANES, ids=IDS)
def test_the_gap_holds(trees, N, F, kind, seed):
    (_, _, gap64), (_, _, _, gap32) = trees[(N, F, seed, kind)]
    print(f"gap float64 {gap64:.3e} float32 {gap32:.3e}")
    assert gap64 >= ar.MIN_GAP


@pytest.mark.parametrize("N, F, kind, seed", ar.PLANES, ids=IDS)
def test_float64_gives_scikit_learn_s_boundaries(trees, N, F, kind, seed):
    from sklearn.cluster import AgglomerativeClustering
    from sklearn.feature_extraction.image import grid_to_graph
    X = ar.plane(N, F, seed, kind).astype(np.float64)
    order = trees[(N, F, seed, kind)][0][1]
    graph = grid_to_graph(N, 1, 1)
    for k in sorted({k for k in ar.k_set(N) if k <= N}):
        labels = AgglomerativeClustering(n_clusters=k, linkage="ward", connectivity=graph).fit(X).labels_
        assert (starts_of_labels(labels) == ar.cut_tree(order, k, N)).all(), k
        assert (ar.cluster64(X, k)[0] == ar.cut_tree(order, k, N)).all(), k


@pytest.mark.parametrize("N, F, seed", ar.NOISE_PLANES, ids=[f"{N}x{F}-noise{seed}" for N, F, seed in ar.NOISE_PLANES])
def test_float64_gives_scikit_learn_s_boundaries_on_long_noise(N, F, seed):
    """The long planes above are of one well-separated family, so the float64 form and scikit-learn are also compared on noise of 257
    and 1025 frames.  Both compute in float64, whose operations round at 1.1e-16: with the cost a sum of up to 130 rounded terms a
    relative gap of 1e-9 between the best and the second-best cost of every step keeps every decision seven decades clear of it, and
    that gap is asserted (the float32 form is not compared here: its rounding is inside noise's gaps, profiles/agglo_accuracy.md)."""
    from sklearn.cluster import AgglomerativeClustering
    from sklearn.feature_extraction.image import grid_to_graph
    X = ar.plane(N, F, seed).astype(np.float64)
    _, order, gap = ar.cluster64(X, 1)
    print(f"gap float64 {gap:.3e}")
    assert gap >= 1e-9
    graph = grid_to_graph(N, 1, 1)
    for k in (2, 7, 12, N // 4):
        labels = AgglomerativeClustering(n_clusters=k, linkage="ward", connectivity=graph).fit(X).labels_
        assert (starts_of_labels(labels) == ar.cut_tree(order, k, N)).all(), k


@pytest.mark.parametrize("N, F, kind, seed", ar.PLANES, ids=IDS)
def test_float32_gives_the_float64_boundaries(trees, N, F, kind, seed):
    (_, order64, _), (_, order32, _, _) = trees[(N, F, seed, kind)]
    assert (order32 == order64).all()


@pytest.mark.parametrize("N, F, kind, seed", ar.PLANES, ids=IDS)
def test_the_tree_of_k_1_read_at_k(trees, N, F, kind, seed):
    X = ar.plane(N, F, seed, kind)
    _, order, height, _ = trees[(N, F, seed, kind)][1]
    for k in ar.k_set(N):
        starts, o, h, _ = ar.cluster32(X, k)
        kk = min(k, N)
        assert (starts == ar.cut_tree(order, k, N)).all() and len(starts) == kk
        assert (o == order[:N - kk]).all() and (h.view(np.uint32) == height[:N - kk].view(np.uint32)).all()


def test_subsegment_equals_the_calls_a_stretch():
    X = ar.plane(300, 7, 3)
    bounds = np.array([-5, 0, 10, 10, 11, 80, 150, 290, 400], np.int32)
    for pad in (True, False):
        for k in (1, 4, 500):
            n_out, out, n, u, steps = ar.segment(X, bounds, len(bounds), k, pad)
            assert u.tolist() == [0, 10, 11, 80, 150, 290, 300]          # 0 and N are in the clipped list itself
            want, want_steps = [], []
            for a, b in zip(u[:-1], u[1:]):
                starts, order, height, _ = ar.cluster32(X[a:b], k)
                want += list(a + starts)
                want_steps += [(a + j, a + int(r), int(h.view(np.uint32))) for j, (r, h) in enumerate(zip(order, height))]
            assert n == len(u) - 1 and n_out == len(want) == sum(min(k, b - a) for a, b in zip(u[:-1], u[1:])) and out.tolist() == want and steps == want_steps
            # the same through the trees the caller keeps
            tree = lambda a, b: ar.cluster32(X[a:b], 1)[1:3]
            again = ar.segment(X, bounds, len(bounds), k, pad, tree=tree)
            assert again[0] == n_out and again[1].tolist() == want and again[4] == steps
    n_out, out, n, u, _ = ar.segment(X, bounds[2:6], 4, 3, False)          # without the pad the plane's ends are no boundaries
    assert u.tolist() == [10, 11, 80] and out.tolist() == [10] + list(11 + ar.cluster32(X[11:80], 3)[0])
    assert ar.segment(X, np.zeros(0, np.int32), 0, 5, True)[1].tolist() == ar.cluster32(X, 5)[0].tolist()          # agglomerative


def test_a_constant_plane_merges_from_the_left():
    for value in (0.0, -0.0, 2.5):
        X = np.full((40, 9), value, np.float32)
        starts, order, height, gap = ar.cluster32(X, 1)
        assert order.tolist() == list(range(1, 40)) and (height.view(np.uint32) == 0).all() and gap == 0.0 and starts.tolist() == [0]
        assert ar.cluster32(X, 5)[0].tolist() == [0, 36, 37, 38, 39]
    mixed = np.zeros((6, 2), np.float32)
    mixed[1::2] = -0.0          # -0 against +0: every difference is a zero, every cost +0
    assert ar.cluster32(mixed, 1)[1].tolist() == [1, 2, 3, 4, 5] and (ar.cluster32(mixed, 1)[2].view(np.uint32) == 0).all()
    twice = np.repeat(ar.plane(10, 4, 1), 2, axis=0)          # repeated frames: the ten costs of 0 go first, from the left
    assert ar.cluster32(twice, 10)[1].tolist() == list(range(1, 20, 2))


def test_costs_that_overflow_still_sort():
    X = ar.OVERFLOW
    starts, order, height, _ = ar.cluster32(X, 1)
    # the two costs of 0 from the left; the sums are infinities from there on: inf - finite sorts below inf - inf, which has one spelling
    assert order.tolist() == [1, 3, 4, 2] and height.view(np.uint32).tolist() == [0, 0, 0x7F800000, ar.NAN_BITS]
    assert starts.tolist() == [0]


def test_the_refusals():
    X = ar.plane(50, 3, 1)
    b = np.array([10, 20, 30], np.int32)
    assert ar.segment(X, b, -1, 2, True)[0:3:2] == (-1, -1)          # a negative count
    assert ar.segment(X, np.array([10, 30, 20], np.int32), 3, 2, True)[0:3:2] == (-1, -1)          # a decreasing list
    assert ar.segment(X, np.array([10, 30, 20], np.int32), 2, 2, True)[0:3:2] == (2 + 2 + 2, 3)          # ... beyond the count
    for bad in (np.nan, np.inf, -np.inf):
        Y = X.copy()
        Y[25, 1] = bad
        n_out, out, n, u, steps = ar.segment(Y, b, 3, 2, True)
        assert (n_out, n, out.size, steps) == (-1, 4, 0, []) and u.tolist() == [0, 10, 20, 30, 50]
        assert ar.segment(Y, b[:2], 2, 2, False)[0] == 2 and ar.segment(Y, b[:1], 1, 2, False)[0] == 0          # frames 10..19 alone; no stretch
        Y = X.copy()
        Y[5, 0] = Y[30, 2] = bad          # outside u[0] .. u[U-1]-1
        assert ar.segment(Y, b, 3, 2, False)[0] == 4
    long = np.zeros((ar.MAX_STRETCH + 2, 1), np.float32)
    assert ar.segment(long, np.array([1], np.int32), 1, ar.MAX_STRETCH, True)[0] == -1          # a stretch of MAX_STRETCH + 1 frames
    assert ar.segment(long, np.array([2], np.int32), 1, ar.MAX_STRETCH, True)[0] == 2 + ar.MAX_STRETCH
