"""tests/sync_ref.py, the float32 restatement of include/jsgx.h sections 15 and 16, against plain numpy on exact data (small integers, where
no order of summation shows): np.mean, np.min, np.max and np.median over np.split at the unique padded boundaries, np.pad + np.roll for the
stacking; the segment rule on its edge cases; the keys; and that the chunked order of the mean can be told from a single chain.  CPU only."""
import numpy as np
import pytest

import sync_ref as sr

ORDER_SEED = 0          # chosen on the CPU: test_the_chunked_order_shows asserts that it serves


def small_integers(N, F, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(N, F)).astype(np.float32)


@pytest.mark.parametrize("name, fn", [("mean", np.mean), ("min", np.min), ("max", np.max), ("median", np.median)])
@pytest.mark.parametrize("pad", [True, False])
def test_aggregates_against_numpy_on_exact_data(name, fn, pad):
    N, F = 1025, 5
    X = small_integers(N, F, 1)
    rng = np.random.default_rng(2)
    bounds = np.sort(rng.integers(-3, N + 4, size=40)).astype(np.int32)
    bounds[7] = bounds[6]          # a repeat
    n, u, out = sr.sync(X, bounds, len(bounds), sr.AGGREGATES[name], pad, max_segments=N)
    edges = np.unique(np.concatenate(([0, N], np.clip(bounds, 0, N))) if pad else np.clip(bounds, 0, N))
    assert n == len(edges) - 1 and (u == edges).all()
    pieces = np.split(X, edges, axis=0)[1:-1]          # without what lies in front of the first edge and behind the last
    assert [len(piece) for piece in pieces] == np.diff(edges).tolist()
    want = np.stack([fn(piece.astype(np.float64), axis=0) for piece in pieces]).astype(np.float32)
    # sums of at most 1025 integers of at most 8 are exact in float32, and so is half the sum of two of them: only the divide rounds
    assert (out.view(np.float32) == want).all()


def test_segment_rule():
    N = 100
    seg = lambda b, n=None, pad=True, **kw: sr.segments(np.asarray(b, np.int32), len(b) if n is None else n, N, pad, **kw)
    n, u = seg([])
    assert n == 1 and u.tolist() == [0, N]          # no boundary, padded: one segment
    assert seg([], pad=False)[0] == 0 and seg([], pad=False)[1].size == 0          # and none without
    assert seg([5, 5, 9, 9, 9, 40])[1].tolist() == [0, 5, 9, 40, N]          # repeats (a backtracked list)
    assert seg([-7, -1, 3, 250, 300])[1].tolist() == [0, 3, N]          # below 0 and above N: clipped, then repeats
    assert seg([0, 50, N])[1].tolist() == [0, 50, N]          # 0 and N given with pad
    assert seg([0, 50, N], pad=False)[1].tolist() == [0, 50, N]
    assert seg([10, 20, 30, 40], n=9, max_bounds=3)[1].tolist() == [0, 10, 20, 30, N]          # n_bounds > max_bounds
    assert seg([10, 20], n=-1) == (-1, None) and seg([10, 9, 50]) == (-1, None)          # refused
    assert seg([10, 9, 50], n=1)[0] == 2          # the decrease lies behind the count
    assert seg([-5, -9])[0] == -1          # judged on the raw values, not the clipped ones
    assert seg([7], pad=False)[0] == 0 and seg([7, 7, 7], pad=False)[0] == 0          # U = 1: no segment
    n, u, out = sr.sync(np.zeros((N, 2), np.float32), np.arange(10, 60, 10, dtype=np.int32), 5, sr.MEAN, True, max_segments=3)
    assert n == 6 and u.tolist() == [0, 10, 20, 30] and out.shape == (3, 2)          # cut by max_segments, the whole count reported


def test_keys_and_special_values():
    inf = np.float32(np.inf)
    v = np.array([-inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.0, inf], np.float32)
    k = sr.key(v)
    assert (np.diff(k.astype(np.int64)) > 0).all() and (sr.unkey(k).view(np.uint32) == v.view(np.uint32)).all()
    col = lambda *x: np.array(x, np.float32)[:, None]
    bits = lambda f: int(np.float32(f).view(np.uint32))
    assert sr.aggregate(col(0.0, -0.0), sr.MIN)[0] == bits(-0.0) and sr.aggregate(col(-0.0, 0.0), sr.MAX)[0] == bits(0.0)
    assert sr.aggregate(col(0.0, -0.0, -0.0), sr.MEDIAN)[0] == bits(-0.0)
    assert sr.aggregate(col(3e38, 3e38), sr.MEDIAN)[0] == bits(np.inf)          # the even median's sum overflows: stated
    assert sr.aggregate(col(3e38, 1.0, 3e38), sr.MEDIAN)[0] == bits(3e38)
    assert sr.aggregate(col(-0.0, -0.0), sr.MEAN)[0] == bits(0.0)          # the chains start from +0
    X = np.ones((4, 3), np.float32)
    X[2, 1] = np.nan
    for agg in range(4):
        got = sr.aggregate(X, agg)
        assert got[1] == sr.NAN_BITS and (got[[0, 2]] == bits(1.0)).all()
    assert sr.aggregate(col(np.inf, -np.inf), sr.MEAN)[0] == sr.NAN_BITS          # a mean that is a NaN, without one in the data
    assert sr.aggregate(col(np.inf, -np.inf), sr.MEDIAN)[0] == sr.NAN_BITS and sr.aggregate(col(np.inf, -np.inf, 1.0), sr.MEDIAN)[0] == bits(1.0)


def test_the_chunked_order_shows():
    """cnt = 513: three chunks.  On this seeded data the contract's order and a single ascending chain differ in at least one output, so a
    comparison as bits can tell a kernel that sums the wrong way."""
    X = np.random.default_rng(ORDER_SEED).standard_normal((513, 130)).astype(np.float32)
    a, b = sr.mean_chunked(X), sr.mean_single_chain(X)
    assert (a.view(np.uint32) != b.view(np.uint32)).any()
    assert np.abs(a - b).max() < 1e-6


@pytest.mark.parametrize("mode", ["constant", "edge"])
@pytest.mark.parametrize("delay", [1, -1, 3, -7, 20, 21])
@pytest.mark.parametrize("n_steps", [1, 2, 5])
def test_stack_memory_against_pad_and_roll(n_steps, delay, mode):
    N, F = 20, 3
    X = small_integers(N, F, 3)
    got = sr.stack_memory(X, n_steps, delay, sr.CONSTANT if mode == "constant" else sr.EDGE, int(np.float32(-2.5).view(np.uint32))).view(np.float32)
    reach = (n_steps - 1) * abs(delay)
    padded = np.pad(X, ((reach, 0) if delay > 0 else (0, reach), (0, 0)), mode=mode, **(dict(constant_values=-2.5) if mode == "constant" else {}))
    want = []
    for s in range(n_steps):
        rolled = np.roll(padded, s * delay, axis=0)          # row t of the rolled plane is row t - s*delay
        want.append(rolled[reach:reach + N] if delay > 0 else rolled[:N])
    assert (got == np.concatenate(want, axis=1)).all()


def test_stack_memory_copies_bits():
    X = np.array([[0x7FC12345, 0xFFC00001], [0x80000000, 0x00000001]], np.uint32)
    got = sr.stack_memory(X, 2, 1, sr.CONSTANT, 0x7FC0BEEF)
    assert got.tolist() == [[0x7FC12345, 0xFFC00001, 0x7FC0BEEF, 0x7FC0BEEF], [0x80000000, 0x00000001, 0x7FC12345, 0xFFC00001]]


def test_lengths_straddle_the_thresholds():
    for t in sr.THRESHOLDS:
        assert {t, t + 1} <= set(sr.LENGTHS)
    assert {1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 512, 513} <= set(sr.LENGTHS) and sr.WHOLE in sr.N_SET
