"""Section 17 of include/jsgx.h restated in numpy: temporally constrained Ward clustering of the frames of a plane, every stretch between
two boundaries on its own.  `cluster32` is the definition operation by operation in float32 (a plain list of clusters whose costs are all
looked at again in every step); every result is compared with the GPU's as int32 bits.  `cluster64` is the same greedy merge in
float64, which is what scikit-learn's AgglomerativeClustering computes on a chain.  Both report the smallest relative gap between the
best and the second-best cost over their steps.  Also the shapes the GPU test runs."""
import numpy as np

import sync_ref as sr

F32 = np.float32
NAN_BITS = sr.NAN_BITS
MAX_STRETCH, SHORT, COPY_FRAMES = 16384, 64, 64          # JSGX_AGGLO_MAX_STRETCH, JSGX_AGGLO_SHORT, JSGX_AGGLO_COPY_FRAMES

# what the GPU test runs: every N with several F, every F with several N; (N, F, pairs)
N_SET = (1, 2, 3, 63, 64, 65, 257, 1025)
F_SET = (1, 63, 64, 65, 130)
PAIRS_SET = (1, 3)
SHAPES = ((1, 1, 3), (1, 130, 1), (2, 1, 1), (2, 64, 3), (3, 63, 1), (3, 65, 3), (63, 1, 3), (63, 130, 1), (64, 64, 3), (64, 65, 1), (65, 63, 3), (65, 1, 1),
          (257, 130, 3), (257, 64, 1), (1025, 65, 3), (1025, 1, 1))
# the planes of the CPU comparisons, one or two for every shape with a step to take: (N, F, kind, seed), the seeds chosen so that the
# best and the second-best cost of every step lie at least MIN_GAP apart, relatively (tests/test_agglo_ref.py asserts it)
MIN_GAP = 1e-4
PLANES = ((3, 63, "random", 1), (3, 65, "steps", 1), (63, 1, "random", 1), (63, 1, "steps", 2), (63, 130, "random", 8), (64, 64, "random", 4), (64, 64, "steps", 2),
          (64, 65, "random", 5), (65, 63, "random", 1), (65, 63, "steps", 27), (65, 1, "random", 1), (65, 1, "steps", 1), (257, 130, "growing", 56),
          (257, 64, "growing", 19), (1025, 65, "growing", 49), (1025, 1, "growing", 53), (2, 1, "random", 1), (2, 64, "random", 1))
# noise at the long sizes, for the float64 form against scikit-learn alone: (N, F, seed)
NOISE_PLANES = ((257, 64, 1), (257, 130, 2), (1025, 1, 3), (1025, 65, 4))
THRESHOLDS = (SHORT,)         # the length at which another kernel takes a stretch
# the stretch lengths of the mixed test: each side of the threshold, next to each other inside one workgroup of four stretches
LENGTHS = (1, 2, 64, 65, 3, 63, 64, 64, 65, 130, 1, 66, 7, 64, 257, 5)
# sums that overflow: two costs of 0, then an infinity (inf - finite) and the NaN (inf - inf)
OVERFLOW = np.array([[3e38, 1], [3e38, 1], [3e38, 2], [3e38, 2], [-3e38, 0]], F32)


def k_set(N):
    return (1, 2, 7, N, N + 3)


def fma32(a, b, acc):
    """float32 fmaf(a, b, acc), exactly (no overflow or underflow of the product in float64: float32 inputs)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)            # 48 bits: exact
        c = np.broadcast_to(acc, p.shape).astype(np.float64)
        s = c + p
        t = s - c
        lost = (c - (s - t)) + (p - t)           # TwoSum: c + p = s + lost exactly
        fix = (lost != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(lost > 0, np.inf, -np.inf)), s)      # round to odd
        return s.astype(F32)


def cost32(SA, mA, SB, mB):
    """The cost of the header for B pairs at once: SA, SB float32 [B][F] sums, mA, mB integer counts [B] -> float32 [B]."""
    SA, SB = np.atleast_2d(np.asarray(SA, F32)), np.atleast_2d(np.asarray(SB, F32))
    mA, mB = np.atleast_1d(np.asarray(mA, np.int64)), np.atleast_1d(np.asarray(mB, np.int64))
    B, F = SA.shape
    with np.errstate(all="ignore"):
        d = SA / mA.astype(F32)[:, None] - SB / mB.astype(F32)[:, None]
        q = np.zeros((B, 64), F32)
        for f0 in range(0, F, 64):
            c = d[:, f0:f0 + 64]
            q[:, :c.shape[1]] = fma32(c, c, q[:, :c.shape[1]])
        lanes = np.arange(64)
        for s in (32, 16, 8, 4, 2, 1):
            q = q + q[:, lanes ^ s]
        w = (mA.astype(F32) * mB.astype(F32)) / (mA + mB).astype(F32)
        c = (w * q[:, 0]).astype(F32)
    return np.where(np.isnan(c), np.uint32(NAN_BITS).view(F32), c).astype(F32)


def cost64(SA, mA, SB, mB):
    d = SA / mA - SB / mB
    return mA * mB / (mA + mB) * float(np.dot(d, d))


def _gap(costs):
    """The relative gap between the least and the second least of a step's costs."""
    if len(costs) < 2:
        return np.inf
    two = np.partition(np.asarray(costs, np.float64), 1)[:2]
    return float((two[1] - two[0]) / two[1]) if two[1] > 0 and np.isfinite(two[1]) else 0.0


def cluster32(X, k):
    """One stretch X float32 [L][F] -> (the starts of the min(k, L) clusters, order [L - min(k, L)], height as float32, the smallest gap)."""
    X = np.asarray(X, F32)
    L = X.shape[0]
    starts, counts, sums = list(range(L)), [1] * L, [X[t].copy() for t in range(L)]
    costs = list(cost32(X[:-1], np.ones(L - 1), X[1:], np.ones(L - 1))) if L > 1 else []
    order, height, gap = [], [], np.inf
    pair = lambda i: cost32(sums[i], counts[i], sums[i + 1], counts[i + 1])[0]
    while len(starts) > min(k, L):
        c = np.array(costs, F32)
        i = int(np.argmin(sr.key(c)))           # the first of the least keys: a tie goes to the lower frame
        gap = min(gap, _gap(c))
        order.append(starts[i + 1])
        height.append(c[i])
        with np.errstate(all="ignore"):
            sums[i] = sums[i] + sums[i + 1]
        counts[i] += counts[i + 1]
        del starts[i + 1], counts[i + 1], sums[i + 1], costs[i]
        if i > 0:
            costs[i - 1] = pair(i - 1)
        if i < len(starts) - 1:
            costs[i] = pair(i)
    return np.array(starts, np.int32), np.array(order, np.int32), np.array(height, F32), gap


def cluster64(X, k):
    """The same greedy merge in float64: (starts, order, the smallest gap)."""
    X = np.asarray(X, np.float64)
    L = X.shape[0]
    starts, counts, sums = list(range(L)), [1] * L, [X[t].copy() for t in range(L)]
    pair = lambda i: cost64(sums[i], counts[i], sums[i + 1], counts[i + 1])
    costs = [pair(i) for i in range(L - 1)]
    order, gap = [], np.inf
    while len(starts) > min(k, L):
        i = int(np.argmin(costs))
        gap = min(gap, _gap(costs))
        order.append(starts[i + 1])
        sums[i] = sums[i] + sums[i + 1]
        counts[i] += counts[i + 1]
        del starts[i + 1], counts[i + 1], sums[i + 1], costs[i]
        if i > 0:
            costs[i - 1] = pair(i - 1)
        if i < len(starts) - 1:
            costs[i] = pair(i)
    return np.array(starts, np.int32), np.array(order, np.int32), gap


def cut_tree(order, k, L):
    """The starts of min(k, L) clusters from the whole tree (k = 1) of a stretch of L frames: frame 0 and what its last k - 1 steps removed."""
    kk = min(k, L)
    return np.sort(np.concatenate(([0], order[L - kk:]))).astype(np.int32)


def segment(X, bounds, n_bounds, k, pad, max_bounds=None, tree=None):
    """One pair: X float32 [N][F] -> (n_out, out_bounds, n_segments, u, steps) with steps a list of (index, removed frame, height bits) over
    all stretches.  n_out = -1: a refused pair (n_segments = -1 where the list is refused).  tree: a function (u0, u1) -> (order, height)
    of the whole tree of a stretch, where the caller keeps them; else the stretch is clustered here."""
    X = np.asarray(X, F32)
    N = X.shape[0]
    n, u = sr.segments(bounds, n_bounds, N, pad, max_bounds)
    none = np.zeros(0, np.int32)
    if n < 0:
        return -1, none, -1, none, []
    if n == 0:
        return 0, none, 0, none, []
    if not np.isfinite(X[u[0]:u[-1]]).all() or (np.diff(u) > MAX_STRETCH).any():
        return -1, none, n, u, []
    out, steps = [], []
    for o in range(n):
        u0, L = int(u[o]), int(u[o + 1] - u[o])
        if tree is None:
            starts, order, height, _ = cluster32(X[u0:u0 + L], k)
        else:
            order, height = tree(u0, u0 + L)
            starts, order, height = cut_tree(order, k, L), order[:L - min(k, L)], height[:L - min(k, L)]
        out.append(u0 + starts)
        steps += [(u0 + j, u0 + int(b), int(np.array(h, F32).view(np.uint32))) for j, (b, h) in enumerate(zip(order, height))]
    out = np.concatenate(out).astype(np.int32)
    return len(out), out, n, u, steps


def plane(N, F, seed, kind="random"):
    """A test plane float32 [N][F]: normal noise; a few constant sections with a little noise on top; or every feature growing
    geometrically at a rate of its own.  Among hundreds of costs of noise two of the least lie closer than 1e-4 at some step whatever
    the seed (the costs of F features concentrate around F); the growing plane spreads them over many decades."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.standard_normal((N, F)).astype(F32)
    if kind == "growing":
        rate = 1.02 + 0.01 * rng.uniform(size=F)
        return (rng.uniform(0.5, 1.5, size=F)[None, :] * rate[None, :] ** np.arange(N)[:, None]).astype(F32)
    edges = np.sort(rng.choice(np.arange(1, N), size=min(N - 1, 5), replace=False)) if N > 1 else np.zeros(0, np.int64)
    level = rng.standard_normal((len(edges) + 1, F)) * 4
    return (level[np.searchsorted(edges, np.arange(N), side="right")] + 0.1 * rng.standard_normal((N, F))).astype(F32)
