"""Temporally constrained agglomerative segmentation of libjsgx.so on the GPU (include/jsgx.h section 17) against tests/agglo_ref.py: every
output is compared as int32 bits.  Every buffer is pitched and full of sentinels that must come back untouched: the padding of every
plane and list, the entries behind what a pair has, everything of a refused pair, the steps of the tree no merge took, the inputs, the
bytes around the scratch.  First the graph capture of a first launch; then the frame, feature, cluster and pair counts; the stretch
lengths on both sides of the threshold between the two merge kernels, mixed inside a workgroup; the boundary lists; the refused pairs;
the ties; the sums that overflow; the longest stretch; the scratch handed in with other contents; and the Python chain from audio to
beats, sub-beats and features a sub-beat."""
import functools
import hashlib

import numpy as np
import pytest

import agglo_ref as ar
from test_gpu_sync import FLOAT_SENTINEL, INT_SENTINEL, Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


_TREES = {}


def whole_tree(X):
    """(order, height) of the whole tree (k = 1) of a stretch, computed once for its bits: every k reads its answer from it."""
    key = (X.shape, hashlib.sha1(np.ascontiguousarray(X).tobytes()).hexdigest())
    if key not in _TREES:
        _TREES[key] = ar.cluster32(X, 1)[1:3]
    return _TREES[key]


def reference(Xp, bounds, count, k, pad, M, direct=False):
    """direct: every stretch clustered down to k as it stands (a long stretch that takes a few steps), not read from its whole tree."""
    return ar.segment(Xp, bounds, count, k, pad, max_bounds=M, tree=None if direct else lambda a, b: whole_tree(Xp[a:b]))


def run(jsg, torch, X, bounds, n_bounds, k, pad, what, max_out=None, tree=True, bounds_all=None, share_bounds=False, scratch=None, direct=False):
    """One launch over X float32 [pairs][N][F], bounds int32 [pairs][max_bounds] (share_bounds: [max_bounds], one list), n_bounds a list
    or None: every output against the restatement, and that nothing else was written.  scratch: (fill byte or int32 tensor, extra bytes).
    Returns per pair (n_out, out_bounds as written, n_segments), and the outputs' bits."""
    X = np.asarray(X, np.float32)
    P, N, F = X.shape
    bounds = np.asarray(bounds, np.int32).reshape((-1,) if share_bounds else (P, -1))
    M = bounds.shape[-1]
    S = max(1, min(N, (M if n_bounds is not None or bounds_all is None else bounds_all) + 2 * int(pad) - 1))
    max_out = max(1, min(N, S * k)) if max_out is None else max_out
    d_x = Guarded(torch, P, N, F, 3, 7, FLOAT_SENTINEL, 3)
    d_x.fill(torch, X)
    d_b = None
    if M:
        d_b = Guarded(torch, 1, 1 if share_bounds else P, M, 2, 0, INT_SENTINEL, 1)
        d_b.fill(torch, bounds)
    d_nb = None
    if n_bounds is not None:
        d_nb = torch.full((P + 3,), INT_SENTINEL, dtype=torch.int32, device="cuda")
        d_nb[1:1 + P] = torch.tensor(n_bounds, dtype=torch.int32)
    d_seg = Guarded(torch, 1, P, S + 1, 3, 0, INT_SENTINEL, 2)
    d_counts = torch.full((2, P + 4), INT_SENTINEL, dtype=torch.int32, device="cuda")
    d_out = Guarded(torch, 1, P, max_out, 2, 0, INT_SENTINEL, 1)
    d_order = Guarded(torch, 1, P, N, 4, 0, INT_SENTINEL, 2) if tree else None
    d_height = Guarded(torch, 1, P, N, 4, 0, FLOAT_SENTINEL, 2) if tree else None
    b_view = None if d_b is None else d_b.view[0, 0] if share_bounds else d_b.view[0]
    args = (d_x.f32, b_view, None if d_nb is None else d_nb[1:1 + P], d_seg.view[0], d_counts[0, 2:2 + P], d_out.view[0], d_counts[1, 2:2 + P])
    kw = dict(n_clusters=k, pad=pad, bounds_all=bounds_all, d_order=None if not tree else d_order.view[0], d_height=None if not tree else d_height.f32[0])
    need = jsg.agglomerative_scratch_bytes(*args, **kw)
    fill, extra = (0xA5, 0) if scratch is None else scratch
    d_scratch = torch.full((need + extra + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    if isinstance(fill, int):
        d_scratch[32:32 + need + extra] = fill
    else:          # what another launch left
        d_scratch[32:32 + need + extra] = fill.view(torch.uint8)[:need + extra]
    before = [t.clone() for t in (d_x.flat, None if d_b is None else d_b.flat, d_nb) if t is not None]
    jsg.agglomerative_launch(*args, d_scratch=d_scratch[32:32 + need + extra], **kw)
    torch.cuda.synchronize()
    assert (d_scratch[:32] == 0xEE).all() and (d_scratch[32 + need + extra:] == 0xEE).all(), "a byte next to the scratch was written"
    if extra and isinstance(fill, int):
        assert (d_scratch[32 + need:32 + need + extra] == fill).all(), "the scratch behind the stated size was written"
    assert d_seg.untouched() and d_out.untouched() and (not tree or (d_order.untouched() and d_height.untouched())), "a guard element was written"
    for t, was in zip([t for t in (d_x.flat, None if d_b is None else d_b.flat, d_nb) if t is not None], before):
        assert torch.equal(t, was), "an input was written"
    counts = d_counts.cpu().numpy()
    assert (counts[:, :2] == INT_SENTINEL).all() and (counts[:, 2 + P:] == INT_SENTINEL).all()
    seg, out = d_seg.view[0].cpu().numpy(), d_out.view[0].cpu().numpy()
    order = d_order.view[0].cpu().numpy() if tree else None
    height = d_height.view[0].cpu().numpy().view(np.uint32) if tree else None
    res = []
    for p in range(P):
        count = (M if bounds_all is None else bounds_all) if n_bounds is None else n_bounds[p]
        n_out, w_out, n_seg, u, steps = reference(X[p], bounds if share_bounds else bounds[p], count, k, pad, M, direct)
        assert (int(counts[1, 2 + p]), int(counts[0, 2 + p])) == (n_out, n_seg), (what, p, "n_out, n_segments", counts[:, 2 + p], n_out, n_seg)
        written = max(0, min(n_out, max_out))
        assert out[p, :written].tolist() == w_out[:written].tolist(), (what, p, "out_bounds", out[p, :written][:12], w_out[:12])
        assert (out[p, written:] == INT_SENTINEL).all(), (what, p, "an entry behind the boundaries was written")
        assert seg[p, :len(u)].tolist() == u.tolist() and (seg[p, len(u):] == INT_SENTINEL).all(), (what, p, "segments")
        if tree:
            w_order, w_height = np.full(N, INT_SENTINEL, np.int32), np.full(N, FLOAT_SENTINEL, np.uint32)
            for at, removed, bits in steps:
                w_order[at], w_height[at] = removed, bits
            bad = np.flatnonzero((order[p] != w_order) | (height[p] != w_height))
            assert bad.size == 0, (what, p, "tree", [(int(i), int(order[p, i]), int(w_order[i]), hex(height[p, i]), hex(w_height[i])) for i in bad[:4]])
        res.append((n_out, out[p, :written].copy(), n_seg))
    return res, (counts, seg, out, order, height), d_scratch[32:32 + need + extra]


@functools.lru_cache(maxsize=None)
def noise(P, N, F, seed=0):
    X = np.random.default_rng(seed).standard_normal((P, N, F)).astype(np.float32)
    X.setflags(write=False)
    return X


NONE = lambda P: np.zeros((P, 0), np.int32)


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The five kernels ("agglo_group" with its LDS asked for once per device) are launched here for the first time in the process, under
    capture, on one stream."""
    torch = torch_cuda
    P, N, F, k = 2, 300, 65, 3
    X = noise(P, N, F, 7)
    bounds, n_bounds = np.array([[5, 70, 71, 290], [100, 100, 200, 0]], np.int32), [4, 3]
    d_x = torch.zeros((P, N, F), dtype=torch.float32, device="cuda")
    d_b, d_nb = torch.from_numpy(bounds).cuda(), torch.tensor(n_bounds, dtype=torch.int32, device="cuda")
    d_seg, d_ns, d_no = (torch.full(s, INT_SENTINEL, dtype=torch.int32, device="cuda") for s in ((P, 6), (P,), (P,)))
    d_out, d_order = torch.full((P, 15), INT_SENTINEL, dtype=torch.int32, device="cuda"), torch.full((P, N), INT_SENTINEL, dtype=torch.int32, device="cuda")
    d_height = torch.zeros((P, N), dtype=torch.float32, device="cuda")
    d_scratch = torch.zeros((jsg.agglomerative_scratch_bytes(d_x, d_b, d_nb, d_seg, d_ns, d_out, d_no, n_clusters=k, d_order=d_order, d_height=d_height),), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.agglomerative_launch(d_x, d_b, d_nb, d_seg, d_ns, d_out, d_no, n_clusters=k, d_order=d_order, d_height=d_height, d_scratch=d_scratch, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert (d_no.cpu().numpy() == INT_SENTINEL).all() and (d_ns.cpu().numpy() == INT_SENTINEL).all()          # captured, not run
    d_x.copy_(torch.from_numpy(np.array(X)))
    g.replay()
    torch.cuda.synchronize()
    no, ns, seg, out, order, height = (t.cpu().numpy() for t in (d_no, d_ns, d_seg, d_out, d_order, d_height))
    for p in range(P):
        n_out, w_out, n_seg, u, steps = reference(X[p], bounds[p], n_bounds[p], k, True, 4)
        assert (no[p], ns[p]) == (n_out, n_seg) and out[p, :n_out].tolist() == w_out.tolist() and seg[p, :n_seg + 1].tolist() == u.tolist()
        assert all(order[p, at] == removed and height[p, at].view(np.uint32) == bits for at, removed, bits in steps) and len(steps) == u[-1] - u[0] - n_out


@pytest.mark.parametrize("N, F, P", ar.SHAPES, ids=[f"{N}x{F}x{P}" for N, F, P in ar.SHAPES])
def test_shapes(jsg, torch_cuda, N, F, P):
    """The whole plane as one stretch (librosa.segment.agglomerative) for every k, with and without the tree."""
    X = noise(P, N, F, 1)
    for k in ar.k_set(N):
        res, _, _ = run(jsg, torch_cuda, X, NONE(P), None, k, True, (N, F, P, k), tree=k != 2)
        assert [r[0] for r in res] == [min(k, N)] * P and all(r[1][0] == 0 for r in res)
    res, _, _ = run(jsg, torch_cuda, X, NONE(P), None, 1, False, (N, F, P, "no stretch"))
    assert [r[0] for r in res] == [0] * P


def test_the_planes_of_the_cpu_comparison(jsg, torch_cuda):
    """The planes on which the restatement gave scikit-learn's boundaries (tests/test_agglo_ref.py), the two longest ones."""
    for N, F, kind, seed in ar.PLANES:
        if N >= 257:
            run(jsg, torch_cuda, ar.plane(N, F, seed, kind)[None], NONE(1), None, 1, True, (N, F, kind))


@pytest.mark.parametrize("k", (1, 4, 64, 300))
def test_stretch_lengths(jsg, torch_cuda, k):
    """subsegment: the listed lengths as they stand (stretches of both kernels inside one group of four), sorted (the first groups are all
    short) and shuffled; then a list that leaves the plane's ends out."""
    F = 20
    for order, seed in ((ar.LENGTHS, 2), (tuple(sorted(ar.LENGTHS)), 3), (tuple(np.random.default_rng(3).permutation(ar.LENGTHS).tolist()), 4)):
        edges = np.cumsum(order)
        N = int(edges[-1])
        res, (_, seg, _, _, _), _ = run(jsg, torch_cuda, noise(2, N, F, seed), np.stack([edges[:-1], edges[:-1]]), None, k, True, ("lengths", k, order[:4]))
        assert np.diff(seg[0, :len(order) + 1]).tolist() == list(order) and res[0][0] == sum(min(k, n) for n in order)
        res, _, _ = run(jsg, torch_cuda, noise(2, N, F, seed), np.stack([edges[1:-2], edges[2:-1]]), None, k, False, ("lengths, no pad", k))
        assert res[0][0] == sum(min(k, n) for n in order[2:-2]) and res[0][1][0] == edges[1]


def test_boundary_lists(jsg, torch_cuda):
    torch = torch_cuda
    N, F, k = 257, 65, 3
    X = noise(3, N, F, 6)
    # repeats (the second row is a backtracked list: non-decreasing with runs), frames below 0 and above N, 0 and N given with pad
    lists = np.array([[5, 5, 9, 9, 9, 40, 200, 200], [0, 0, 0, 31, 31, 100, 100, 256], [-7, -1, 0, 3, 257, 258, 300, 1 << 30]], np.int32)
    res, _, _ = run(jsg, torch, X, lists, [8, 8, 8], k, True, "repeats and clipping")
    assert [r[0] for r in res] == [15, 10, 6]
    run(jsg, torch, X, lists, [8, 8, 8], k, False, "repeats and clipping, not padded")
    run(jsg, torch, X, np.array([[0, 100, N]] * 3, np.int32), [3, 2, 1], k, True, "0 and N given")
    run(jsg, torch, X, lists, None, k, True, "bounds_all", bounds_all=5)
    run(jsg, torch, X, lists, None, k, True, "bounds_all, no tree", bounds_all=0, tree=False)
    run(jsg, torch, X, lists[0], None, k, True, "one list for every pair", share_bounds=True)
    res, _, _ = run(jsg, torch, X, lists, [100, 8, 1 << 30], k, True, "n_bounds > max_bounds")
    assert res[0][0] == 15
    res, _, _ = run(jsg, torch, X, lists, [0, 0, 0], k, False, "an empty list")
    assert [r[0] for r in res] == [0, 0, 0]
    res, _, _ = run(jsg, torch, X, lists, [0, 1, 8], k, True, "an empty list, padded")
    assert [r[0] for r in res] == [3, 3, 6]
    # cut by max_out: the whole count is still reported
    res, _, _ = run(jsg, torch, X, lists, [8, 8, 8], k, True, "cut", max_out=7)
    assert [r[0] for r in res] == [15, 10, 6] and [len(r[1]) for r in res] == [7, 7, 6]
    run(jsg, torch, X, lists, [8, 8, 8], k, True, "cut to one", max_out=1)
    # more stretches than a step of the prefix sums takes (256), across its wavefronts
    many = np.sort(np.random.default_rng(8).integers(0, 1025, size=(2, 700)), axis=1).astype(np.int32)
    res, _, _ = run(jsg, torch, noise(2, 1025, 3, 9), many, [700, 513], 2, True, "700 boundaries")
    assert res[0][2] > 256


def test_refused_pairs(jsg, torch_cuda):
    """A negative count, a decreasing list, a NaN, an infinity among good pairs: n_out = -1 and the pair's rows untouched (run() checks
    them against the restatement, which leaves them full of sentinels)."""
    torch = torch_cuda
    N, F, k = 200, 9, 2
    lists = np.array([[5, 9, 40, 150]] * 5, np.int32)
    lists[1, 2] = 8
    X = np.array(noise(5, N, F, 10))
    X[2, 77, 3] = np.nan
    X[3, 149, 8] = -np.inf
    X[4, 2, 0] = X[4, 150, 1] = np.inf          # outside the frames 5 .. 149
    res, _, _ = run(jsg, torch, X, lists, [4, 4, 4, 4, -1], k, False, "refused, not padded")
    assert [(r[0], r[2]) for r in res] == [(6, 3), (-1, -1), (-1, 3), (-1, 3), (-1, -1)]
    res, _, _ = run(jsg, torch, X, lists, [-5, 2, 1, 3, 4], k, False, "refused, not padded, other counts")
    assert [(r[0], r[2]) for r in res] == [(-1, -1), (2, 1), (0, 0), (4, 2), (6, 3)]
    res, _, _ = run(jsg, torch, X, lists, [4, 4, 4, 4, 4], k, True, "refused, padded")
    assert [r[0] for r in res] == [10, -1, -1, -1, -1]
    X[2, 77, 3] = np.uint32(0xFFC00123).view(np.float32)          # a negative NaN with a payload, in the last lane's only feature
    X[3, 149, 8] = 1.0
    res, _, _ = run(jsg, torch, X[:, :, 3:4], lists, [4, 4, 4, 4, 4], k, False, "one feature")
    assert [r[0] for r in res] == [6, -1, -1, 6, 6]


def test_the_longest_stretch(jsg, torch_cuda):
    """A stretch of JSGX_AGGLO_MAX_STRETCH frames fills the LDS of "agglo_group" to its last byte; one frame more refuses the pair."""
    L = ar.MAX_STRETCH
    N = L + 70
    X = noise(2, N, 3, 11)
    res, _, _ = run(jsg, torch_cuda, X, np.array([[L], [L + 1]], np.int32), None, L - 4, True, "longest", direct=True)
    assert [(r[0], r[2]) for r in res] == [(L - 4 + 70, 2), (-1, 2)]
    res, _, _ = run(jsg, torch_cuda, X, np.array([[L + 1], [L]], np.int32), None, L - 4, True, "longest, the other pair", tree=False, direct=True)
    assert [r[0] for r in res] == [-1, L - 4 + 70]


def test_ties(jsg, torch_cuda):
    """A constant plane (every cost +0: the merges run from the left), -0 against +0, repeated frames."""
    torch = torch_cuda
    for N in (40, 200):
        for value in (0.0, -0.0, 2.5):
            res, (_, _, _, order, height), _ = run(jsg, torch, np.full((1, N, 9), value, np.float32), NONE(1), None, 5, True, ("constant", N, value))
            assert res[0][1].tolist() == [0] + list(range(N - 4, N)) and order[0, :N - 5].tolist() == list(range(1, N - 4)) and (height[0, :N - 5] == 0).all()
        mixed = np.zeros((1, N, 2), np.float32)
        mixed[0, 1::2] = -0.0
        res, _, _ = run(jsg, torch, mixed, NONE(1), None, 1, True, ("zeros of both signs", N))
        twice = np.repeat(noise(1, N // 2, 4, 12), 2, axis=1)
        res, (_, _, _, order, _), _ = run(jsg, torch, twice, NONE(1), None, N // 2, True, ("repeated frames", N))
        assert order[0, :N // 2].tolist() == list(range(1, N, 2)) and res[0][1].tolist() == list(range(0, N, 2))


def test_sums_that_overflow(jsg, torch_cuda):
    """Values near 3e38: the sums are infinities, the costs infinities and the NaN, which has one spelling and sorts last."""
    torch = torch_cuda
    res, (_, _, _, order, height), _ = run(jsg, torch, ar.OVERFLOW[None], NONE(1), None, 1, True, "overflow")
    assert order[0, :4].tolist() == [1, 3, 4, 2] and height[0, :4].tolist() == [0, 0, 0x7F800000, ar.NAN_BITS]
    rng = np.random.default_rng(13)
    for N in (50, 130):
        X = (rng.choice(np.array([3e38, -3e38, 2.9e38, 1e38], np.float32), size=(2, N, 5)) * rng.choice(np.array([1, 1, 1, 1e-38], np.float32), size=(2, N, 1))).astype(np.float32)
        run(jsg, torch, X, NONE(2), None, 1, True, ("overflow", N))
        run(jsg, torch, X, np.array([[N // 3, N // 2]] * 2, np.int32), None, 2, True, ("overflow, stretches", N))


def test_the_scratch_contents_do_not_show(jsg, torch_cuda):
    """Zeros, 0x5A, 0xFF and what a larger launch left in the scratch: the same bits every time, and nothing written around it."""
    torch = torch_cuda
    N, F, k = 300, 20, 4
    X = noise(3, N, F, 14)
    lists = np.array([[5, 64, 129, 290], [100, 100, 200, 0], [1, 2, 3, 4]], np.int32)
    _, _, left = run(jsg, torch, noise(3, 2 * N, F + 3, 15), np.array([[10, 300, 450, 599]] * 3, np.int32), [4, 4, 4], 2, True, "a larger launch")
    first = None
    for fill in (0x00, 0x5A, 0xFF, left):
        _, outs, _ = run(jsg, torch, X, lists, [4, 3, 4], k, True, ("scratch", fill if isinstance(fill, int) else "left"), scratch=(fill, 4096))
        first = outs if first is None else first
        for a, b in zip(first, outs):
            assert (a == b).all()


def test_python_layer(jsg, torch_cuda):
    torch = torch_cuda
    X = noise(3, 257, 20, 16)
    for k in (1, 6, 300):
        b, n = jsg.agglomerative(np.array(X[0]), k)
        want = reference(X[0], np.zeros(0, np.int32), 0, k, True, 0)
        assert int(n) == want[0] == min(k, 257) and b.cpu().numpy().tolist() == want[1].tolist()
        b, n, order, height = jsg.agglomerative(torch.from_numpy(np.array(X)).cuda(), k, return_tree=True)
        assert tuple(b.shape) == (3, min(k, 257)) and tuple(order.shape) == tuple(height.shape) == (3, 257)
        for p in range(3):
            w = reference(X[p], np.zeros(0, np.int32), 0, k, True, 0)
            assert int(n[p]) == w[0] and b[p].cpu().numpy().tolist() == w[1].tolist()
            o, h = order[p].cpu().numpy(), height[p].cpu().numpy().view(np.uint32)
            assert all(o[at] == r and h[at] == bits for at, r, bits in w[4]) and (o[len(w[4]):] == 0).all() and (h[len(w[4]):] == 0).all()
    frames = [-3, 10, 10, 80, 81, 200, 400]
    for pad in (True, False):
        b, n = jsg.subsegment(np.array(X[1]), frames, n_segments=4, pad=pad)
        w = reference(X[1], np.array(frames, np.int32), len(frames), 4, pad, len(frames))
        assert int(n) == w[0] == b.shape[0] and b.cpu().numpy().tolist() == w[1].tolist()
        d_frames, d_count = torch.tensor(frames + [7, 7], dtype=torch.int32, device="cuda"), torch.tensor([len(frames)], dtype=torch.int32, device="cuda")
        bd, nd = jsg.subsegment(torch.from_numpy(np.array(X)).cuda(), d_frames, n_segments=4, pad=pad, n_frames=d_count)
        assert nd.cpu().tolist() == [reference(X[p], np.array(frames, np.int32), len(frames), 4, pad, len(frames))[0] for p in range(3)]
        assert bd[1, :w[0]].cpu().numpy().tolist() == w[1].tolist()
        b2, n2 = jsg.subsegment(np.array(X[1]), frames, n_segments=4, pad=pad, max_bounds=5)
        assert int(n2) == w[0] and b2.cpu().numpy().tolist() == w[1][:5].tolist()
    with pytest.raises(jsg.JsgError, match="subsegment: frames must be non-decreasing"):
        jsg.subsegment(np.array(X[1]), [5, 3])
    with pytest.raises(jsg.JsgError):
        jsg.agglomerative(np.array(X[1]), 0)
    with pytest.raises(jsg.JsgError, match="without boundaries"):
        jsg.agglomerative(np.zeros((ar.MAX_STRETCH + 1, 1), np.float32), 2)


def test_python_chain(jsg, torch_cuda):
    """A short click track: beat_track_audio, then subsegment of the mel plane between the beats with the device's own list and count,
    then sync over the sub-beats with the device's own count, enqueued one after the other; the host is asked only at the end."""
    torch = torch_cuda
    sr_, hop, n_fft, n_mels = 22050, 512, 2048, 40
    x = np.random.default_rng(17).standard_normal(sr_ * 6).astype(np.float32) * 0.01
    period = sr_ // 2          # 120 beats a minute
    for at in range(period // 2, x.size - 256, period):
        x[at:at + 256] += np.hanning(256).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    bpm, beats, n_beats = jsg.beat_track_audio(xt, sr_, n_fft, hop, n_mels)
    S = jsg.mel_spectrogram_db(xt, sr_, n_fft, hop, n_mels)
    sub, n_sub = jsg.subsegment(S, beats, n_segments=2, n_frames=n_beats)
    out, seg, n_seg = jsg.sync(S, sub, aggregate="mean", pad=True, n_idx=n_sub)
    # only now the host looks
    nb, ns = int(n_beats), int(n_sub)
    host_beats, Sh = beats[:nb].cpu().numpy(), S.cpu().numpy()
    assert nb >= 2 and ns > nb
    want = reference(Sh, host_beats, nb, 2, True, beats.shape[-1])
    assert ns == want[0] and sub[:ns].cpu().numpy().tolist() == want[1].tolist()
    assert set(np.clip(host_beats, 0, Sh.shape[0]).tolist()) <= set(want[1].tolist()) | {Sh.shape[0]}
    import sync_ref as sr
    w_sync = sr.sync(Sh, want[1], ns, sr.MEAN, True, out.shape[0])
    assert int(n_seg) == w_sync[0] and (out[:w_sync[0]].cpu().numpy().view(np.uint32) == w_sync[2]).all()
    b2, n2 = jsg.subsegment(S, host_beats, n_segments=2)          # the host-list route on the same beats
    assert int(n2) == ns and torch.equal(b2, sub[:ns])
