"""Aggregation over segments and time-delay embedding of libjsgx.so on the GPU (include/jsgx.h sections 15 and 16) against
tests/sync_ref.py: every output is compared as int32 bits.  Every buffer is pitched and full of sentinels that must come back untouched:
the padding of every plane and list, the rows and entries behind what a pair has, everything of a refused pair, the inputs.  First the
graph capture of a first launch of either section; then the frame, feature and pair counts; the segment lengths on both sides of every
threshold between two forms of the kernel; the boundary lists; the values; the order of the mean; the stacking; and the Python chain
from a beat tracker's device lists to a recurrence plane."""
import functools

import numpy as np
import pytest

import sync_ref as sr

pytestmark = pytest.mark.gpu

AGGS = ("mean", "min", "max", "median")
INT_SENTINEL = -77
FLOAT_SENTINEL = 0x7FC0DEAD          # a NaN no kernel here produces: planes are compared as bits


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


class Guarded:
    """A flat int32 buffer full of `sentinel` and the view [pairs][rows][cols] inside it, `pad` extra elements a row and `pair_pad` extra a
    pair; .f32 is the same view as float32."""

    def __init__(self, torch, pairs, rows, cols, pad, pair_pad, sentinel, offset):
        pitch = cols + pad
        pair_pitch = rows * pitch + pair_pad
        self.flat = torch.full((pairs * pair_pitch + offset + 5,), sentinel, dtype=torch.int32, device="cuda")
        self.view = torch.as_strided(self.flat, (pairs, rows, cols), (pair_pitch, pitch, 1), storage_offset=offset)
        self.f32 = torch.as_strided(self.flat.view(torch.float32), (pairs, rows, cols), (pair_pitch, pitch, 1), storage_offset=offset)
        self.sentinel, self.offset = sentinel, offset

    def fill(self, torch, values):
        self.view.copy_(torch.from_numpy(np.array(values).view(np.int32).reshape(tuple(self.view.shape))))

    def untouched(self):
        """Whether the elements that are not the view's still hold the sentinel."""
        got = self.flat.cpu().numpy()
        inside = np.zeros(got.size, bool)
        P, R, W = self.view.shape
        sp, sr_, _ = self.view.stride()
        inside[(self.offset + np.arange(P)[:, None, None] * sp + np.arange(R)[None, :, None] * sr_ + np.arange(W)[None, None, :]).ravel()] = True
        return bool((got[~inside] == self.sentinel).all())


def run_sync(jsg, torch, X, bounds, n_bounds, agg, pad, max_segments=None, bounds_all=None, share_bounds=False):
    """One launch over X float32 [pairs][N][F], bounds int32 [pairs][max_bounds] (share_bounds: [max_bounds], one list), n_bounds a list
    or None -> per pair (n_segments, segments as written, out bits uint32 [rows written][F]) after checking that nothing else was
    written, and the same from the restatement."""
    X = np.asarray(X, np.float32)
    P, N, F = X.shape
    bounds = np.asarray(bounds, np.int32).reshape((-1,) if share_bounds else (P, -1))
    M = bounds.shape[-1]
    S = max(1, min(N, M + 2 * int(pad) - 1)) if max_segments is None else max_segments
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
    d_ns = torch.full((P + 4,), INT_SENTINEL, dtype=torch.int32, device="cuda")
    d_out = Guarded(torch, P, S, F, 5, 9, FLOAT_SENTINEL, 1)
    before = [t.clone() for t in (d_x.flat, None if d_b is None else d_b.flat, d_nb) if t is not None]
    b_view = None if d_b is None else d_b.view[0, 0] if share_bounds else d_b.view[0]
    jsg.sync_launch(d_x.f32, b_view, None if d_nb is None else d_nb[1:1 + P], d_seg.view[0], d_ns[2:2 + P], d_out.f32, aggregate=agg, pad=pad, bounds_all=bounds_all)
    torch.cuda.synchronize()
    assert d_seg.untouched() and d_out.untouched(), "a guard element was written"
    for t, was in zip([t for t in (d_x.flat, None if d_b is None else d_b.flat, d_nb) if t is not None], before):
        assert torch.equal(t, was), "an input was written"
    ns = d_ns.cpu().numpy()
    assert (ns[:2] == INT_SENTINEL).all() and (ns[2 + P:] == INT_SENTINEL).all()
    seg, out = d_seg.view[0].cpu().numpy(), d_out.view.cpu().numpy().view(np.uint32)
    got, want = [], []
    for p in range(P):
        n = int(ns[2 + p])
        rows = max(0, min(n, S))
        assert (seg[p, rows + 1 if rows else 0:] == INT_SENTINEL).all(), "an entry behind the segments was written"
        assert (out[p, rows:] == FLOAT_SENTINEL).all(), "a row behind the pair's segments was written"
        got.append((n, seg[p, :rows + 1 if rows else 0], out[p, :rows]))
        count = (M if bounds_all is None else bounds_all) if n_bounds is None else n_bounds[p]
        want.append(sr.sync(X[p], bounds if share_bounds else bounds[p], count, sr.AGGREGATES[agg], pad, S, max_bounds=M))
    return got, want


def check(got, want, what):
    for p, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (what, p, "n_segments", g[0], w[0])
        assert g[1].tolist() == w[1].tolist(), (what, p, "segments")
        bad = np.argwhere(g[2] != w[2])
        assert bad.size == 0, (what, p, "out", [(int(o), int(f), hex(g[2][o, f]), hex(w[2][o, f])) for o, f in bad[:4]])


def both(jsg, torch, X, bounds, n_bounds, agg, pad, what, **kw):
    got, want = run_sync(jsg, torch, X, bounds, n_bounds, agg, pad, **kw)
    check(got, want, (what, agg))
    return got


@functools.lru_cache(maxsize=None)
def noise(P, N, F, seed=0):
    X = np.random.default_rng(seed).standard_normal((P, N, F)).astype(np.float32)
    X.setflags(write=False)
    return X


def some_bounds(P, N, M, seed):
    """Sorted frames in -2..N+2 with repeats, [P][M], and a different count for every pair."""
    rng = np.random.default_rng(seed)
    b = np.sort(rng.integers(-2, N + 3, size=(P, M)), axis=1).astype(np.int32)
    return b, [M - 2 * p for p in range(P)]


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The two kernels of a median (the one with the tile in LDS, asked for once per device) and of a mean, and the stacking kernel, are
    launched here for the first time in the process, under capture, on one stream."""
    torch = torch_cuda
    P, N, F = 2, 300, 65
    X = noise(P, N, F, 7)
    bounds, n_bounds = np.array([[5, 70, 71, 290], [100, 100, 200, 0]], np.int32), [4, 3]
    for agg in ("median", "mean"):
        d_x = torch.zeros((P, N, F), dtype=torch.float32, device="cuda")
        d_b, d_nb = torch.from_numpy(bounds).cuda(), torch.tensor(n_bounds, dtype=torch.int32, device="cuda")
        d_seg, d_ns = torch.full((P, 6), INT_SENTINEL, dtype=torch.int32, device="cuda"), torch.full((P,), INT_SENTINEL, dtype=torch.int32, device="cuda")
        d_out = torch.zeros((P, 5, F), dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                jsg.sync_launch(d_x, d_b, d_nb, d_seg, d_ns, d_out, aggregate=agg, stream=side.cuda_stream)
        torch.cuda.synchronize()
        assert (d_ns.cpu().numpy() == INT_SENTINEL).all()          # captured, not run
        d_x.copy_(torch.from_numpy(np.array(X)))
        g.replay()
        torch.cuda.synchronize()
        ns, seg, out = d_ns.cpu().numpy(), d_seg.cpu().numpy(), d_out.cpu().numpy().view(np.uint32)
        for p in range(P):
            n, u, want = sr.sync(X[p], bounds[p], n_bounds[p], sr.AGGREGATES[agg], True, 5)
            assert ns[p] == n and seg[p, :n + 1].tolist() == u.tolist() and (out[p, :n] == want).all(), (agg, p)
    d_x = torch.zeros((P, N, F), dtype=torch.float32, device="cuda")
    d_out = torch.zeros((P, N, 3 * F), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.stack_memory_launch(d_x, d_out, n_steps=3, delay=2, mode="edge", stream=side.cuda_stream)
    torch.cuda.synchronize()
    d_x.copy_(torch.from_numpy(np.array(X)))
    g.replay()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    for p in range(P):
        assert (out[p] == sr.stack_memory(X[p], 3, 2, sr.EDGE)).all()


@pytest.mark.parametrize("N", sr.N_SET)
@pytest.mark.parametrize("F", sr.F_SET)
def test_shapes(jsg, torch_cuda, N, F):
    for P in (1, 3):
        bounds, n_bounds = some_bounds(P, N, 9, N + F)
        for agg in AGGS:
            both(jsg, torch_cuda, noise(P, N, F, 1), bounds, n_bounds, agg, True, (P, N, F))


@pytest.mark.parametrize("agg", AGGS)
def test_segment_lengths(jsg, torch_cuda, agg):
    """Every listed length, ascending (the first workgroups hold short segments only: a wavefront a segment) and shuffled (long and short
    ones share a workgroup: the four wavefronts together), and one segment that is the whole of N = 1025."""
    F = 65
    for order, seed in ((sr.LENGTHS, 2), (tuple(np.random.default_rng(3).permutation(sr.LENGTHS).tolist()), 4)):
        bounds, N = sr.bounds_of_lengths(order)
        got = both(jsg, torch_cuda, noise(1, N, F, seed), bounds[None], None, agg, True, ("lengths", order[:4]))
        assert np.diff(got[0][1]).tolist() == list(order)
    got = both(jsg, torch_cuda, noise(3, sr.WHOLE, F, 5), np.zeros((3, 0), np.int32), None, agg, True, "whole")
    assert [g[0] for g in got] == [1, 1, 1] and got[0][1].tolist() == [0, sr.WHOLE]


@pytest.mark.parametrize("agg", ("mean", "median"))
def test_boundary_lists(jsg, torch_cuda, agg):
    torch = torch_cuda
    N, F = 257, 65
    X = noise(3, N, F, 6)
    none = np.zeros((3, 0), np.int32)
    got = both(jsg, torch, X, none, None, agg, True, "none, padded")
    assert [g[0] for g in got] == [1, 1, 1]
    got = both(jsg, torch, X, none, None, agg, False, "none, not padded")
    assert [g[0] for g in got] == [0, 0, 0]
    # repeats (the second row is a backtracked list: non-decreasing with runs), frames below 0 and above N, 0 and N given with pad
    lists = np.array([[5, 5, 9, 9, 9, 40, 200, 200], [0, 0, 0, 31, 31, 100, 100, 256], [-7, -1, 0, 3, 257, 258, 300, 1 << 30]], np.int32)
    got = both(jsg, torch, X, lists, [8, 8, 8], agg, True, "repeats and clipping")
    assert got[0][1].tolist() == [0, 5, 9, 40, 200, N] and got[2][1].tolist() == [0, 3, N]
    both(jsg, torch, X, lists, [8, 8, 8], agg, False, "repeats and clipping, not padded")
    both(jsg, torch, X, np.array([[0, 100, N]] * 3, np.int32), [3, 2, 1], agg, True, "0 and N given")
    both(jsg, torch, X, lists, None, agg, True, "bounds_all", bounds_all=5)
    both(jsg, torch, X, lists[0], None, agg, True, "one list for every pair", share_bounds=True)
    # n_bounds beyond max_bounds; a pair with n_bounds = -1 and a pair whose list decreases among good pairs
    got = both(jsg, torch, X, lists, [100, 8, 1 << 30], agg, True, "n_bounds > max_bounds")
    assert got[0][0] == 5
    down = lists.copy()
    down[1, 5] = 30
    got = both(jsg, torch, X, down, [8, 8, 8], agg, True, "a decreasing list")
    assert [g[0] for g in got] == [5, -1, 2], got
    got = both(jsg, torch, X, lists, [-1, 8, 8], agg, True, "a refused row upstream")
    assert [g[0] for g in got] == [-1, 4, 2]
    got = both(jsg, torch, X, down, [8, 5, -1], agg, False, "the decrease behind the count")
    assert got[0][0] == 3 and got[1][0] == 1 and got[2][0] == -1
    # cut by max_segments: the whole count is still reported
    got = both(jsg, torch, X, lists, [8, 8, 8], agg, True, "cut", max_segments=3)
    assert [g[0] for g in got] == [5, 4, 2] and got[0][1].tolist() == [0, 5, 9, 40] and got[0][2].shape[0] == 3
    both(jsg, torch, X, lists, [8, 8, 8], agg, True, "cut to one", max_segments=1)
    # more boundaries than a step of the segment kernel takes (256), across its wavefronts
    many = np.sort(np.random.default_rng(8).integers(0, 1025, size=(2, 700)), axis=1).astype(np.int32)
    got = both(jsg, torch, noise(2, 1025, 3, 9), many, [700, 513], agg, True, "700 boundaries")
    assert got[0][0] > 256


@pytest.mark.parametrize("cnt", (1, 2, 3, 4, 64, 65, 256, 257))
def test_values(jsg, torch_cuda, cnt):
    """All equal; both zeros; infinities; denormals; an even median whose sum overflows; a NaN at one feature of one segment.  A plane of
    three segments of cnt frames, the middle one special, 65 features of which a few columns are set by hand."""
    inf, tiny = np.float32(np.inf), np.float32(1e-45)
    N, F = 3 * cnt, 65
    X = np.array(noise(1, N, F, 11))
    mid = X[0, cnt:2 * cnt]
    rng = np.random.default_rng(cnt)
    mid[:, 0] = 2.5
    mid[:, 1] = rng.choice(np.array([0.0, -0.0], np.float32), cnt)
    mid[:, 2] = rng.choice(np.array([inf, -inf, 1.0], np.float32), cnt)
    mid[:, 3] = rng.choice(np.array([tiny, -tiny, 3 * tiny, 0.0], np.float32), cnt)
    mid[:, 4] = 3e38
    mid[:, 5] = -0.0
    mid[:, 6] = inf
    mid[:, 64] = -inf
    mid[:cnt // 2, 9], mid[cnt // 2:, 9] = -inf, inf          # an even median of the two infinities is a NaN of its own making
    mid[cnt // 2, 7] = np.nan
    mid[0, 8] = np.uint32(0xFFC00123).view(np.float32)          # a negative NaN with a payload
    bounds = np.array([[cnt, 2 * cnt]], np.int32)
    for agg in AGGS:
        got = both(jsg, torch_cuda, X, bounds, None, agg, True, ("values", cnt))
        out = got[0][2]
        nan_at = np.flatnonzero(out[1] == sr.NAN_BITS).tolist()
        assert set(nan_at) >= {7, 8} and (out[[0, 2]] != sr.NAN_BITS).all(), (agg, nan_at)          # only that segment, only those features
        if agg != "mean":
            assert set(nan_at) <= ({2, 7, 8, 9} if agg == "median" and cnt % 2 == 0 else {7, 8})
            assert out[1, 0] == np.float32(2.5).view(np.uint32) and out[1, 5] == 0x80000000 and out[1, 64] == 0xFF800000
        if agg == "median" and cnt % 2 == 0:
            assert out[1, 4] == 0x7F800000          # fl(3e38 + 3e38) overflows: stated


def test_the_order_of_the_mean(jsg, torch_cuda):
    """cnt = 513 on the data of tests/test_sync_ref.py, where the chunked order and a single chain differ: the kernel has the chunked one."""
    from test_sync_ref import ORDER_SEED
    X = np.random.default_rng(ORDER_SEED).standard_normal((1, 513, 130)).astype(np.float32)
    got = both(jsg, torch_cuda, X, np.zeros((1, 0), np.int32), None, "mean", True, "order")
    chain = sr.mean_single_chain(X[0]).view(np.uint32)
    assert (got[0][2][0] != chain).any()
    # the same frames as the second of three segments, and among short ones: no other form gives other bits
    Y = np.concatenate([X[0, :100], X[0], X[0, :7]])[None]
    got2 = both(jsg, torch_cuda, Y, np.array([[100, 613]], np.int32), None, "mean", True, "order, inside")
    assert (got2[0][2][1] == got[0][2][0]).all()


@pytest.mark.parametrize("F", (1, 64, 65))
@pytest.mark.parametrize("n_steps", (1, 2, 5))
def test_stack_memory(jsg, torch_cuda, F, n_steps):
    torch = torch_cuda
    N = 37
    payload = 0x7FC01234
    fill = np.uint32(payload).view(np.float32)
    for P in (1, 3):
        X = np.array(noise(P, N, F, 12))
        X[0, 5, 0] = np.uint32(0xFFC00077).view(np.float32)          # a NaN with a payload in the data
        for delay in (1, -1, 3, -7, N, N + 1):
            for mode in ("constant", "edge"):
                d_x = Guarded(torch, P, N, F, 2, 5, FLOAT_SENTINEL, 3)
                d_x.fill(torch, X)
                d_out = Guarded(torch, P, N, n_steps * F, 3, 7, FLOAT_SENTINEL, 1)
                was = d_x.flat.clone()
                jsg.stack_memory_launch(d_x.f32, d_out.f32, n_steps=n_steps, delay=delay, mode=mode, constant_values=fill)
                torch.cuda.synchronize()
                assert d_out.untouched() and torch.equal(d_x.flat, was)
                out = d_out.view.cpu().numpy().view(np.uint32)
                for p in range(P):
                    want = sr.stack_memory(X[p], n_steps, delay, sr.CONSTANT if mode == "constant" else sr.EDGE, payload)
                    assert (out[p] == want).all(), (P, p, delay, mode, np.argwhere(out[p] != want)[:4].tolist())


def test_stack_memory_wide_and_long(jsg, torch_cuda):
    """A row wider than a workgroup's run (one frame a workgroup) and a plane of many runs, through the Python layer."""
    for N, F, n_steps, delay in ((9, 1025, 5, 2), (3000, 3, 2, -5)):
        X = np.array(noise(1, N, F, 13)[0])
        out = jsg.stack_memory(X, n_steps=n_steps, delay=delay, mode="constant", constant_values=-1.5)
        want = sr.stack_memory(X, n_steps, delay, sr.CONSTANT, int(np.float32(-1.5).view(np.uint32)))
        assert (out.cpu().numpy().view(np.uint32) == want).all()


def test_python_chain(jsg, torch_cuda):
    """beat_track on a device envelope, then sync with the device's idx and n_idx, equals the host-idx route on the same beats; then
    stack_memory and recurrence_matrix run on the result."""
    torch = torch_cuda
    T, F = 1025, 20
    rng = np.random.default_rng(14)
    env = (rng.random(T) * 0.1).astype(np.float32)
    env[::23] += 1.0
    feats = torch.from_numpy(np.array(noise(1, T, F, 15)[0])).cuda()
    beats, n_beats = jsg.beat_track(torch.from_numpy(env).cuda(), period=23)
    out_d, seg_d, n_d = jsg.sync(feats, beats, aggregate="median", n_idx=n_beats)
    n = int(n_beats)
    host_beats = beats[:n].cpu().numpy()
    assert n > 30 and (np.diff(host_beats) > 0).all()
    out_h, seg_h, n_h = jsg.sync(feats, host_beats, aggregate="median")
    k = int(n_h)
    assert int(n_d) == k == out_h.shape[0] == seg_h.shape[0] - 1
    assert torch.equal(out_d[:k].view(torch.int32), out_h.view(torch.int32)) and torch.equal(seg_d[:k + 1], seg_h)
    want = sr.sync(feats.cpu().numpy(), host_beats, n, sr.MEDIAN, True, k)
    assert (out_h.cpu().numpy().view(np.uint32) == want[2]).all() and seg_h.cpu().numpy().tolist() == want[1].tolist()
    # a batch of planes with one list, and the other aggregates by name
    batch = torch.stack([feats, feats * 2])
    for agg in AGGS:
        ob, sb, nb = jsg.sync(batch, host_beats, aggregate=agg)
        assert ob.shape == (2, k, F) and sb.shape == (2, k + 1) and nb.cpu().tolist() == [k, k]
        assert (ob[0].cpu().numpy().view(np.uint32) == sr.sync(feats.cpu().numpy(), host_beats, n, sr.AGGREGATES[agg], True, k)[2]).all()
    with pytest.raises(jsg.JsgError):
        jsg.sync(feats, [5, 3])
    stacked = jsg.stack_memory(out_h, n_steps=3, delay=1, mode="edge")
    assert stacked.shape == (k, 3 * F)
    assert (stacked.cpu().numpy().view(np.uint32) == sr.stack_memory(out_h.cpu().numpy(), 3, 1, sr.EDGE)).all()
    R = jsg.recurrence_matrix(stacked, k=5, width=1, metric="euclidean", sym=False, mode="connectivity")
    assert tuple(R.shape) == (k, k) and float(R.sum()) > 0
