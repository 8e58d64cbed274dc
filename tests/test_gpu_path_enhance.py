"""Path enhancement of libjsgx.so on the GPU (include/jsgx.h section 10) against tests/path_enhance_ref.py, bit for bit (NaN positions equal,
all other bits equal): shapes around the tile edges with the n = 7 bank (extents 7, 8 and 9: both parities of the centre rule, a reach
beyond the small planes) on affinities and on small integers, the n = 51 bank, the largest reach, a single slope-1 filter, callers' lists
(an empty filter, a tap beyond the reach, a zero weight, a broken table), zero_mean with and without the clip, negative cells, a NaN and an
infinity that stay where the taps take them and in their pair, three pairs in pitched buffers with poisoned padding, graph capture of a
first launch, and recurrence_matrix -> path_enhance -> rqa under one captured graph."""
import functools

import numpy as np
import pytest

import path_enhance_ref as pr
import rqa_ref as rr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
PLANES = {"floats": pr.affinity_plane, "integers": pr.integer_plane}
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 70), (63, 64), (64, 64), (65, 65), (64, 130), (130, 64), (129, 67), (200, 131)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=None)
def bank(n, **kw):
    """(tap_w, tap_at, filter_first, reach_i, reach_j) of the package's builder; built once and shared."""
    import jadespectrogram_amd as jsg
    b = jsg.path_enhance_filters(n, **dict(kw))
    for a in b[:3]:
        a.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def plane(kind, N, M, seed):
    R = PLANES[kind](N, M, seed)
    R.setflags(write=False)
    return R


def guarded(torch, planes, rows, cols, pad, sentinel, offset):
    """A flat buffer full of `sentinel` and the view [planes][rows][cols] inside it with `pad` extra elements per row and 3 * pad per plane."""
    pitch, size = cols + pad, rows * (cols + pad) + 3 * pad
    flat = torch.full((planes * size + offset + 5,), sentinel, dtype=torch.float32, device="cuda")
    return flat, torch.as_strided(flat, (planes, rows, cols), (size, pitch, 1), storage_offset=offset)


def untouched(flat, view, sentinel, offset):
    got = flat.cpu().numpy()
    inside = np.zeros(got.size, bool)
    P, R, W = view.shape
    inside[(offset + np.arange(P)[:, None, None] * view.stride(0) + np.arange(R)[None, :, None] * view.stride(1) + np.arange(W)[None, None, :]).ravel()] = True
    return bool((got[~inside] == sentinel).all() if sentinel == sentinel else np.isnan(got[~inside]).all())


def run(jsg, torch, planes, taps, *, clip=True, pad=0, reach=None):
    """One launch over the pairs `planes` (equal shapes) in pitched buffers full of sentinels -> out [P][N][M] as numpy, after checking
    that nothing outside it was written and that the inputs are as they were."""
    tap_w, tap_at, first, ri, rj = taps
    ri, rj = (ri, rj) if reach is None else reach
    P, (N, M) = len(planes), planes[0].shape
    fr, d_r = guarded(torch, P, N, M, pad, float("nan"), 3)
    d_r.copy_(torch.from_numpy(np.stack(planes)))
    fo, d_out = guarded(torch, P, N, M, 2 * pad, float(SENTINEL), 1)
    d_w, d_at, d_first = (torch.from_numpy(np.concatenate([a, a[:0]])).cuda() for a in (np.asarray(tap_w, np.float32), np.asarray(tap_at, np.int32), np.asarray(first, np.int32)))
    jsg.path_enhance_launch(d_r, d_w, d_at, d_first, d_out, reach_i=ri, reach_j=rj, clip=clip)
    torch.cuda.synchronize()
    assert untouched(fo, d_out, SENTINEL, 1), "a guard element was written"
    assert untouched(fr, d_r, float("nan"), 3) and pr.same_bits(d_r.cpu().numpy(), np.stack(planes)), "the plane was written"
    assert pr.same_bits(d_w.cpu().numpy(), tap_w) and np.array_equal(d_at.cpu().numpy(), tap_at) and np.array_equal(d_first.cpu().numpy(), first), "the list was written"
    return d_out.cpu().numpy()


def check(got, want, what):
    assert pr.same_bits(got, want), (what, np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))[:4])


def reference(R, taps, clip=True, reach=None):
    tap_w, tap_at, first, ri, rj = taps
    ri, rj = (ri, rj) if reach is None else reach
    return pr.path_enhance32(R, tap_w, tap_at, first, ri, rj, clip)


def test_the_plan(jsg):
    """64 x 64 tiles of 256 lanes; the window's rows are 1 (mod 4) words so that eight rows fall on different banks; two workgroups fit a
    compute unit at reach 32 and the largest window fits the LDS."""
    for reach in (0, 1, 25, 32, 64):
        name, tr, tc, threads, lds = jsg.path_enhance_plan(reach, reach)
        assert (name, tr, tc, threads) == ("path_enhance_tiles", 64, 64, 256) and lds == 4 * (64 + 2 * reach) * (((64 + 2 * reach + 3) // 4) * 4 + 1)
    assert 2 * jsg.path_enhance_plan(32, 32)[4] <= 163840 and jsg.path_enhance_plan(64, 64)[4] == 148224


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The first launch of the kernel in this process, which is why this test stands in front of every other one that launches: the window
    of the largest reach (148 224 bytes; the n = 51 bank's 65 016 would stay under the 65 536 a kernel gets without asking) is more dynamic
    LDS than a kernel gets without asking, the launcher asks once per device at the first launch, and asking is no stream operation, so
    it works under capture.  (test_gpu_lag.py runs earlier and launches other kernels.)"""
    torch = torch_cuda
    taps = bank(101)[:3] + (64, 64)
    assert jsg.path_enhance_plan(taps[3], taps[4])[4] == 148224 > 65536
    N, M = 67, 69
    d_r = torch.zeros((2, N, M), dtype=torch.float32, device="cuda")
    d_out = torch.full((2, N, M), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_w, d_at, d_first = (torch.from_numpy(np.array(a)).cuda() for a in taps[:3])
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.path_enhance_launch(d_r, d_w, d_at, d_first, d_out, reach_i=taps[3], reach_j=taps[4], stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == SENTINEL).all()          # captured, not run
    planes = [plane("floats", N, M, seed) for seed in (21, 22)]
    d_r.copy_(torch.from_numpy(np.stack(planes)))
    g.replay()
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    for p, R in enumerate(planes):
        check(got[p], reference(R, taps), ("replay", p))


def plan_shapes():
    """What the plan's tile makes edge cases, beside SHAPES: a last tile of one row or column behind two full ones with a plane narrower
    than a lane's four columns, two full tiles each way, and one cell short of and beyond a tile."""
    import jadespectrogram_amd as jsg
    tr, tc = jsg.path_enhance_plan(3, 3)[1:3]
    return [(2 * tr + 1, 3), (3, 2 * tc + 1), (2 * tr, 2 * tc), (tr - 1, tc + 1), (tr + 1, tc - 1)]


N_PLAN_SHAPES = 5


@pytest.mark.parametrize("kind", list(PLANES))
@pytest.mark.parametrize("index", range(len(SHAPES) + N_PLAN_SHAPES))
def test_shapes_around_the_tile_edges(jsg, torch_cuda, index, kind):
    shapes = SHAPES + plan_shapes()
    assert len(shapes) == len(SHAPES) + N_PLAN_SHAPES
    N, M = shapes[index]
    taps = bank(7)
    assert taps[3] == taps[4] == 3 and len(taps[2]) == 8          # the 9 x 9 tables' outermost entries are zero
    R = plane(kind, N, M, index)
    check(run(jsg, torch_cuda, [R], taps)[0], reference(R, taps), (N, M, kind))


def test_the_default_bank_of_51(jsg, torch_cuda):
    taps = bank(51)
    assert taps[3] == taps[4] == 31 and 3000 < len(taps[0]) < 3400
    R = plane("floats", 130, 131, 51)
    got = run(jsg, torch_cuda, [R], taps)[0]
    check(got, reference(R, taps), "n = 51")
    assert (got >= 0).all() and got.max() > 0


@pytest.mark.parametrize("shape", [(70, 70), (129, 67)])
def test_the_largest_reach(jsg, torch_cuda, shape):
    """The n = 101 bank (a 128 x 128 table at slope 2: taps out to 63) launched with the largest reach, 64, and a caller's list with taps
    at the four corners of that reach."""
    taps = bank(101)
    assert taps[3] == taps[4] == 63
    R = plane("floats", *shape, 101)
    check(run(jsg, torch_cuda, [R], taps, reach=(64, 64))[0], reference(R, taps, reach=(64, 64)), ("n = 101", shape))
    corners = (np.array([0.5, 0.25, 2.0, 1.0, 0.125], np.float32), pr.pack([64, 64, -64, -64, 0], [64, -64, 64, -64, 0]), np.array([0, 5], np.int32), 64, 64)
    Ri = plane("integers", *shape, 102)
    want = reference(Ri, corners)
    assert (want != 0.125 * Ri).any()
    check(run(jsg, torch_cuda, [Ri], corners)[0], want, ("corners", shape))


def test_a_single_slope_one_filter(jsg, torch_cuda):
    taps = bank(31, n_filters=1, max_ratio=1.0, min_ratio=1.0)
    assert len(taps[0]) == 29 and taps[3] == taps[4] == 14
    R = plane("floats", 129, 67, 31)
    check(run(jsg, torch_cuda, [R], taps)[0], reference(R, taps), "slope 1")


def test_callers_lists(jsg, torch_cuda):
    """An empty filter (acc = +0: with the clip off it lifts every negative cell to +0), a tap beyond the reach (skipped), a zero weight (a
    tap like any other), runs of every length in both directions, and a table whose filter_first leaves 0..n_taps or descends."""
    rng = np.random.default_rng(77)
    R = np.array(plane("integers", 70, 75, 9))
    R[rng.random(R.shape) < 0.2] *= -1
    w = (rng.integers(-8, 9, 40) / 8.0).astype(np.float32)
    w[5] = 0.0
    di = np.concatenate([np.full(11, -2), np.full(9, 0), [1, 1, 1], [2, 2], np.arange(-3, 4), rng.integers(-3, 4, 8)])
    dj = np.concatenate([np.arange(5, -6, -1), np.arange(4, -5, -1), [0, 1, 2], [3, 1], np.arange(3, -4, -1), rng.integers(-5, 6, 8)])
    at = pr.pack(di, dj)
    for first in ([0, 11, 11, 25, 40], [0, 40], [0, 20, 20, 20, 40], [-5, 17, 99], [30, 10, 40]):
        for clip in (True, False):
            for reach in ((3, 5), (2, 3), (0, 0)):
                taps = (w, at, np.array(first, np.int32), *reach)
                want = reference(R, taps, clip)
                check(run(jsg, torch_cuda, [R], taps, clip=clip)[0], want, (first, clip, reach))
                assert not np.signbit(want[want == 0]).any()
    empty = reference(R, (w, at, np.array([0, 11, 11, 25, 40], np.int32), 3, 5), False)
    assert (empty >= 0).all() and (reference(R, (w, at, np.array([0, 11, 25, 40], np.int32), 3, 5), False) < 0).any()


def test_zero_mean_and_negative_cells(jsg, torch_cuda):
    """zero_mean makes the tables dense and their sums negative where the plane is bright off the diagonals: with the clip these cells are
    +0, never -0; without it they stay negative."""
    taps = bank(7, zero_mean=True)
    assert len(taps[0]) == 49 + 4 * 64 + 2 * 81 and (taps[0] < 0).any()
    R = np.array(plane("floats", 65, 70, 3))
    R[20:30, 20:30] = 1.0
    R[40:44] *= -1.0
    for clip in (True, False):
        want = reference(R, taps, clip)
        got = run(jsg, torch_cuda, [R], taps, clip=clip)[0]
        check(got, want, ("zero_mean", clip))
        assert (want < 0).any() != clip and not np.signbit(got[got == 0]).any()


def test_a_nan_and_an_infinity_stay_in_their_pair(jsg, torch_cuda):
    taps = bank(7)
    N, M = 69, 73
    clean = [plane("floats", N, M, seed) for seed in (11, 12, 13)]
    bad = np.array(clean[1])
    bad[63, 64], bad[5, 70] = np.nan, np.inf
    want = reference(bad, taps)
    # exactly the cells that a tap connects to the special cell
    di, dj = pr.unpack(taps[1])
    nan_at = np.zeros((N, M), bool)
    inf_at = np.zeros((N, M), bool)
    for a, b in zip(di, dj):
        if 0 <= 63 - a < N and 0 <= 64 - b < M:
            nan_at[63 - a, 64 - b] = True
        if 0 <= 5 - a < N and 0 <= 70 - b < M:
            inf_at[5 - a, 70 - b] = True
    assert np.array_equal(np.isnan(want), nan_at) and np.array_equal(np.isposinf(want), inf_at & ~nan_at) and nan_at.sum() > 20
    got = run(jsg, torch_cuda, [clean[0], bad, clean[2]], taps, pad=2)
    check(got[0], reference(clean[0], taps), "before the special pair")
    check(got[1], want, "the special pair")
    check(got[2], reference(clean[2], taps), "after the special pair")


def test_three_pairs_in_padded_buffers(jsg, torch_cuda):
    taps = bank(7)
    N, M = 69, 73
    planes = [plane(kind, N, M, seed) for kind, seed in (("floats", 1), ("integers", 2), ("floats", 3))]
    got = run(jsg, torch_cuda, planes, taps, pad=7)
    for p, R in enumerate(planes):
        check(got[p], reference(R, taps), p)


def test_recurrence_matrix_to_path_enhance_to_rqa_under_one_graph(jsg, torch_cuda):
    """200 frames [A, B, A]: the affinity plane, its enhancement and the alignment, enqueued on one stream under one captured graph; score
    and path equal the restatements chained from the plane the device made.  The python layer gives the same enhancement."""
    torch = torch_cuda
    rng = np.random.default_rng(0)
    A, B = rng.standard_normal((60, 12)).astype(np.float32), rng.standard_normal((80, 12)).astype(np.float32)
    X = torch.from_numpy(np.concatenate([A, B, A])).cuda()
    N = 200
    taps = bank(7)
    rec = jsg.recurrence_matrix(X, mode="affinity")         # eager once: the shapes, and the tables the layers keep per device
    assert tuple(rec.shape) == (N, N)
    k = jsg.knn_default_k(N, 1)
    d_index = torch.empty((N, k), dtype=torch.int32, device="cuda")
    d_dist = torch.empty((N, k), dtype=torch.float32, device="cuda")
    d_knn_scratch = torch.empty((max(1, jsg.knn_scratch_bytes(X, X, d_index, d_dist, width=1) // 4),), dtype=torch.int32, device="cuda")
    d_bw = torch.empty((1,), dtype=torch.float32, device="cuda")
    d_rec, d_enh, d_score = (torch.full((N, N), float(SENTINEL), dtype=torch.float32, device="cuda") for _ in range(3))
    d_pi, d_pj = (torch.full((1, N), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    d_len = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_w, d_at, d_first = (torch.from_numpy(np.array(a)).cuda() for a in taps[:3])
    kw = dict(d_path_i=d_pi, d_path_j=d_pj, d_path_len=d_len)
    d_scratch = torch.empty((jsg.rqa_scratch_bytes(d_enh, d_score, **kw) // 4,), dtype=torch.int32, device="cuda")
    # the bandwidth as recurrence_matrix computes it, taken from the eager run: a number on the device, not part of the captured work
    jsg.knn_launch(X, X, d_index, d_dist, width=1, d_scratch=d_knn_scratch)
    last = d_dist[:, k - 1]
    v = torch.sort(last[torch.isfinite(last)]).values
    d_bw[0] = 0.5 * (v[(v.numel() - 1) // 2] + v[v.numel() // 2])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            s = side.cuda_stream
            jsg.knn_launch(X, X, d_index, d_dist, width=1, d_scratch=d_knn_scratch, stream=s)
            jsg.recurrence_launch(d_index, d_dist, d_rec, mode="affinity", d_bandwidth=d_bw, stream=s)
            jsg.path_enhance_launch(d_rec, d_w, d_at, d_first, d_enh, reach_i=taps[3], reach_j=taps[4], stream=s)
            jsg.rqa_launch(d_enh, d_score, d_scratch=d_scratch, stream=s, **kw)
    torch.cuda.synchronize()
    assert (d_score.cpu().numpy() == SENTINEL).all() and int(d_len.cpu()) == -7
    g.replay()
    torch.cuda.synchronize()
    R = d_rec.cpu().numpy()
    assert pr.same_bits(R, rec.cpu().numpy())
    enhanced = reference(R, taps)
    check(d_enh.cpu().numpy(), enhanced, "enhanced")
    S, _ = rr.rqa32(enhanced, 1.0, 1.0, True)
    path, end, total = rr.backtrace32(S, enhanced, 1.0, 1.0, True)
    L = int(d_len.cpu())
    assert rr.same_bits(d_score.cpu().numpy(), S) and L == len(path) >= 50
    assert np.array_equal(d_pi.cpu().numpy()[0, :L], path[:, 0]) and np.array_equal(d_pj.cpu().numpy()[0, :L], path[:, 1])
    lag = path[:, 0] - path[:, 1]
    assert abs(np.median(lag)) == 140, path          # the repeat: most of the run lies on the diagonal of the second A against the first
    # the python layer: the same bank, the same plane; an `out` of the caller's; a batch
    check(jsg.path_enhance(rec, 7).cpu().numpy(), enhanced, "path_enhance")
    out = torch.empty((2, N, N), dtype=torch.float32, device="cuda")
    assert jsg.path_enhance(torch.stack([rec, rec]), 7, out=out) is out
    check(out[1].cpu().numpy(), enhanced, "batch")
    with pytest.raises(jsg.JsgError, match="out overlaps r"):
        jsg.path_enhance(rec, 7, out=rec)
