"""The pairwise cost and dynamic time warping of libjsgx.so on the GPU (include/jsgx.h sections 2 and 3) against tests/dtw_ref.py, bit for
bit (NaN positions equal, all other bits equal): D, the path, its length and the total over shapes around the tile edges on costs with
many ties and with none; weights, subseq and bands on both sides of the connectivity rule; three pairs in pitched buffers with poisoned
padding; a NaN cell that stays in its pair; graph capture of a first launch; the total alone under subseq, without a scratch; the cost
kernel per metric around its own tile edges, with 16-byte stores beside a scalar tail, feature counts around its panel and at the limit,
three pairs in one pitched plane, a shared sequence and a zero vector; and the Python layer end to end."""
import functools

import numpy as np
import pytest

import dtw_ref as dr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
ISENTINEL = np.int32(-77777)
WEIGHTS = [(None, None), ((1, 1.5, 0.75), (0, 0.25, 0.5))]
COSTS = {"integers": dr.integer_costs, "floats": dr.float_costs}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def tiles(jsg):
    name, rows, cols, launches, threads, lds = jsg.dtw_plan(1, 1)
    assert name == "dtw_tiles" and launches == 2 and threads == 64
    return rows, cols


@functools.lru_cache(maxsize=None)
def reference(kind, N, M, seed, weights, subseq, band):
    """(C, D, path or None, total) of the restatement; computed once and shared."""
    C = COSTS[kind](N, M, seed)
    wm, wa = WEIGHTS[weights]
    D = dr.dtw32(C, wm, wa, subseq, band)
    path, total = dr.backtrace32(D, C, wm, wa, subseq)
    for a in (C, D):
        a.setflags(write=False)
    return C, D, path, total


def guarded(torch, planes, rows, cols, pad, dtype, sentinel, offset):
    """A flat buffer full of `sentinel` and the view [planes][rows][cols] inside it with `pad` extra elements per row and 3 * pad per plane."""
    pitch, plane = cols + pad, rows * (cols + pad) + 3 * pad
    flat = torch.full((planes * plane + offset + 5,), sentinel, dtype=dtype, device="cuda")
    return flat, torch.as_strided(flat, (planes, rows, cols), (plane, pitch, 1), storage_offset=offset)


def untouched(flat, view, sentinel, offset):
    got = flat.cpu().numpy()
    inside = np.zeros(got.size, bool)
    P, R, W = view.shape
    inside[(offset + np.arange(P)[:, None, None] * view.stride(0) + np.arange(R)[None, :, None] * view.stride(1) + np.arange(W)[None, None, :]).ravel()] = True
    return bool((got[~inside] == sentinel).all() if sentinel == sentinel else np.isnan(got[~inside]).all())


def run(jsg, torch, costs, *, weights=0, subseq=False, band=0, pad=0):
    """One launch over the pairs `costs` (equal shapes) in pitched buffers full of sentinels -> (D [P][N][M], path_i, path_j [P][N + M - 1],
    path_len [P], total [P]) as numpy, after checking that nothing outside these was written."""
    P, (N, M) = len(costs), costs[0].shape
    L = N + M - 1
    wm, wa = WEIGHTS[weights]
    fc, d_cost = guarded(torch, P, N, M, pad, torch.float32, float("nan"), 3)
    d_cost.copy_(torch.from_numpy(np.stack(costs)))
    fd, d_acc = guarded(torch, P, N, M, 2 * pad, torch.float32, float(SENTINEL), 1)
    fi, d_pi = guarded(torch, 1, P, L, pad, torch.int32, int(ISENTINEL), 2)
    fj, d_pj = guarded(torch, 1, P, L, pad, torch.int32, int(ISENTINEL), 2)
    d_len = torch.full((P + 2,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_total = torch.full((P + 2,), float(SENTINEL), dtype=torch.float32, device="cuda")
    jsg.dtw_launch(d_cost, d_acc, weights_mul=wm, weights_add=wa, subseq=subseq, band=band, d_path_i=d_pi[0], d_path_j=d_pj[0], d_path_len=d_len[1:P + 1],
                   d_total=d_total[1:P + 1])
    torch.cuda.synchronize()
    assert untouched(fd, d_acc, SENTINEL, 1) and untouched(fi, d_pi, ISENTINEL, 2) and untouched(fj, d_pj, ISENTINEL, 2), "a guard element was written"
    assert untouched(fc, d_cost, float("nan"), 3) and dr.same_bits(d_cost.cpu().numpy(), np.stack(costs)), "the cost was written"
    n, t = d_len.cpu().numpy(), d_total.cpu().numpy()
    assert n[0] == n[-1] == ISENTINEL and t[0] == t[-1] == SENTINEL
    return d_acc.cpu().numpy(), d_pi[0].cpu().numpy(), d_pj[0].cpu().numpy(), n[1:P + 1], t[1:P + 1]


def check_pair(got, p, want, what):
    D, pi, pj, n, total = got
    _, wD, wpath, wtotal = want
    assert dr.same_bits(D[p], wD), (what, "D", np.argwhere(D[p].view(np.uint32) != wD.view(np.uint32))[:4])
    if wpath is None:       # no path: the length says so and nothing else is written
        assert n[p] == -1 and (pi[p] == ISENTINEL).all() and (pj[p] == ISENTINEL).all() and total[p] == SENTINEL, (what, n[p])
        return
    L = len(wpath)
    assert n[p] == L and (pi[p, :L] == wpath[:, 0]).all() and (pj[p, :L] == wpath[:, 1]).all(), (what, "path", n[p], L)
    assert (pi[p, L:] == ISENTINEL).all() and (pj[p, L:] == ISENTINEL).all() and dr.same_bits(total[p:p + 1], np.asarray([wtotal])), (what, "total")


def shapes(tiles):
    TR, TC = tiles
    return [(1, 1), (1, 3 * TC + 2), (2 * TR + 1, 1), (2, 2), (TR - 1, TC - 1), (TR, TC), (TR + 1, TC + 1), (2 * TR + 1, TC + 1), (2, 3 * TC + 2),
            (TR - 1, TC + 1), (TR + 1, TC - 1), (2 * TR + 1, 3 * TC + 2), (TR, 2), (1, TC)]


@pytest.mark.parametrize("kind", list(COSTS))
@pytest.mark.parametrize("index", range(14))
def test_shapes_around_the_tile_edges(jsg, torch_cuda, tiles, index, kind):
    """N from {1, 2, TR-1, TR, TR+1, 2TR+1} and M from {1, 2, TC-1, TC, TC+1, 3TC+2}: 1 x 1, one row, one column, and up to six tile
    anti-diagonals; small-integer costs (about a quarter of the cells tie, a -0 among them) and random floats (no ties)."""
    N, M = shapes(tiles)[index]
    assert jsg.dtw_plan(N, M)[3] == -(-N // tiles[0]) + -(-M // tiles[1])
    want = reference(kind, N, M, index, 0, False, 0)
    check_pair(run(jsg, torch_cuda, [want[0]]), 0, want, (N, M, kind))


@pytest.mark.parametrize("kind", list(COSTS))
@pytest.mark.parametrize("subseq", [False, True])
@pytest.mark.parametrize("weights", [0, 1])
def test_weights_and_subseq(jsg, torch_cuda, tiles, weights, subseq, kind):
    TR, TC = tiles
    for N, M in ((TR + 1, TC + 1), (2 * TR + 1, TC - 1), (3, 2 * TC + 5)):
        want = reference(kind, N, M, 40 + weights, weights, subseq, 0)
        check_pair(run(jsg, torch_cuda, [want[0]], weights=weights, subseq=subseq), 0, want, (N, M, kind, weights, subseq))


@pytest.mark.parametrize("shape, band, connected", [((65, 200), 1, False), ((65, 200), 2, True), ((10, 100), 4, False), ((10, 100), 5, True)])
def test_bands_on_both_sides_of_the_connectivity_rule(jsg, torch_cuda, shape, band, connected):
    for kind in COSTS:
        want = reference(kind, *shape, 7, 0, False, band)
        assert (want[2] is not None) == connected
        check_pair(run(jsg, torch_cuda, [want[0]], band=band), 0, want, (shape, band, kind))


def test_a_band_that_leaves_whole_tiles_outside(jsg, torch_cuda, tiles):
    TR, TC = tiles
    N, M = 4 * TR + 3, 2 * TC + 9
    for band in (2, 200):
        want = reference("floats", N, M, 9, 1, False, band)
        assert want[2] is not None and np.isinf(want[1][:TR, TC:2 * TC]).all() == (band == 2)
        check_pair(run(jsg, torch_cuda, [want[0]], weights=1, band=band, pad=3), 0, want, (N, M, band))


@pytest.mark.parametrize("subseq", [False, True])
def test_three_pairs_in_padded_buffers(jsg, torch_cuda, tiles, subseq):
    """The result is a function of the cell: a pair computes what it computes alone, whatever the pitches; the poisoned padding stays."""
    TR, TC = tiles
    N, M = TR + 5, TC + 9
    wants = [reference(kind, N, M, seed, 1, subseq, 0) for kind, seed in (("floats", 1), ("integers", 2), ("floats", 3))]
    got = run(jsg, torch_cuda, [w[0] for w in wants], weights=1, subseq=subseq, pad=7)
    for p, want in enumerate(wants):
        check_pair(got, p, want, (p, subseq))


def test_a_nan_cell_stays_in_its_pair(jsg, torch_cuda, tiles):
    TR, TC = tiles
    N, M = TR + 9, TC + 9
    clean = [reference("floats", N, M, seed, 0, False, 0) for seed in (11, 12, 13)]
    bad = np.array(clean[1][0])
    bad[TR - 1, TC - 1] = np.nan                 # the last cell of the first tile: its NaN runs down the diagonal (a NaN v_0 stays) into the end cell
    D = dr.dtw32(bad)
    want_bad = (bad, D) + dr.backtrace32(D, bad)
    assert want_bad[2] is None and np.isnan(D[-1, -1]) and not np.isnan(D[:TR - 1]).any()
    got = run(jsg, torch_cuda, [clean[0][0], bad, clean[2][0]], pad=2)
    check_pair(got, 0, clean[0], "before the NaN pair")
    check_pair(got, 1, want_bad, "the NaN pair")
    check_pair(got, 2, clean[2], "after the NaN pair")
    # a NaN in the last row under subseq: no path, whatever the rest of the row holds
    late = np.array(clean[0][0])
    late[N - 1, 5] = np.nan
    D = dr.dtw32(late, subseq=True)
    want_late = (late, D) + dr.backtrace32(D, late, subseq=True)
    assert want_late[2] is None and np.isnan(D[-1]).sum() < M
    ok = reference("floats", N, M, 11, 0, True, 0)
    got = run(jsg, torch_cuda, [late, ok[0]], subseq=True)
    check_pair(got, 0, want_late, "a NaN in the last row")
    check_pair(got, 1, ok, "next to it")


def test_graph_capture_of_a_first_launch(jsg, torch_cuda, tiles):
    """A captured first launch (several kernels on the one stream), replayed twice with changed input."""
    torch = torch_cuda
    TR, TC = tiles
    N, M = TR + 3, TC + 5           # four tiles, three anti-diagonals, the backtrace
    L = N + M - 1
    d_cost = torch.zeros((2, N, M), dtype=torch.float32, device="cuda")
    d_acc = torch.full((2, N, M), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_pi, d_pj = (torch.full((2, L), int(ISENTINEL), dtype=torch.int32, device="cuda") for _ in range(2))
    d_len = torch.full((2,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_total = torch.full((2,), float(SENTINEL), dtype=torch.float32, device="cuda")
    kw = dict(weights_mul=WEIGHTS[1][0], weights_add=WEIGHTS[1][1], d_path_i=d_pi, d_path_j=d_pj, d_path_len=d_len, d_total=d_total)
    d_scratch = torch.empty((jsg.dtw_scratch_bytes(d_cost, d_acc, **kw) // 4,), dtype=torch.int32, device="cuda")
    assert d_scratch.numel() == 2 * 2 * L
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.dtw_launch(d_cost, d_acc, d_scratch=d_scratch, stream=side.cuda_stream, **kw)
    torch.cuda.synchronize()
    assert (d_len.cpu().numpy() == ISENTINEL).all() and (d_acc.cpu().numpy() == SENTINEL).all()      # captured, not run
    for seeds in ((21, 22), (23, 24)):
        wants = [reference("floats", N, M, seed, 1, False, 0) for seed in seeds]
        d_cost.copy_(torch.from_numpy(np.stack([w[0] for w in wants])))
        d_pi.fill_(int(ISENTINEL)), d_pj.fill_(int(ISENTINEL))
        g.replay()
        torch.cuda.synchronize()
        got = (d_acc.cpu().numpy(), d_pi.cpu().numpy(), d_pj.cpu().numpy(), d_len.cpu().numpy(), d_total.cpu().numpy())
        for p, want in enumerate(wants):
            check_pair(got, p, want, ("replay", seeds, p))


def test_forward_alone_needs_no_scratch(jsg, torch_cuda):
    torch = torch_cuda
    want = reference("integers", 70, 300, 5, 0, False, 0)
    d_cost = torch.from_numpy(np.array(want[0])).cuda()
    d_acc = torch.empty_like(d_cost)
    assert jsg.dtw_scratch_bytes(d_cost, d_acc) == 0
    jsg.dtw_launch(d_cost, d_acc)
    d_total = torch.full((1,), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_acc2 = torch.empty_like(d_cost)
    jsg.dtw_launch(d_cost, d_acc2, d_total=d_total)
    torch.cuda.synchronize()
    assert dr.same_bits(d_acc.cpu().numpy(), want[1]) and dr.same_bits(d_acc2.cpu().numpy(), want[1])
    assert dr.same_bits(d_total.cpu().numpy(), np.asarray([want[3]]))


def test_total_alone_under_subseq_needs_no_scratch(jsg, torch_cuda, tiles):
    """d_total without paths and without a path length, subseq on: the backtrace kernel reduces the last row to its lowest minimal column
    and walks without recording, so the scratch is 0 bytes and none is passed.  Integer costs: the minimum of the last row is tied."""
    torch = torch_cuda
    TR, TC = tiles
    N, M = 3, 2 * TC + 5
    C, D, path, total = reference("integers", N, M, 40, 0, True, 0)
    assert path is not None and (D[N - 1] == D[N - 1].min()).sum() > 1 and path[-1][1] == int(np.argmin(D[N - 1])) < M - 1
    d_cost = torch.from_numpy(np.array(C)).cuda()
    d_acc = torch.full((N, M), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_total = torch.full((3,), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert jsg.dtw_scratch_bytes(d_cost, d_acc, subseq=True, d_total=d_total[1:2]) == 0
    assert jsg.dtw_plan(N, M, backtrack=False)[3] + 1 == jsg.dtw_plan(N, M)[3]
    none = torch.empty((0,), dtype=torch.int32, device="cuda")
    assert none.numel() == 0
    jsg.dtw_launch(d_cost, d_acc, subseq=True, d_total=d_total[1:2], d_scratch=none)
    torch.cuda.synchronize()
    t = d_total.cpu().numpy()
    assert t[0] == t[2] == SENTINEL and dr.same_bits(t[1:2], np.asarray([total])), (t, total)
    assert dr.same_bits(d_acc.cpu().numpy(), D)


# ---------------------------------------------------------------------------------------------------- the cost kernel
def features(N, K, seed):
    return np.random.default_rng(seed).standard_normal((N, K)).astype(np.float32)


@pytest.mark.parametrize("K", [1, 3, 12, 129])
@pytest.mark.parametrize("metric", list(dr.METRICS))
def test_cdist_per_metric_around_its_tile_edges(jsg, torch_cuda, metric, K):
    """N and M around the cost kernel's tile (its plan names it), K below, at and across its panel of 32 features; padded frames and a
    padded cost plane whose poison stays."""
    torch = torch_cuda
    name, threads, lds = jsg.cdist_plan(64, 64, K, metric=metric)
    T = jsg.capix.CDIST_TILE
    assert name == f"cdist_{T}x{T}" and threads == 256
    for N, M in ((1, 1), (T - 1, T + 1), (T, T), (2 * T + 1, T - 1), (3, 2 * T + 2)):
        X, Y = features(N, K, N), features(M, K, 1000 + M)
        fx, d_x = guarded(torch, 1, N, K, 3, torch.float32, float("nan"), 1)
        fy, d_y = guarded(torch, 1, M, K, 1, torch.float32, float("nan"), 2)
        d_x.copy_(torch.from_numpy(X[None])), d_y.copy_(torch.from_numpy(Y[None]))
        for pad, offset in ((0, 0), (5, 3)):        # 16-byte stores where the plane allows them, single ones where it does not
            fc, d_cost = guarded(torch, 1, N, M, pad, torch.float32, float(SENTINEL), offset)
            jsg.cdist_launch(d_x[0], d_y[0], d_cost[0], metric=metric)
            torch.cuda.synchronize()
            assert untouched(fc, d_cost, SENTINEL, offset), "a guard element was written"
            assert dr.same_bits(d_cost[0].cpu().numpy(), dr.cost32(X, Y, metric)), (metric, K, N, M, pad)


def aligned_planes(torch, planes, rows, cols, offset):
    """A flat buffer full of SENTINEL and the view [planes][rows][cols] inside it whose every row starts on a 16-byte boundary: the row pitch
    is cols rounded up to a multiple of 4, the plane pitch a multiple of 4 with two guard rows of 4 behind the plane, `offset` (0 or 4)
    elements in front."""
    pitch = -(-cols // 4) * 4
    plane = rows * pitch + 8
    flat = torch.full((offset + planes * plane + 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
    view = torch.as_strided(flat, (planes, rows, cols), (plane, pitch, 1), storage_offset=offset)
    assert view.data_ptr() % 16 == 0 and pitch % 4 == 0 and plane % 4 == 0
    return flat, view


@pytest.mark.parametrize("metric", list(dr.METRICS))
def test_cdist_16_byte_stores_beside_a_scalar_tail(jsg, torch_cuda, metric):
    """Planes aligned to 16 bytes whose m is no multiple of 4: a row goes out as 16-byte stores up to its last whole group of four and as
    single stores behind it (3, 2 and 3 of them), in the tile's last lanes, in a second tile, and in a third; the guard elements that
    close each row's pitch stay."""
    torch = torch_cuda
    T, K = jsg.capix.CDIST_TILE, 12
    for N, M in ((5, T - 1), (T + 1, T + 2), (3, 2 * T + 3)):
        assert M % 4 != 0
        X, Y = features(N, K, 10 + N), features(M, K, 2000 + M)
        want = dr.cost32(X, Y, metric)
        d_x, d_y = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        for offset in (0, 4):
            fc, d_cost = aligned_planes(torch, 1, N, M, offset)
            jsg.cdist_launch(d_x, d_y, d_cost[0], metric=metric)
            torch.cuda.synchronize()
            assert untouched(fc, d_cost, SENTINEL, offset), ("a guard element was written", metric, N, M, offset)
            assert dr.same_bits(d_cost[0].cpu().numpy(), want), (metric, N, M, offset)


@pytest.mark.parametrize("K", [31, 32, 33, 64, 1024])
def test_cdist_feature_counts_around_the_panel(jsg, torch_cuda, K):
    """K one below, at and one above the panel of 32 features, two whole panels, and the limit 1024 (32 panels: the longest fmaf chain)."""
    torch = torch_cuda
    T = jsg.capix.CDIST_TILE
    assert K <= jsg.capix.CDIST_MAX_FEATURES
    N, M = T + 1, T - 1
    X, Y = features(N, K, 3000 + K), features(M, K, 4000 + K)
    d_x, d_y = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    for metric in dr.METRICS:
        fc, d_cost = guarded(torch, 1, N, M, 5, torch.float32, float(SENTINEL), 3)
        jsg.cdist_launch(d_x, d_y, d_cost[0], metric=metric)
        torch.cuda.synchronize()
        assert untouched(fc, d_cost, SENTINEL, 3), "a guard element was written"
        assert dr.same_bits(d_cost[0].cpu().numpy(), dr.cost32(X, Y, metric)), (metric, K)


@pytest.mark.parametrize("aligned", [False, True])
def test_cdist_three_pairs_in_one_pitched_guarded_plane(jsg, torch_cuda, aligned):
    """pairs = 3 written into one pitched buffer full of sentinels, with single stores (an odd offset and pitch) and with 16-byte stores
    beside a scalar tail (every row of every plane on a 16-byte boundary); X is one sequence for every pair (a pair pitch of 0), Y is
    padded per frame and per pair with poison."""
    torch = torch_cuda
    T, K = jsg.capix.CDIST_TILE, 12
    N, M = T + 5, T + 9
    X, Ys = features(N, K, 21), np.stack([features(M, K, s) for s in (22, 23, 24)])
    d_x = torch.from_numpy(X).cuda()
    fy, d_y = guarded(torch, 3, M, K, 3, torch.float32, float("nan"), 2)
    d_y.copy_(torch.from_numpy(Ys))
    for metric in dr.METRICS:
        if aligned:
            offset = 4
            fc, d_cost = aligned_planes(torch, 3, N, M, offset)
        else:
            offset = 3
            fc, d_cost = guarded(torch, 3, N, M, 5, torch.float32, float(SENTINEL), offset)
        jsg.cdist_launch(d_x, d_y, d_cost, metric=metric)
        torch.cuda.synchronize()
        assert untouched(fc, d_cost, SENTINEL, offset), ("a guard element was written", metric)
        assert untouched(fy, d_y, float("nan"), 2) and dr.same_bits(d_y.cpu().numpy(), Ys), "y was written"
        got = d_cost.cpu().numpy()
        for p in range(3):
            assert dr.same_bits(got[p], dr.cost32(X, Ys[p], metric)), (metric, p, aligned)


def test_cdist_with_a_shared_sequence_and_pairs(jsg, torch_cuda):
    """A pair pitch of 0: one X for every pair (query by example); three Y."""
    torch = torch_cuda
    X, Ys = features(70, 12, 1), np.stack([features(65, 12, s) for s in (2, 3, 4)])
    for metric in dr.METRICS:
        got = jsg.cdist(X, Ys, metric).cpu().numpy()
        assert got.shape == (3, 70, 65)
        for p in range(3):
            assert dr.same_bits(got[p], dr.cost32(X, Ys[p], metric)), (metric, p)
        d_x = torch.from_numpy(X).cuda()
        cost = torch.empty((3, 70, 65), dtype=torch.float32, device="cuda")
        jsg.cdist_launch(d_x[None].expand(3, 70, 12), torch.from_numpy(Ys).cuda(), cost, metric=metric)
        assert np.array_equal(cost.cpu().numpy().view(np.uint32), got.view(np.uint32))


def test_cdist_special_values(jsg, torch_cuda):
    """A zero vector under cosine gives 1 (scipy: NaN); NaN and infinity go through the operations."""
    X = features(5, 7, 1)
    X[1] = 0
    X[2, 3] = np.nan
    X[3, 0] = np.inf
    Y = features(6, 7, 2)
    Y[4] = 0
    for metric in dr.METRICS:
        got = jsg.cdist(X, Y, metric).cpu().numpy()
        assert dr.same_bits(got, dr.cost32(X, Y, metric)), metric
    got = jsg.cdist(X, Y, "cosine").cpu().numpy()
    assert (got[1] == 1).all() and (got[[0, 4], 4] == 1).all() and np.isnan(got[2]).all()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_end_to_end_a_sequence_against_itself_at_half_speed(jsg, torch_cuda):
    """Y[2i] = Y[2i+1] = X[i]: the total is 0 and the path is exactly (i, 2i), (i, 2i+1)."""
    X = features(150, 20, 5)
    Y = np.repeat(X, 2, axis=0)
    D, wp = jsg.dtw(X, Y, metric="sqeuclidean")
    wp = wp.cpu().numpy()
    assert D.shape == (150, 300) and float(D[-1, -1]) == 0 and wp.dtype == np.int32
    assert wp.tolist() == [[i // 2, i] for i in range(300)]
    C = dr.cost32(X, Y, "sqeuclidean")
    assert dr.same_bits(D.cpu().numpy(), dr.dtw32(C))
    # the same from a cost plane, and without the path
    D2 = jsg.dtw(C=C, backtrack=False)
    assert dr.same_bits(D2.cpu().numpy(), D.cpu().numpy())
    # a query inside a longer recording
    D3, wp3 = jsg.dtw(X[40:60], X, metric="euclidean", subseq=True)
    wp3 = wp3.cpu().numpy()
    assert wp3.tolist() == [[i, 40 + i] for i in range(20)] and float(D3[-1, 59]) == 0


def test_no_path_raises(jsg, torch_cuda):
    C = dr.float_costs(10, 100, 1)
    with pytest.raises(jsg.JsgError, match="no warping path"):
        jsg.dtw(C=C, band=4)
    D, wp = jsg.dtw(C=C, band=5)
    assert wp[0].tolist() == [0, 0] and wp[-1].tolist() == [9, 99]
    with pytest.raises(jsg.JsgError, match="band and subseq"):
        jsg.dtw(C=C, band=5, subseq=True)
    D, wps = jsg.dtw(C=np.stack([C, C]))
    assert D.shape == (2, 10, 100) and len(wps) == 2 and wps[0].tolist() == wps[1].tolist()
