"""The k nearest frames, the recurrence plane and the neighbour aggregation of libjsgx.so on the GPU (include/jsgx.h sections 6 to 8)
against tests/knn_ref.py, bit for bit: indices equal, distances equal with NaN positions equal, nothing outside the pitched outputs
touched.  Shapes on both sides of every strip and tile edge the plan reports, N != M both ways; feature counts around the panel and at
the limit; k from 1 to 256 and above the number of candidates; widths; the three metrics; eight kinds of data (massive ties, none,
every tile inserting, nothing inserting, NaN in y, NaN in x, +inf, zero vectors); every column split with identical bits; three pairs
in pitched buffers and a shared y; the distances against the plane of jsgx_cdist_launch; graph capture of a first launch of the three
operations; every mode of the recurrence plane with and without sym and diag and a bandwidth of 0 and of NaN; nn_filter by mean and by
weights; and the Python layer end to end."""
import functools

import numpy as np
import pytest

import knn_ref as kr
from test_gpu_dtw import guarded, untouched

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
ISENTINEL = np.int32(-77777)
METRICS = ("sqeuclidean", "euclidean", "cosine")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def edge(jsg):
    """The one form of the forward kernel, over every k and a spread of shapes: its strip rows are its tile columns are `edge`."""
    plans = {jsg.knn_plan(n, m, 3, k)[:2] + jsg.knn_plan(n, m, 3, k)[3:4] for n in (1, 64, 65, 4096, 65536) for m in (1, 64, 65, 65536) for k in (1, 64, 65, 256)}
    assert plans == {("knn_64", jsg.capix.KNN_STRIP, jsg.capix.KNN_THREADS)} and jsg.capix.KNN_STRIP == jsg.capix.KNN_TILE == 64
    return jsg.capix.KNN_STRIP


@functools.lru_cache(maxsize=None)
def data(kind, N, M, K, seed):
    X, Y = kr.frames(kind, N, M, K, seed)
    X.setflags(write=False), Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def reference(kind, N, M, K, seed, k, width, metric):
    """(X, Y, index, dist) of the restatement; computed once and shared."""
    X, Y = data(kind, N, M, K, seed)
    index, dist = kr.knn32(X, Y, k, width, metric)
    index.setflags(write=False), dist.setflags(write=False)
    return X, Y, index, dist


def run(jsg, torch, Xs, Ys, k, *, width=0, metric="euclidean", split=0, pad=0):
    """One launch over the pairs (Xs[p], Ys[p]) (one Y: shared, a pair pitch of 0) in pitched buffers full of sentinels -> (index, dist)
    [P][N][k] as numpy, after checking that nothing outside these was written and that the inputs are as they were."""
    P, (N, K), M = len(Xs), Xs[0].shape, Ys[0].shape[0]
    fx, d_x = guarded(torch, P, N, K, pad, torch.float32, float("nan"), 3)
    d_x.copy_(torch.from_numpy(np.stack(Xs)))
    fy, d_y = guarded(torch, len(Ys), M, K, 2 * pad, torch.float32, float("nan"), 1)
    d_y.copy_(torch.from_numpy(np.stack(Ys)))
    fi, d_i = guarded(torch, P, N, k, pad, torch.int32, int(ISENTINEL), 2)
    fd, d_d = guarded(torch, P, N, k, 3 * pad, torch.float32, float(SENTINEL), 1)
    jsg.knn_launch(d_x, d_y, d_i, d_d, width=width, metric=metric, split=split)
    torch.cuda.synchronize()
    assert untouched(fi, d_i, ISENTINEL, 2) and untouched(fd, d_d, SENTINEL, 1), "a guard element was written"
    assert untouched(fx, d_x, float("nan"), 3) and untouched(fy, d_y, float("nan"), 1) and kr.same_bits(d_x.cpu().numpy(), np.stack(Xs)) and kr.same_bits(d_y.cpu().numpy(), np.stack(Ys)), "an input was written"
    return d_i.cpu().numpy(), d_d.cpu().numpy()


def check(got, p, want, what):
    index, dist = got
    assert np.array_equal(index[p], want[2]), (what, "index", np.argwhere(index[p] != want[2])[:4])
    assert kr.same_bits(dist[p], want[3]), (what, "dist", np.argwhere(dist[p].view(np.uint32) != want[3].view(np.uint32))[:4])


def edges(E):
    return (1, 2, E - 1, E, E + 1, 2 * E - 1, 2 * E + 1, 3 * E + 1)


@pytest.mark.parametrize("kind", ["integers", "floats"])
@pytest.mark.parametrize("index", range(10))
def test_shapes_around_the_strip_and_tile_edges(jsg, torch_cuda, edge, index, kind):
    """N and M each over 1, 2, 63, 64, 65, 127, 129, 193, paired so that N < M, N == M and N > M all occur; width 0 and 1 alternate."""
    e = edges(edge)
    assert e == (1, 2, 63, 64, 65, 127, 129, 193)
    shapes = [(e[i], e[7 - i]) for i in range(8)] + [(edge, edge), (2 * edge + 1, 3 * edge + 1)]
    assert {n for n, _ in shapes} >= set(e) and {m for _, m in shapes} >= set(e)
    N, M = shapes[index]
    want = reference(kind, N, M, 12, index, 10, index % 2, "euclidean")
    check(run(jsg, torch_cuda, [want[0]], [want[1]], 10, width=index % 2, pad=index % 3), 0, want, (N, M, kind))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("K", [1, 31, 32, 33, 1024])
def test_feature_counts_around_the_panel_and_at_the_limit(jsg, torch_cuda, edge, K, metric):
    N, M = (edge + 1, edge + 1) if K == 1024 else (edge + 1, 2 * edge + 1)
    want = reference("floats", N, M, K, 100 + K, 7, 1, metric)
    check(run(jsg, torch_cuda, [want[0]], [want[1]], 7, width=1, metric=metric), 0, want, (K, metric))


@pytest.mark.parametrize("kind", ["integers", "floats", "approaching"])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 255, 256])
def test_list_lengths(jsg, torch_cuda, edge, k, kind):
    """k on both sides of the 64 entries a lane step covers and at the limit; 300 columns: more than k everywhere, five tiles."""
    N, M = edge + 6, 4 * edge + 44
    want = reference(kind, N, M, 6, 200 + k, k, 0, "sqeuclidean")
    assert jsg.knn_plan(N, M, 6, k)[4] == jsg.capix.KNN_LDS_STATIC + 384 * k <= jsg.capix.KNN_LDS_LIMIT
    check(run(jsg, torch_cuda, [want[0]], [want[1]], k, metric="sqeuclidean", pad=1), 0, want, (k, kind))


@pytest.mark.parametrize("N, M, k, width, candidates", [(7, 5, 8, 0, 5), (3, 3, 4, 3, 0), (5, 5, 3, 9, 0), (6, 70, 68, 2, None), (70, 6, 5, 2, None)])
def test_k_above_the_number_of_candidates(jsg, torch_cuda, N, M, k, width, candidates):
    """M = 5 with k = 8; width 3 at N = 3 and a width above N: no candidate at all; a band that leaves some rows short."""
    for kind in ("integers", "floats"):
        want = reference(kind, N, M, 4, 300, k, width, "euclidean")
        if candidates is not None:
            assert ((want[2] >= 0).sum(axis=1) == min(k, candidates)).all()
        assert (want[2] < 0).any() and np.isinf(want[3][want[2] < 0]).all()
        check(run(jsg, torch_cuda, [want[0]], [want[1]], k, width=width, pad=2), 0, want, (N, M, k, width, kind))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kind", kr.KINDS)
def test_kinds_of_data_under_every_metric(jsg, torch_cuda, edge, kind, metric):
    N, M, K, k = 2 * edge + 2, 3 * edge + 1, 5, 9
    want = reference(kind, N, M, K, 400, k, 1, metric)
    if kind == "nan_y":
        assert not (want[2] == M // 2).any()
    if kind == "nan_x":
        assert (want[2][N // 2] == -1).all() and (want[2][N // 2 - 1] >= 0).all()
    if kind == "inf" and metric != "cosine":
        assert np.isinf(kr.cost32(want[0], want[1], metric)[:, M // 3]).all()
    if kind == "zero" and metric == "cosine":
        assert (want[3][N // 2] == 1).all() and (want[2][N // 2] == np.arange(k)).all()       # the cost 1 everywhere: the tie rule alone
    if kind == "integers":
        assert (np.diff(want[3], axis=1) == 0).mean() > 0.5        # the tie rule decides most entries
    check(run(jsg, torch_cuda, [want[0]], [want[1]], k, width=1, metric=metric), 0, want, (kind, metric))


@pytest.mark.parametrize("width", [0, 1, 5])
def test_widths_on_a_self_comparison(jsg, torch_cuda, edge, width):
    """x == y: width 0 finds every frame as its own nearest (cost 0), width 1 and 5 exclude the band."""
    N = 2 * edge + 1
    for kind in ("integers", "floats"):
        X = data(kind, N, N, 8, 500)[0]
        index, dist = kr.knn32(X, X, 6, width, "euclidean")
        assert (np.abs(index - np.arange(N)[:, None]) >= width).all() and (width > 0 or kind != "floats" or (index[:, 0] == np.arange(N)).all())
        check(run(jsg, torch_cuda, [X], [X], 6, width=width), 0, (X, X, index, dist), (width, kind))


@pytest.mark.parametrize("kind", ["integers", "floats", "approaching", "receding"])
def test_every_split_gives_the_same_bits(jsg, torch_cuda, edge, kind):
    """193 columns are four tiles: splits 1, 2, 3, 4, 8, 16 (the last two capped at four workgroups) and the automatic one."""
    N, M, k = edge + 6, 3 * edge + 1, 34
    want = reference(kind, N, M, 9, 600, k, 2, "euclidean")
    assert [jsg.knn_plan(N, M, 9, k, split=s)[2] for s in (1, 2, 3, 4, 8, 16)] == [1, 2, 3, 4, 4, 4]
    for split in (1, 2, 3, 4, 8, 16, 0):
        check(run(jsg, torch_cuda, [want[0]], [want[1]], k, width=2, split=split, pad=1), 0, want, (kind, split))
    for S in (2, 3, 4):
        got = kr.split_select32(kr.cost32(want[0], want[1]), k, 2, S)
        assert np.array_equal(got[0], want[2]) and kr.same_bits(got[1], want[3])


def test_three_pairs_in_pitched_buffers_and_a_shared_y(jsg, torch_cuda, edge):
    N, M, K, k = edge + 3, 2 * edge + 5, 11, 12
    wants = [reference(kind, N, M, K, 700 + p, k, 1, "cosine") for p, kind in enumerate(("floats", "integers", "nan_x"))]
    for split in (1, 2):
        got = run(jsg, torch_cuda, [w[0] for w in wants], [w[1] for w in wants], k, width=1, metric="cosine", split=split, pad=3)
        for p, want in enumerate(wants):
            check(got, p, want, ("pairs", split, p))
    Y = wants[0][1]
    shared = [(w[0], Y) + kr.knn32(w[0], Y, k, 1, "cosine") for w in wants]
    got = run(jsg, torch_cuda, [w[0] for w in wants], [Y], k, width=1, metric="cosine", pad=2)
    for p, want in enumerate(shared):
        check(got, p, want, ("shared y", p))


@pytest.mark.parametrize("metric", METRICS)
def test_the_distances_are_the_cost_plane_of_cdist_in_every_bit(jsg, torch_cuda, edge, metric):
    torch = torch_cuda
    N, M, K, k = 2 * edge + 1, 3 * edge + 1, 33, 20
    X, Y = data("floats", N, M, K, 800)
    d_x, d_y = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(Y.copy()).cuda()
    cost = jsg.cdist(d_x, d_y, metric)
    index, dist = jsg.knn(d_x, d_y, k, metric=metric, split=2)
    torch.cuda.synchronize()
    assert (index >= 0).all()
    picked = torch.gather(cost, 1, index.long())
    assert kr.same_bits(picked.cpu().numpy(), dist.cpu().numpy())


def test_graph_capture_of_a_first_launch(jsg, torch_cuda, edge):
    """The three operations captured on a side stream (the search with two workgroups per strip: two kernels), replayed twice with changed input."""
    torch = torch_cuda
    N, K, k = edge + 7, 9, 11
    d_x = torch.zeros((N, K), dtype=torch.float32, device="cuda")
    d_i = torch.full((N, k), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_d = torch.full((N, k), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_rec = torch.full((N, N), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_f = torch.full((N, K), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_bw = torch.full((1,), 1.5, dtype=torch.float32, device="cuda")
    d_scratch = torch.empty((jsg.knn_scratch_bytes(d_x, d_x, d_i, d_d, width=1, split=2) // 4,), dtype=torch.int32, device="cuda")
    assert d_scratch.numel() == 2 * N * k * 2
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.knn_launch(d_x, d_x, d_i, d_d, width=1, split=2, d_scratch=d_scratch, stream=side.cuda_stream)
            jsg.recurrence_launch(d_i, d_d, d_rec, mode="affinity", sym=True, d_bandwidth=d_bw, stream=side.cuda_stream)
            jsg.nn_filter_launch(d_x, d_i, d_f, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert (d_i.cpu().numpy() == ISENTINEL).all() and (d_rec.cpu().numpy() == SENTINEL).all() and (d_f.cpu().numpy() == SENTINEL).all()      # captured, not run
    for seed in (31, 32):
        X = data("floats", N, N, K, seed)[0]
        index, dist = kr.knn32(X, X, k, 1)
        d_x.copy_(torch.from_numpy(X.copy()))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d_i.cpu().numpy(), index) and kr.same_bits(d_d.cpu().numpy(), dist)
        assert kr.same_bits(d_rec.cpu().numpy(), kr.recurrence32(index, dist, N, "affinity", True, False, np.float32(1.5)))
        assert kr.same_bits(d_f.cpu().numpy(), kr.nn_filter32(X, index))


@functools.lru_cache(maxsize=None)
def lists(P, N, M, k, width, seed):
    """The lists of P pairs (x == y where N == M) for the plane and the filter; the last pair is short of candidates in some rows."""
    out = []
    for p in range(P):
        X, Y = data("integers" if p == 1 else "floats", N, M, 6, seed + p)
        out.append(kr.knn32(X, X if N == M else Y, k, width if p < P - 1 else max(N, M) - 3))
    return out


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("mode", list(kr.MODES))
def test_the_recurrence_plane(jsg, torch_cuda, edge, mode, sym, diag):
    """Three pairs in pitched planes; the bandwidths 0.75, 0 and NaN: every link of the last two pairs is a NaN in affinity mode.  The
    mutual plane is symmetric, values included."""
    torch = torch_cuda
    P, N, k = 3, edge + 9, 7
    for M in ((N,) if sym else (N, N + 70, N - 30)):
        ls = lists(P, N, M, k, 1, 900)
        bws = np.array([0.75, 0.0, np.nan], np.float32)
        fi, d_i = guarded(torch, P, N, k, 2, torch.int32, int(ISENTINEL), 1)
        fd, d_d = guarded(torch, P, N, k, 1, torch.float32, float("nan"), 2)
        d_i.copy_(torch.from_numpy(np.stack([l[0] for l in ls])))
        d_d.copy_(torch.from_numpy(np.stack([l[1] for l in ls])))
        fo, d_o = guarded(torch, P, N, M, 3, torch.float32, float(SENTINEL), 2)
        jsg.recurrence_launch(d_i, None if mode == "connectivity" else d_d, d_o, mode=mode, sym=sym, diag=diag, d_bandwidth=torch.from_numpy(bws).cuda())
        torch.cuda.synchronize()
        assert untouched(fo, d_o, SENTINEL, 2), "a guard element was written"
        got = d_o.cpu().numpy()
        for p in range(P):
            want = kr.recurrence32(ls[p][0], ls[p][1], M, mode, sym, diag, bws[p])
            assert kr.same_bits(got[p], want), (mode, sym, diag, M, p, np.argwhere(got[p].view(np.uint32) != want.view(np.uint32))[:4])
            if sym:
                assert kr.same_bits(got[p], got[p].T)
            if mode == "affinity" and p > 0:
                links = want != 0 if not diag else (want != 0) & ~np.eye(N, M, dtype=bool)
                assert np.isnan(want[links]).all() and links.any()
        assert (got[0] != 0).sum() > 0 and (not sym or (got[0] != 0).sum() < N * k)


def test_a_plane_wider_than_one_piece(jsg, torch_cuda):
    """M above the 4096 columns that a workgroup builds at a time: links in both pieces and on their seam."""
    torch = torch_cuda
    N, M, k = 3, jsg.capix.REC_CHUNK + 37, 5
    index = np.array([[0, 4095, 4096, 4132, -1], [4133, 1, 4097, 4095, 2], [-1, -1, -1, -1, -1]], np.int32)      # 4133: outside the plane, no link
    dist = np.arange(N * k, dtype=np.float32).reshape(N, k) + 1
    fo, d_o = guarded(torch, 1, N, M, 5, torch.float32, float(SENTINEL), 1)
    jsg.recurrence_launch(torch.from_numpy(index).cuda(), torch.from_numpy(dist).cuda(), d_o[0], mode="distance", diag=True)
    torch.cuda.synchronize()
    assert untouched(fo, d_o, SENTINEL, 1)
    assert kr.same_bits(d_o[0].cpu().numpy(), kr.recurrence32(index, dist, M, "distance", False, True))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 1025])
def test_nn_filter(jsg, torch_cuda, edge, F, weighted):
    """Mean and weighted mean over three pairs in pitched planes; the last pair has rows without neighbours, and with weights one row
    whose weights sum to zero: both keep their own values."""
    torch = torch_cuda
    P, N, k = 3, edge + 9, 7
    ls = lists(P, N, N, k, 1, 900)
    rng = np.random.default_rng(F)
    S = rng.standard_normal((P, N, F)).astype(np.float32)
    W = rng.random((P, N, k)).astype(np.float32)
    W[0, 5] = [1, -1, 0.5, -0.5, 0, 0, 0]
    assert (ls[2][0] < 0).all(axis=1).any() and W[0, 5].sum() == 0
    fs, d_s = guarded(torch, P, N, F, 1, torch.float32, float("nan"), 1)
    d_s.copy_(torch.from_numpy(S))
    fo, d_o = guarded(torch, P, N, F, 2, torch.float32, float(SENTINEL), 3)
    d_i = torch.from_numpy(np.stack([l[0] for l in ls])).cuda()
    jsg.nn_filter_launch(d_s, d_i, d_o, d_weights=torch.from_numpy(W).cuda() if weighted else None)
    torch.cuda.synchronize()
    assert untouched(fo, d_o, SENTINEL, 3), "a guard element was written"
    got = d_o.cpu().numpy()
    for p in range(P):
        want = kr.nn_filter32(S[p], ls[p][0], W[p] if weighted else None)
        assert kr.same_bits(got[p], want), (F, weighted, p)
    alone = (ls[2][0] < 0).all(axis=1)
    assert kr.same_bits(got[2][alone], S[2][alone]) and (not weighted or kr.same_bits(got[0][5], S[0][5]))


def test_the_python_layer_end_to_end(jsg, torch_cuda, edge):
    """recurrence_matrix on an MFCC-like plane (20 coefficients a frame) and cross_similarity against the restatement, defaults included;
    bandwidth None is the restated median; nn_filter on the same lists."""
    torch = torch_cuda
    N, M, K = 3 * edge + 8, 2 * edge + 1, 20
    rng = np.random.default_rng(77)
    X = np.cumsum(rng.standard_normal((N, K)), axis=0).astype(np.float32)
    Y = X[rng.integers(0, N, M)] + np.float32(0.05) * rng.standard_normal((M, K)).astype(np.float32)
    k = jsg.knn_default_k(N, 1)
    assert k == kr.default_k(N, 1) == 2 * int(np.ceil(np.sqrt(N - 1))) and jsg.knn_default_k(10 ** 6, 0) == 256 and jsg.knn_default_k(3, 5) == 1
    index, dist = kr.knn32(X, X, k, 1)
    gi, gd = jsg.knn(X, k=k, width=1)
    assert np.array_equal(gi.cpu().numpy(), index) and kr.same_bits(gd.cpu().numpy(), dist)
    for mode in kr.MODES:
        for sym in (False, True):
            bw = kr.bandwidth32(dist)
            want = kr.recurrence32(index, dist, N, mode, sym, False, bw)
            assert kr.same_bits(jsg.recurrence_matrix(X, sym=sym, mode=mode).cpu().numpy(), want), (mode, sym)
    assert kr.same_bits(jsg.recurrence_matrix(torch.from_numpy(X).cuda(), k=5, width=3, metric="cosine", mode="affinity", bandwidth=0.25, self=True).cpu().numpy(),
                        kr.recurrence32(*kr.knn32(X, X, 5, 3, "cosine"), N, "affinity", False, True, np.float32(0.25)))
    kc = min(M, 2 * int(np.ceil(np.sqrt(M))))
    ci, cd = kr.knn32(X, Y, kc, 0)
    for mode in kr.MODES:
        assert kr.same_bits(jsg.cross_similarity(X, Y, mode=mode).cpu().numpy(), kr.recurrence32(ci, cd, M, mode, False, False, kr.bandwidth32(cd))), mode
    # three pairs at once: the bandwidth is per pair
    X3 = np.stack([X, X[::-1].copy(), (2 * X).astype(np.float32)])
    got = jsg.recurrence_matrix(X3, k=6, mode="affinity").cpu().numpy()
    for p in range(3):
        i6, d6 = kr.knn32(X3[p], X3[p], 6, 1)
        assert kr.same_bits(got[p], kr.recurrence32(i6, d6, N, "affinity", False, False, kr.bandwidth32(d6))), p
    S = rng.standard_normal((N, 40)).astype(np.float32)
    assert kr.same_bits(jsg.nn_filter(S, gi).cpu().numpy(), kr.nn_filter32(S, index))
    assert kr.same_bits(jsg.nn_filter(S, index, weights=dist).cpu().numpy(), kr.nn_filter32(S, index, dist))
    with pytest.raises(jsg.JsgError, match="k must be in 1..256"):
        jsg.knn(X, k=257)
    with pytest.raises(jsg.JsgError, match="mode must be one of"):
        jsg.recurrence_matrix(X, mode="median")
