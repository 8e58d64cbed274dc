"""Recurrence quantification alignment of libjsgx.so on the GPU (include/jsgx.h section 9) against tests/rqa_ref.py, bit for bit (NaN
positions equal, all other bits equal): S, the step plane, the path, its length, the end cell and the total over shapes around the tile
edges and the two halo rows, with and without knight moves, on planes with many ties and with none, under three pairs of penalties;
three pairs in pitched buffers with poisoned padding; a NaN and a negative cell that stay in their pair; the outputs one by one with the
scratch each needs; the all-zero plane; graph capture of a first launch; and the Python layer end to end, behind recurrence_matrix."""
import functools

import numpy as np
import pytest

import rqa_ref as rr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
ISENTINEL = np.int32(-77777)
BSENTINEL = np.int8(77)
PLANES = {"integers": rr.integer_links, "floats": rr.float_links}
PENALTIES = [(1.0, 1.0), (0.5, 0.25), (0.0, 0.0)]
# 65 and 66 are the rows that read one and two halo rows from the tile above; the off-square shapes put knight moves across tile corners
SHAPES = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 70), (3, 3), (63, 64), (64, 64), (65, 65), (66, 66), (64, 130), (130, 64), (129, 67), (200, 131)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def reference_of(R, on, ex, knight):
    S, step = rr.rqa32(R, on, ex, knight)
    path, end, total = rr.backtrace32(S, R, on, ex, knight)
    for a in (S, step):
        a.setflags(write=False)
    return R, S, step, path, end, total


@functools.lru_cache(maxsize=None)
def reference(kind, N, M, seed, penalties, knight):
    """(R, S, step, path, end, total) of the restatement; computed once and shared."""
    R = PLANES[kind](N, M, seed)
    R.setflags(write=False)
    return reference_of(R, *PENALTIES[penalties], knight)


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


def run(jsg, torch, planes, on, ex, knight, *, pad=0):
    """One launch over the pairs `planes` (equal shapes) in pitched buffers full of sentinels -> (S [P][N][M], step, path_i, path_j
    [P][min(N, M)], path_len [P], end [P][2], total [P]) as numpy, after checking that nothing outside these was written."""
    P, (N, M) = len(planes), planes[0].shape
    L = min(N, M)
    fr, d_sim = guarded(torch, P, N, M, pad, torch.float32, float("nan"), 3)
    d_sim.copy_(torch.from_numpy(np.stack(planes)))
    fs, d_score = guarded(torch, P, N, M, 2 * pad, torch.float32, float(SENTINEL), 1)
    fb, d_step = guarded(torch, P, N, M, 3 * pad, torch.int8, int(BSENTINEL), 5)
    fi, d_pi = guarded(torch, 1, P, L, pad, torch.int32, int(ISENTINEL), 2)
    fj, d_pj = guarded(torch, 1, P, L, pad, torch.int32, int(ISENTINEL), 2)
    d_len = torch.full((P + 2,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_end = torch.full((2 * P + 4,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_total = torch.full((P + 2,), float(SENTINEL), dtype=torch.float32, device="cuda")
    jsg.rqa_launch(d_sim, d_score, gap_onset=on, gap_extend=ex, knight_moves=knight, d_step=d_step, d_path_i=d_pi[0], d_path_j=d_pj[0], d_path_len=d_len[1:P + 1],
                   d_end=d_end[2:2 * P + 2], d_total=d_total[1:P + 1])
    torch.cuda.synchronize()
    assert untouched(fs, d_score, SENTINEL, 1) and untouched(fb, d_step, BSENTINEL, 5) and untouched(fi, d_pi, ISENTINEL, 2) and untouched(fj, d_pj, ISENTINEL, 2), \
        "a guard element was written"
    assert untouched(fr, d_sim, float("nan"), 3) and rr.same_bits(d_sim.cpu().numpy(), np.stack(planes)), "sim was written"
    n, e, t = d_len.cpu().numpy(), d_end.cpu().numpy(), d_total.cpu().numpy()
    assert n[0] == n[-1] == ISENTINEL and (e[:2] == ISENTINEL).all() and (e[-2:] == ISENTINEL).all() and t[0] == t[-1] == SENTINEL
    return d_score.cpu().numpy(), d_step.cpu().numpy(), d_pi[0].cpu().numpy(), d_pj[0].cpu().numpy(), n[1:P + 1], e[2:2 * P + 2].reshape(P, 2), t[1:P + 1]


def check_pair(got, p, want, what):
    S, step, pi, pj, n, end, total = got
    _, wS, wstep, wpath, wend, wtotal = want
    assert rr.same_bits(S[p], wS), (what, "S", np.argwhere(S[p].view(np.uint32) != wS.view(np.uint32))[:4])
    assert np.array_equal(step[p], wstep), (what, "step", np.argwhere(step[p] != wstep)[:4])
    L = len(wpath)
    assert n[p] == L and tuple(end[p]) == tuple(wend) and rr.same_bits(total[p:p + 1], np.asarray([wtotal])), (what, "end", n[p], L, end[p], wend, total[p], wtotal)
    assert not np.signbit(total[p]) or wtotal != 0
    assert (pi[p, :L] == wpath[:, 0]).all() and (pj[p, :L] == wpath[:, 1]).all(), (what, "path")
    assert (pi[p, L:] == ISENTINEL).all() and (pj[p, L:] == ISENTINEL).all(), (what, "behind the path")


@pytest.mark.parametrize("kind", list(PLANES))
@pytest.mark.parametrize("index", range(len(SHAPES)))
def test_shapes_around_the_tile_edges(jsg, torch_cuda, index, kind):
    """Every shape with and without knight moves under the three pairs of penalties: small-integer planes (many ties, every operation
    exact) and affinities in (0, 1] (none)."""
    N, M = SHAPES[index]
    assert jsg.rqa_plan(N, M)[3] == -(-N // 64) + -(-M // 64)
    for knight in (False, True):
        for pen, (on, ex) in enumerate(PENALTIES):
            want = reference(kind, N, M, index, pen, knight)
            check_pair(run(jsg, torch_cuda, [want[0]], on, ex, knight), 0, want, (N, M, kind, knight, on, ex))


@pytest.mark.parametrize("knight", [False, True])
def test_three_pairs_in_padded_buffers(jsg, torch_cuda, knight):
    """The result is a function of the plane: a pair computes what it computes alone, whatever the pitches; the poisoned padding stays."""
    N, M = 69, 73
    wants = [reference(kind, N, M, seed, 1, knight) for kind, seed in (("floats", 1), ("integers", 2), ("floats", 3))]
    got = run(jsg, torch_cuda, [w[0] for w in wants], *PENALTIES[1], knight, pad=7)
    for p, want in enumerate(wants):
        check_pair(got, p, want, (p, knight))


def test_a_nan_cell_and_a_negative_cell_stay_in_their_pair(jsg, torch_cuda):
    """A NaN or a negative cell is no link: off the border it is a gap cell like any other, on the border it is copied, and a NaN S from
    there runs through the links that follow it (a NaN first candidate stays) and resets the gap cell behind them.  The pairs before and
    after compute what they compute alone."""
    N, M = 73, 69
    on, ex = PENALTIES[1]
    clean = [reference("floats", N, M, seed, 1, True) for seed in (11, 12, 13)]
    bad = np.array(clean[1][0])
    bad[63, 63], bad[64, 64], bad[65, 65], bad[66, 67] = 0.5, np.nan, 0.75, 0.5         # a NaN in the first cell of the last tile, links around it
    bad[10, 10], bad[0, 5], bad[0, 9] = -2.0, -1.5, -0.0
    bad[7, 0], bad[8, 1], bad[9, 2], bad[10, 3] = np.nan, 0.5, 0.5, 0.0                 # a NaN on the border, two links behind it, then a gap
    want_bad = reference_of(bad, on, ex, True)
    S, step = want_bad[1], want_bad[2]
    assert not np.isnan(S[64, 64]) and S[64, 64] >= 0 and S[10, 10] >= 0                # off the border a NaN or a negative cell is a gap like any other
    assert S[0, 5] == np.float32(-1.5) and np.isnan(S[7, 0]) and step[0, 5] == step[7, 0] == step[0, 9] == -1 and np.signbit(S[0, 9])
    assert np.isnan(S[8, 1]) and np.isnan(S[9, 2]) and step[9, 2] == 0 and not np.isnan(S[10, 3])      # a NaN first candidate stays; a NaN best resets a gap
    got = run(jsg, torch_cuda, [clean[0][0], bad, clean[2][0]], on, ex, True, pad=2)
    check_pair(got, 0, clean[0], "before the special pair")
    check_pair(got, 1, want_bad, "the special pair")
    check_pair(got, 2, clean[2], "after the special pair")
    # a NaN S that runs down a diagonal of links into the next tile, and the end cell that ignores it
    run_nan = np.zeros((N, M), np.float32)
    run_nan[0, 0] = np.nan
    for i in range(1, 67):
        run_nan[i, i] = 1.0
    run_nan[5, 30] = run_nan[6, 31] = 2.0
    want_run = reference_of(run_nan, 1.0, 1.0, False)
    assert np.isnan(want_run[1][66, 66]) and want_run[4] == (6, 31) and want_run[5] == 4 and len(want_run[3]) == 2
    check_pair(run(jsg, torch_cuda, [run_nan], 1.0, 1.0, False), 0, want_run, "a NaN run")


def test_outputs_one_by_one_and_their_scratch(jsg, torch_cuda):
    """step = NULL gives the same S; the score alone needs no scratch; total and end without paths need the tiles' entries alone."""
    torch = torch_cuda
    N, M = 130, 67
    for knight in (False, True):
        R, S, step, path, end, total = reference("integers", N, M, 5, 0, knight)
        d_sim = torch.from_numpy(np.array(R)).cuda()
        kw = dict(gap_onset=1.0, gap_extend=1.0, knight_moves=knight)
        # the score alone, with a zero scratch
        d_score = torch.full((N, M), float(SENTINEL), dtype=torch.float32, device="cuda")
        assert jsg.rqa_scratch_bytes(d_sim, d_score, **kw) == 0 and jsg.rqa_plan(N, M, backtrack=False)[3] + 1 == jsg.rqa_plan(N, M)[3]
        none = torch.empty((0,), dtype=torch.int32, device="cuda")
        jsg.rqa_launch(d_sim, d_score, d_scratch=none, **kw)
        # the score and the steps
        d_score2 = torch.full((N, M), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_step = torch.full((N, M), int(BSENTINEL), dtype=torch.int8, device="cuda")
        assert jsg.rqa_scratch_bytes(d_sim, d_score2, d_step=d_step, **kw) == 0
        jsg.rqa_launch(d_sim, d_score2, d_step=d_step, d_scratch=none, **kw)
        # total and end without paths
        d_score3 = torch.full((N, M), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_total = torch.full((3,), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_end = torch.full((6,), int(ISENTINEL), dtype=torch.int32, device="cuda")
        assert jsg.rqa_scratch_bytes(d_sim, d_score3, d_total=d_total[1:2], d_end=d_end[2:4], **kw) == 8 * 3 * 2
        jsg.rqa_launch(d_sim, d_score3, d_total=d_total[1:2], d_end=d_end[2:4], **kw)
        # the length alone: the walk without a record
        d_score4 = torch.empty_like(d_score)
        d_len = torch.full((3,), int(ISENTINEL), dtype=torch.int32, device="cuda")
        assert jsg.rqa_scratch_bytes(d_sim, d_score4, d_path_len=d_len[1:2], **kw) == 8 * 3 * 2
        jsg.rqa_launch(d_sim, d_score4, d_path_len=d_len[1:2], **kw)
        torch.cuda.synchronize()
        for d in (d_score, d_score2, d_score3, d_score4):
            assert rr.same_bits(d.cpu().numpy(), S), knight
        assert np.array_equal(d_step.cpu().numpy(), step)
        t, e, n = d_total.cpu().numpy(), d_end.cpu().numpy(), d_len.cpu().numpy()
        assert t[0] == t[2] == SENTINEL and rr.same_bits(t[1:2], np.asarray([total])) and e.tolist() == [ISENTINEL] * 2 + list(end) + [ISENTINEL] * 2
        assert n.tolist() == [ISENTINEL, len(path), ISENTINEL]


def test_the_all_zero_plane_and_the_identity(jsg, torch_cuda):
    """The known answers of the header: an all-zero plane has no path (a result, not a refusal); the identity's path is its diagonal."""
    N, M = 70, 131
    zero = np.zeros((N, M), np.float32)
    want = reference_of(zero, 1.0, 1.0, True)
    assert len(want[3]) == 0 and want[4] == (-1, -1) and (want[2] == -1).all()
    got = run(jsg, torch_cuda, [zero, zero], 1.0, 1.0, True)
    for p in range(2):
        check_pair(got, p, want, "zeros")
        assert got[4][p] == 0 and got[6][p] == 0 and not np.signbit(got[6][p]) and not np.signbit(got[0][p]).any()
    # a plane of -0 under penalties of zero: the border keeps its bits, and behind it best = -0 - 0 = -0 is not > 0, so S is +0
    minus = np.full((67, 66), -0.0, np.float32)
    want = reference_of(minus, 0.0, 0.0, True)
    assert np.signbit(want[1][0]).all() and np.signbit(want[1][:, 0]).all() and not np.signbit(want[1][1:, 1:]).any() and len(want[3]) == 0
    check_pair(run(jsg, torch_cuda, [minus], 0.0, 0.0, True), 0, want, "minus zero")
    # equal maxima in two tiles, in two rows of one tile and in two lanes of one row: the lowest i, then the lowest j
    ties = np.zeros((80, 131), np.float32)
    for i, j in ((70, 5), (5, 100), (5, 70), (9, 66), (70, 100)):
        ties[i, j] = 3.0
    want = reference_of(ties, 1.0, 1.0, True)
    assert want[4] == (5, 70) and want[5] == 3 and (want[1] == 3).sum() == 5 and len(want[3]) == 1
    check_pair(run(jsg, torch_cuda, [ties], 1.0, 1.0, True), 0, want, "ties")
    N, g = 70, 2
    for knight in (False, True):
        I = np.eye(N, dtype=np.float32)
        G = np.array(I)
        G[g, g] = G[g + 1, g + 1] = 0
        wants = [reference_of(I, 0.5, 0.25, knight), reference_of(G, 0.5, 0.25, knight)]
        got = run(jsg, torch_cuda, [I, G], 0.5, 0.25, knight)
        for p in range(2):
            check_pair(got, p, wants[p], ("identity", p, knight))
        assert got[6][0] == N and got[4][0] == N and got[6][1] == (67.5 if knight else 67.25) and got[4][1] == (69 if knight else 70)


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """A captured first launch (several kernels on the one stream), replayed once."""
    torch = torch_cuda
    N, M = 67, 69               # four tiles, three anti-diagonals, the backtrace
    L = min(N, M)
    on, ex = PENALTIES[1]
    d_sim = torch.zeros((2, N, M), dtype=torch.float32, device="cuda")
    d_score = torch.full((2, N, M), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_step = torch.full((2, N, M), int(BSENTINEL), dtype=torch.int8, device="cuda")
    d_pi, d_pj = (torch.full((2, L), int(ISENTINEL), dtype=torch.int32, device="cuda") for _ in range(2))
    d_len = torch.full((2,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_end = torch.full((4,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_total = torch.full((2,), float(SENTINEL), dtype=torch.float32, device="cuda")
    kw = dict(gap_onset=on, gap_extend=ex, knight_moves=True, d_step=d_step, d_path_i=d_pi, d_path_j=d_pj, d_path_len=d_len, d_end=d_end, d_total=d_total)
    d_scratch = torch.empty((jsg.rqa_scratch_bytes(d_sim, d_score, **kw) // 4,), dtype=torch.int32, device="cuda")
    assert d_scratch.numel() == 2 * 2 * 4 + 2 * 2 * L
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.rqa_launch(d_sim, d_score, d_scratch=d_scratch, stream=side.cuda_stream, **kw)
    torch.cuda.synchronize()
    assert (d_len.cpu().numpy() == ISENTINEL).all() and (d_score.cpu().numpy() == SENTINEL).all()      # captured, not run
    wants = [reference("floats", N, M, seed, 1, True) for seed in (21, 22)]
    d_sim.copy_(torch.from_numpy(np.stack([w[0] for w in wants])))
    g.replay()
    torch.cuda.synchronize()
    got = (d_score.cpu().numpy(), d_step.cpu().numpy(), d_pi.cpu().numpy(), d_pj.cpu().numpy(), d_len.cpu().numpy(), d_end.cpu().numpy().reshape(2, 2), d_total.cpu().numpy())
    for p, want in enumerate(wants):
        check_pair(got, p, want, ("replay", p))


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_the_python_layer_end_to_end(jsg, torch_cuda):
    R = rr.integer_links(90, 70, 3)
    want = reference_of(R, 1.0, 1.0, True)
    score, path = jsg.rqa(R)
    assert rr.same_bits(score.cpu().numpy(), want[1]) and path.dtype == torch_cuda.int32 and np.array_equal(path.cpu().numpy(), want[3])
    # a device tensor, no knight moves, other penalties, the score alone
    want = reference_of(R, 0.5, 0.25, False)
    score = jsg.rqa(torch_cuda.from_numpy(R).cuda(), gap_onset=0.5, gap_extend=0.25, knight_moves=False, backtrack=False)
    assert tuple(score.shape) == (90, 70) and rr.same_bits(score.cpu().numpy(), want[1])
    # pairs; an all-zero plane among them has an empty path
    planes = np.stack([R, np.zeros_like(R), rr.float_links(90, 70, 4)])
    score, paths = jsg.rqa(planes, 0.5, 0.25)
    assert tuple(score.shape) == (3, 90, 70) and len(paths) == 3 and tuple(paths[1].shape) == (0, 2)
    for p in range(3):
        want = reference_of(planes[p], 0.5, 0.25, True)
        assert rr.same_bits(score[p].cpu().numpy(), want[1]) and np.array_equal(paths[p].cpu().numpy(), want[3])
    with pytest.raises(jsg.JsgError, match="gap_onset must be finite and >= 0"):
        jsg.rqa(R, gap_onset=-1.0)


CHAIN_SEED = 0


def test_a_repeated_section_behind_recurrence_matrix(jsg, torch_cuda):
    """Features [A, B, A], A of 40 random frames and B of 50: the affinity plane of recurrence_matrix followed by rqa returns the repeat, a
    path on the diagonal j = i - 90 (or its mirror) that covers at least 38 of the 40 frames; the plane never leaves device memory."""
    rng = np.random.default_rng(CHAIN_SEED)
    A, B = rng.standard_normal((40, 12)).astype(np.float32), rng.standard_normal((50, 12)).astype(np.float32)
    X = np.concatenate([A, B, A])
    rec = jsg.recurrence_matrix(X, mode="affinity")
    assert rec.is_cuda and tuple(rec.shape) == (130, 130)
    score, path = jsg.rqa(rec)
    path = path.cpu().numpy()
    lag = path[:, 0] - path[:, 1]
    assert len(path) >= 38 and ((lag == 90).all() or (lag == -90).all()), path
    want = reference_of(rec.cpu().numpy(), 1.0, 1.0, True)
    assert rr.same_bits(score.cpu().numpy(), want[1]) and np.array_equal(path, want[3])
