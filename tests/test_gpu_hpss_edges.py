"""Harmonic-percussive separation on the GPU, what tests/test_gpu_hpss.py does not reach.  Both kernels are persistent: a workgroup
walks work items with `item += gridDim.x`, and the largest launch of that file has fewer items than the grid has workgroups.  Here
each kernel gets more than three grids of items with a ragged last round, so a workgroup rebuilds its window and reuses its LDS tile
for items of another kind; the library's own chunk length above its floor of 32; the two window pairs that put one kernel on the
register window and the other on the LDS window; every odd window length; and negative zeros in real power input.  Every comparison
is bit for bit against tests/hpss_ref.py, except the negative zeros (numbers, as the definition leaves the sign of a zero open)."""
import os
import re
import time

import numpy as np
import pytest

import hpss_ref as hr
from test_gpu_hpss import SENTINEL, check_all, mirror, run, same, torch_cuda  # noqa: F401  (torch_cuda is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = open(os.path.join(ROOT, "jadespectrogram_amd", "csrc", "jsg_hpss.hip")).read()
TILE = 64                   # bins per tile, frames per block of the frequency pass
NAMES = ("mask_h", "mask_p", "out_h", "out_p")


def grid_limit(torch):
    """The grid limit of jsg_hpss_launch: its workgroups per compute unit, read from the source so that a retune is seen here."""
    per_cu = re.search(r"max_grid = \(long long\)cu_count_of_device\(dev\) \* (\d+);", SOURCE)
    assert per_cu, "jsg_hpss_launch no longer sizes its grid as cu_count_of_device(dev) * N"
    return int(per_cu.group(1)) * torch.cuda.get_device_properties(0).multi_processor_count


def default_chunk(T, rows, tiles):
    """The library's choice for chunk_frames = 0, with its three constants read from the source."""
    m = re.search(r"want = \(\(i128\)T \* rows \* tiles \+ (\d+)\) / (\d+);\s*return \(long long\)std::max<i128>\((\d+), std::min<i128>\((\d+), want\)\);", SOURCE)
    assert m, "default_chunk no longer reads as max(lo, min(hi, ceil(T * rows * tiles / per)))"
    add, per, lo, hi = map(int, m.groups())
    assert add == per - 1
    return max(lo, min(hi, -(-T * rows * tiles // per))), lo


def ceil_div(a, b):
    return -(-a // b)


def freq_items_per_row(T, K):
    return ceil_div(T, TILE) * ceil_div(K, TILE)


def time_items_per_row(T, K, chunk):
    return ceil_div(T, chunk) * ceil_div(K, TILE)


def premises(items, per_row, grid, what):
    """More than three rounds, a ragged last one, and successive items of a workgroup of different kinds."""
    assert items >= 3 * grid, (what, items, grid)
    assert items % grid != 0, (what, items, grid)
    assert grid % per_row != 0, (what, per_row, grid)


def rows_for(grid, *per_rows):
    """The fewest rows with which every kernel named by its items per row gets three grids of items and a ragged last round."""
    rows = max(ceil_div(3 * grid + 1, p) for p in per_rows)
    while any(rows * p % grid == 0 for p in per_rows):
        rows += 1
    assert rows <= 65535, (rows, grid)
    return rows


def bits(torch, t):
    t = t.contiguous()
    return (torch.view_as_real(t) if t.is_complex() else t).view(torch.int32)


def launch(jsg, torch, d_X, W, want, **kw):
    """One launch into dense sentinel-filled device buffers: the requested of (mask_h, mask_p, out_h, out_p), None for the others."""
    new = lambda dtype: torch.full(d_X.shape, float(SENTINEL), dtype=dtype, device="cuda")
    mh, mp, oh, op = (new(dt) if w else None for w, dt in zip(want, (torch.float32, torch.float32, d_X.dtype, d_X.dtype)))
    jsg.hpss_launch(d_X, d_harm=oh, d_perc=op, d_mask_h=mh, d_mask_p=mp, kernel_size=W, **kw)
    torch.cuda.synchronize()
    return mh, mp, oh, op


def check_tiled(jsg, torch, T, K, W, rows, real, want, alone, **kw):
    """`rows` rows that repeat `D` distinct planes, in one launch: every row has the bits of the restatement of its plane (compared on
    the device), and the rows `alone` have the bits of a launch of that row alone, which has too few items for a second round."""
    D = 7
    distinct = np.stack([hr.make_input(T, K, seed=s) for s in range(D)])
    distinct = hr.power(distinct) if real else distinct
    expect = [np.stack(e) for e in zip(*(hr.mirror(distinct[s], *W)[:4] for s in range(D)))]
    idx = torch.arange(rows, device="cuda") % D
    d_X = torch.from_numpy(distinct).cuda()[idx]
    got = launch(jsg, torch, d_X, W, want, **kw)
    for name, g, e, w in zip(NAMES, got, expect, want):
        assert (g is not None) == w
        if w:
            bad = int((bits(torch, g) != bits(torch, torch.from_numpy(e).cuda())[idx]).sum())
            assert bad == 0, (name, "elements that differ from the restatement", bad, g.numel())
    for r in alone:
        one = launch(jsg, torch, d_X[r], W, want)
        for name, g, o in zip(NAMES, got, one):
            if g is not None:
                assert torch.equal(bits(torch, g[r]), bits(torch, o)), (name, "row together differs from row alone", r)


def around(grid, per_row, rows):
    """The first row, the last, and the rows on either side of the item with the grid's number."""
    mid = grid // per_row
    return sorted({0, mid - 1, mid, mid + 1, rows - 1})


@pytest.mark.parametrize("W", [(31, 31), (17, 9)], ids=str)
def test_frequency_pass_takes_more_items_than_the_grid(jsg, torch_cuda, W):
    """Real power, masks only, 65 x 129: six items per row (a full block of frames and one of a single frame, two full tiles and one
    of a single bin), and enough rows for three grids of them.  A workgroup's next item is 6 k + 2 further on for a grid of 32 x 256,
    so it reuses its LDS tile for a tile of another kind and passes its trailing barrier into a new staging phase."""
    torch = torch_cuda
    T, K = 65, 129
    grid, per_row = grid_limit(torch), freq_items_per_row(T, K)
    assert per_row == 6
    rows = rows_for(grid, per_row)
    premises(rows * per_row, per_row, grid, "frequency pass")
    t = time.perf_counter()
    check_tiled(jsg, torch, T, K, W, rows, True, (True, True, False, False), around(grid, per_row, rows))
    print(f"hpss frequency pass W {W}: {rows} rows, {rows * per_row} items, grid {grid}, {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("W", [(31, 31), (17, 9)], ids=str)
@pytest.mark.parametrize("chunk", [1, 8], ids=["time", "both"])
def test_complex_input_takes_more_items_than_the_grid(jsg, torch_cuda, chunk, W):
    """Complex input, all four outputs, 65 x 129.  chunk_frames = 1: the fewest rows that give the time pass three grids of items
    (195 per row).  chunk_frames = 8: the rows of the frequency-pass test, so that the complex instantiation of both kernels goes
    round its loop; the time pass then has 27 items per row, the ninth chunk a single frame."""
    torch = torch_cuda
    T, K = 65, 129
    grid = grid_limit(torch)
    per_row_t, per_row_f = time_items_per_row(T, K, chunk), freq_items_per_row(T, K)
    assert per_row_t == {1: 195, 8: 27}[chunk]
    rows = rows_for(grid, per_row_t) if chunk == 1 else rows_for(grid, per_row_t, per_row_f)
    premises(rows * per_row_t, per_row_t, grid, "time pass")
    if chunk == 8:
        premises(rows * per_row_f, per_row_f, grid, "frequency pass")
    t = time.perf_counter()
    check_tiled(jsg, torch, T, K, W, rows, False, (True, True, True, True), around(grid, per_row_t if chunk == 1 else per_row_f, rows), chunk_frames=chunk)
    print(f"hpss complex, chunk_frames {chunk}, W {W}: {rows} rows, time pass {rows * per_row_t} items, frequency pass {rows * per_row_f} items, "
          f"grid {grid}, {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("W", [(31, 31), (17, 9)], ids=str)
def test_time_pass_takes_more_items_than_the_grid(jsg, torch_cuda, W):
    """Eight rows of 1600 x 129, complex, all four outputs, one frame per chunk: 38 400 items, so a workgroup rebuilds its window (in
    LDS or in the 31 registers) for a chunk of another row, frame and tile.  And the same call at the library's own chunk length."""
    torch = torch_cuda
    T, K, rows, D = 1600, 129, 8, 8
    grid, per_row = grid_limit(torch), time_items_per_row(T, K, 1)
    premises(rows * per_row, per_row, grid, "time pass")
    distinct = [hr.make_input(T, K, seed=s) for s in range(D)]
    X = np.stack([distinct[r % D] for r in range(rows)])
    t = time.perf_counter()
    expect = [hr.mirror(x, *W)[:4] for x in distinct]
    t_ref = time.perf_counter() - t
    want = [np.stack([expect[r % D][i] for r in range(rows)]) for i in range(4)]
    t = time.perf_counter()
    for chunk in (1, 0):
        got = run(jsg, torch, X, W, chunk_frames=chunk)
        for name, g, w in zip(NAMES, got, want):
            assert same(g, w), (name, "chunk_frames", chunk, "elements that differ", int((np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).sum()), g.size)
    print(f"hpss time pass W {W}: {rows} rows, {rows * per_row} items, grid {grid}, {time.perf_counter() - t:.2f} s (restatement {t_ref:.2f} s)")


def test_the_library_chunk_above_its_floor(jsg, torch_cuda):
    """chunk_frames = 0 where the library's choice lies above its floor of 32 and below T (8 x 1600 x 129 above still gives 32:
    ceil(38 400 / 4096) = 10): 342 rows of 200 x 129 give 51 frames, so four chunks, the last of 47."""
    torch = torch_cuda
    T, K, rows, W = 200, 129, 342, (31, 31)
    chunk, floor = default_chunk(T, rows, ceil_div(K, TILE))
    assert floor < chunk < T and T % chunk != 0, (chunk, floor)
    t = time.perf_counter()
    check_tiled(jsg, torch, T, K, W, rows, False, (True, True, True, True), (0, 170, rows - 1))
    print(f"hpss library chunk {chunk}: {rows} rows, time pass {rows * time_items_per_row(T, K, chunk)} items, grid {grid_limit(torch)}, {time.perf_counter() - t:.2f} s")


@pytest.mark.parametrize("W", [(17, 31), (31, 17)], ids=str)
def test_one_window_in_registers_and_one_in_lds(jsg, torch_cuda, W):
    """The time kernel on the LDS window with the frequency kernel on the register window, and the reverse, at a size with several
    blocks, tiles and chunks."""
    T, K = 200, 130
    X = hr.make_input(T, K)
    for chunk in (0, 1):
        check_all(run(jsg, torch_cuda, X, W, chunk_frames=chunk), mirror(T, K, *W))


@pytest.mark.parametrize("axis", [0, 1], ids=["time", "frequency"])
def test_every_odd_window_length(jsg, torch_cuda, axis):
    """Every odd length 1..63 on one axis with the other at 31, on 70 x 65 (two blocks, two tiles, windows longer than an edge tile)."""
    T, K = 70, 65
    X = hr.make_input(T, K)
    wrong = []
    for L in range(1, 64, 2):
        W = (L, 31) if axis == 0 else (31, L)
        got, want = run(jsg, torch_cuda, X, W), mirror(T, K, *W)
        wrong += [(L, name) for name, g, w in zip(NAMES, got, want) if not same(g, w)]
    assert not wrong, wrong


@pytest.mark.parametrize("W", [(31, 31), (17, 9)], ids=str)
def test_negative_zero_in_real_power_input(jsg, torch_cuda, W):
    """The sort key orders -0.0 below +0.0 and the definition does not say which sign a median of equal zeros carries, so only this
    is asserted: with -0.0 among the powers all four outputs are finite and equal, as numbers, those of the same planes with +0.0 in
    its place.  Two planes: powers of small integers with a block of zeros, and noise with four elements in ten zeroed, so that
    windows hold zeros of both signs beside equal and beside much larger values."""
    T, K = 96, 257
    rng = np.random.default_rng(96257)
    noise = np.array(hr.power(hr.make_input(T, K)))
    noise[rng.random((T, K)) < 0.4] = 0
    plus = np.stack([hr.power(hr.tie_input(T, K)), noise])
    minus = plus.copy()
    minus[(plus == 0) & (rng.random(plus.shape) < 0.5)] = -0.0
    assert np.array_equal(plus, minus) and not np.signbit(plus).any()
    assert all(np.signbit(m).sum() > 500 and ((m == 0) & ~np.signbit(m)).sum() > 500 for m in minus)
    got_plus, got_minus = run(jsg, torch_cuda, plus, W), run(jsg, torch_cuda, minus, W)
    for r in range(2):
        check_all([g[r] for g in got_plus], hr.mirror(plus[r], *W)[:4])
    zero_medians = 0
    for name, m, p in zip(NAMES, got_minus, got_plus):
        assert np.isfinite(m).all(), name
        assert np.array_equal(m, p), (name, int((m != p).sum()))
        zero_medians += int((p == 0).sum())
    assert zero_medians > 0
