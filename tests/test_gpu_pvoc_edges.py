"""Phase vocoder on the GPU, the edges tests/test_gpu_pvoc.py does not reach: a single partial tile, a full last tile and the largest
n; special values (signed zeros, angles of +-pi, moduli across the float32 range); rates far from 1 and next to 1; more work items
than the grid has workgroups, in the walks and in the scan; the row limit; every number of chunks; the tightest legal pitches; an
infinity in the input; the Python layer on what torch.stft returns, on complex128 and on an unbatched tensor."""
import numpy as np
import pytest

import pvoc_ref as pr
from test_gpu_pvoc import POISON, bits, run, same_bits, torch_cuda  # noqa: F401  (torch_cuda is a fixture)

pytestmark = pytest.mark.gpu


def assert_within_both_bounds(X, Y, rate, hop, n, what):
    """The three assertions of test_accuracy_against_float64 on one [T][K] input and its result."""
    f = pr.accuracy_figures(X, Y, rate, hop, n)
    print(f"{what}: yardstick {f['yardstick']:.3e}, GPU worst {f['worst']:.3e}, GPU / yardstick {f['worst'] / f['yardstick']:.3f}, "
          f"worst ratio to the cap {f['cap_ratio']:.4f}")
    assert f["worst"] <= pr.YARDSTICKS * f["yardstick"], (what, f)
    assert f["cap_ratio"] <= 1.0, (what, f)
    assert f["zeros_exact"], (what, f)
    return f


def max_grid(torch):
    """The launcher's grid limit: 64 workgroups per compute unit."""
    return 64 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("case", pr.edge_cases(), ids=pr.edge_id)
def test_accuracy_on_the_edge_cases(jsg, torch_cuda, case):
    """The bounds of test_accuracy_against_float64 on pr.edge_cases()."""
    n, hop, rate, T, kind = case
    X = pr.edge_input(case)
    Y = run(jsg, torch_cuda, X, rate, hop, n)[0].cpu().numpy()
    assert Y.shape == (pr.n_frames_out(T, rate), n // 2 + 1)
    f = pr.accuracy_figures(X, Y, rate, hop, n)
    print(f"{pr.edge_id(case)}: yardstick {f['yardstick']:.3e}, GPU worst {f['worst']:.3e}, GPU / yardstick {f['worst'] / f['yardstick']:.3f}, "
          f"worst ratio to the cap {f['cap_ratio']:.4f}, {f['n_zero']} zero elements exact: {f['zeros_exact']}")
    assert f["worst"] <= pr.YARDSTICKS * f["yardstick"]
    assert f["cap_ratio"] <= 1.0
    assert f["n_zero"] > 0 and f["zeros_exact"]
    assert f["n_nonzero"] > 0


def test_walks_take_more_items_than_the_grid(jsg, torch_cuda):
    """One output frame per chunk: both walk kernels get more than three times as many (row, chunk, tile) items as the grid has
    workgroups, and a ragged last round, so `item += gridDim.x` runs; eight rows."""
    torch = torch_cuda
    n, hop, rate, T, rows = 512, 128, 0.8, 1040, 8
    tiles = -(-(n // 2 + 1) // 64)
    T_out = jsg.pvoc_frames(T, rate)
    grid = max_grid(torch)
    assert T_out == 1300 and tiles == 5
    for items in (rows * T_out * tiles, rows * (T_out - 1) * tiles):        # the output walk, the walk of the chunk sums
        assert items >= 3 * grid and items % grid != 0, (items, grid)
    X = np.stack([pr.special_input(n, T, seed=r) if r < 4 else pr.make_input(n, hop, T, seed=r) for r in range(rows)])
    d_X = torch.from_numpy(X).cuda()
    base = run(jsg, torch, d_X, rate, hop, n)
    assert same_bits(torch, run(jsg, torch, d_X, rate, hop, n, chunk_frames=1), base)
    Y = base.cpu().numpy()
    for r in range(rows):
        assert_within_both_bounds(X[r], Y[r], rate, hop, n, f"row {r}")


@pytest.mark.parametrize("n", [2, 128])
def test_scan_takes_more_items_than_the_grid_and_the_row_limit(jsg, torch_cuda, n):
    """n = 2: 65535 rows, the most the header allows.  n = 128: two tiles per row and just over 1.5 grids of rows.  Either way the
    scan kernel gets more than three times as many (row, tile) items as the grid has workgroups and passes its barrier again with
    the LDS totals of the item before.  Row r holds input r mod 251, so the equality of rows is checked on the device; the 251
    distinct rows are held to the bounds as one case (their yardstick is the restatement's worst error over all of them: a row
    of 8 x 2 elements alone is too few to take a worst error from)."""
    torch = torch_cuda
    hop, rate, T, chunk, D = max(1, n // 4), 0.5, 4, 3, 251
    K = n // 2 + 1
    tiles = -(-K // 64)
    grid = max_grid(torch)
    rows = 65535 if n == 2 else (3 * grid + tiles) // tiles
    assert rows <= 65535 and rows * tiles >= 3 * grid and (rows * tiles) % grid != 0, (rows, tiles, grid)
    distinct = np.stack([pr.special_input(n, T, seed=q) if q % 2 == 0 else pr.make_input(n, hop, T, seed=q) for q in range(D)])
    idx = torch.arange(rows, device="cuda") % D
    d_X = torch.from_numpy(distinct).cuda()[idx]
    out = run(jsg, torch, d_X, rate, hop, n, chunk_frames=chunk)
    T_out = out.shape[1]
    assert T_out == 8 and -(-T_out // chunk) == 3
    assert torch.equal(bits(torch, out), bits(torch, out[:D])[idx])
    Y = out[:D].cpu().numpy()
    R = np.stack([pr.reference(distinct[q], rate, hop, n) for q in range(D)])
    S = np.stack([pr.restatement(distinct[q], rate, hop, n) for q in range(D)])
    yard, err = float(pr.rel_error(S, R).max()), pr.rel_error(Y, R)
    cap_ratio = float((err / pr.bound_cap(T_out)[None, :, None]).max())
    print(f"n {n}, {rows} rows: yardstick {yard:.3e}, GPU worst {err.max():.3e}, GPU / yardstick {err.max() / yard:.3f}, worst ratio to the cap {cap_ratio:.4f}")
    assert err.max() <= pr.YARDSTICKS * yard
    assert cap_ratio <= 1.0
    assert (np.abs(R) == 0).any() and (np.abs(R) > 0).any() and (Y[np.abs(R) == 0] == 0).all()
    for r in (0, grid - 1, grid, rows - 1):
        assert same_bits(torch, out[r], run(jsg, torch, d_X[r], rate, hop, n)[0]), r


# rate 0.8 has no T with 96 output frames (T = 76 gives 95, T = 77 gives 97), so it takes 95 (= 5 x 19) for the length that chunk
# lengths divide and the prime 97 like rate 1
@pytest.mark.parametrize("rate,T,T_out", [(1.0, 96, 96), (1.0, 97, 97), (0.8, 76, 95), (0.8, 77, 97)])
@pytest.mark.parametrize("n", [126, 128])
def test_same_bits_for_every_number_of_chunks(jsg, torch_cuda, n, rate, T, T_out):
    """Every chunk length from 1 to past T_out: every number of chunks from T_out down to 1, so every shape of the scan's 16 segments
    (one chunk per segment, empty segments, 15 / 16 / 17 and 31 / 32 / 33 chunks, the last chunk alone in its segment) and the
    launches of one and two chunks, where the first walk has nothing or one chunk to do."""
    torch = torch_cuda
    hop, K = n // 4, n // 2 + 1
    assert jsg.pvoc_frames(T, rate) == pr.n_frames_out(T, rate) == T_out
    X = np.stack([pr.special_input(n, T), pr.make_input(n, hop, T)])
    d_X = torch.from_numpy(X).cuda()
    sc = torch.empty(2 * T_out * K + 4, dtype=torch.int32, device="cuda")       # enough for one frame per chunk
    sc.fill_(-1)
    base = run(jsg, torch, d_X, rate, hop, n, chunk_frames=T_out, d_scratch=sc)
    Y = base.cpu().numpy()
    for r in range(2):
        assert_within_both_bounds(X[r], Y[r], rate, hop, n, f"n {n} rate {rate} T_out {T_out} row {r}")
    for chunk in list(range(1, T_out + 2)) + [1024, 65536]:
        sc.fill_(-1)
        assert same_bits(torch, run(jsg, torch, d_X, rate, hop, n, chunk_frames=chunk, d_scratch=sc), base), chunk


@pytest.mark.parametrize("rate", [0.8, 1.3])
def test_tightest_pitches_equal_dense_and_padding_is_untouched(jsg, torch_cuda, rate):
    """in_row_pitch = (T - 1) in_frame_pitch + K, the smallest the header allows: the next row starts inside the padding of the last
    frame.  The same for out."""
    torch = torch_cuda
    n, hop, T, rows = 130, 32, 150, 3
    K = n // 2 + 1
    X = np.stack([pr.special_input(n, T)] + [pr.make_input(n, hop, T, seed=s) for s in (1, 2)])
    dense = run(jsg, torch, X, rate, hop, n)
    T_out = dense.shape[1]

    def tight(frames, frame_pitch):
        row_pitch = (frames - 1) * frame_pitch + K
        flat = torch.full((rows * row_pitch,), POISON, dtype=torch.complex64, device="cuda")
        return flat, torch.as_strided(flat, (rows, frames, K), (row_pitch, frame_pitch, 1))

    flat_in, v_in = tight(T, K + 7)
    v_in.copy_(torch.from_numpy(X).cuda())
    flat_out, v_out = tight(T_out, K + 5)
    assert v_in.stride() == ((T - 1) * (K + 7) + K, K + 7, 1) and v_out.stride() == ((T_out - 1) * (K + 5) + K, K + 5, 1)
    jsg.phase_vocoder_launch(v_in, rate, hop, n, v_out, chunk_frames=33)
    torch.cuda.synchronize()
    assert same_bits(torch, v_out, dense)
    padding = torch.ones(flat_out.shape, dtype=torch.bool, device="cuda")
    torch.as_strided(padding, v_out.shape, v_out.stride()).fill_(False)
    assert padding.sum().item() == flat_out.numel() - rows * T_out * K
    assert torch.equal(bits(torch, flat_out)[padding], bits(torch, torch.full_like(flat_out, POISON))[padding])


@pytest.mark.parametrize("rate", [0.8, 1.0, 2.0])
def test_inf_stays_in_its_bin_and_in_the_frames_that_read_it(jsg, torch_cuda, rate):
    """inf + 0j at (j, k): an infinite modulus and, by IEEE, the angle +0 of 1 + 0j.  So other bins and earlier frames are untouched,
    the frames that interpolate it are not finite, and the frames after it have the bits of a launch with 1 + 0j in its place."""
    torch = torch_cuda
    n, hop, T, j_inf, k_inf = 512, 128, 240, 101, 77
    X = pr.make_input(n, hop, T)
    assert X[j_inf, k_inf] != 0 and X[j_inf - 1, k_inf] != 0 and X[j_inf + 1, k_inf] != 0
    clean = run(jsg, torch, X, rate, hop, n, chunk_frames=16)
    Xi, X1 = X.copy(), X.copy()
    Xi[j_inf, k_inf] = complex(np.inf, 0.0)
    X1[j_inf, k_inf] = complex(1.0, 0.0)
    dirty, one = run(jsg, torch, Xi, rate, hop, n, chunk_frames=16), run(jsg, torch, X1, rate, hop, n, chunk_frames=16)
    others = [k for k in range(n // 2 + 1) if k != k_inf]
    assert same_bits(torch, dirty[:, :, others], clean[:, :, others])
    j = np.floor(np.arange(clean.shape[1], dtype=np.float64) * rate)
    before, reads, after = (torch.from_numpy(m).cuda() for m in (j + 1 < j_inf, (j == j_inf) | (j + 1 == j_inf), j > j_inf))
    assert before.any() and reads.any() and after.any()
    assert same_bits(torch, dirty[0, before][:, k_inf], clean[0, before][:, k_inf])
    assert not torch.isfinite(torch.view_as_real(dirty[0, reads][:, k_inf])).all(dim=-1).any()
    assert torch.isfinite(torch.view_as_real(one[0, :, k_inf])).all()
    assert same_bits(torch, dirty[0, after][:, k_inf], one[0, after][:, k_inf])


def test_python_phase_vocoder_on_what_torch_stft_returns(jsg, torch_cuda):
    """A contiguous [..., bins, frames] tensor (the copy branch), complex128, and an unbatched [bins, frames] tensor."""
    torch = torch_cuda
    n, hop, rate, T = 130, 32, 1.3, 90
    K = n // 2 + 1
    X = np.stack([pr.special_input(n, T), pr.make_input(n, hop, T)])
    d_frames = torch.from_numpy(X).cuda()                                   # [2][T][K]
    view = d_frames.transpose(-1, -2)                                       # bins with stride 1: no copy
    want = jsg.phase_vocoder(view, rate, hop)
    T_out = pr.n_frames_out(T, rate)
    assert want.shape == (2, K, T_out)
    assert same_bits(torch, want.transpose(-1, -2), run(jsg, torch, d_frames, rate, hop, n))
    packed = view.contiguous()                                              # as torch.stft returns it: frames with stride 1
    assert packed.stride() == (K * T, T, 1)
    assert same_bits(torch, jsg.phase_vocoder(packed, rate, hop), want)
    wide = torch.randn((2, K, T, 2), dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    wide = torch.view_as_complex(wide)
    got = jsg.phase_vocoder(wide, rate, hop)
    assert got.dtype == torch.complex64 and same_bits(torch, got, jsg.phase_vocoder(wide.to(torch.complex64), rate, hop))
    single = jsg.phase_vocoder(packed[1], rate, hop)
    assert single.shape == (K, T_out) and same_bits(torch, single, want[1])
    torch.cuda.synchronize()
