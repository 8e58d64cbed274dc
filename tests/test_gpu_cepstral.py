"""Cepstral coefficients and delta features on the GPU (include/jsg.h section 2k) against tests/cepstral_ref.py: graph capture of a
first mfcc -> delta chain, the projection to the bit in pitched buffers with NaN around the input and sentinels around the output over
the band, coefficient and frame corners, at the table limit and on every path of jsg_mfcc_plan, identical bits over chunk lengths,
pitches, offsets and row counts, 65 535 rows, NaN and infinity containment; delta to the bit over widths, orders, modes, lengths and
coefficient counts; and the Python layer down to mfcc_audio."""
import numpy as np
import pytest

import cepstral_ref as cr
from cepstral_ref import same, same_but_nan, raw

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def strides_of(shape, pads):
    strides = [1]
    for n, pad in zip(reversed(shape[1:]), reversed(pads)):
        strides.append(strides[-1] * n + pad)
    return tuple(reversed(strides))


def pitched_in(torch, x, pads, offset):
    """x numpy [..] -> a CUDA view of it whose axes lie pads[i] elements apart beyond their length (last axis: unit stride), starting
    `offset` floats into an allocation that holds NaN everywhere else."""
    strides = strides_of(x.shape, pads)
    size = offset + sum((n - 1) * s for n, s in zip(x.shape, strides)) + 1
    flat = torch.full((size,), float("nan"), dtype=torch.float32, device="cuda")
    view = torch.as_strided(flat, x.shape, strides, storage_offset=offset)
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def pitched_out(torch, shape, pads, offset):
    """(allocation filled with the sentinel, view of `shape` into it, flat indices of the view's elements)."""
    strides = strides_of(shape, pads)
    size = offset + sum((n - 1) * s for n, s in zip(shape, strides)) + 1 + 3
    flat = torch.full((size,), SENTINEL.item(), dtype=torch.float32, device="cuda")
    at = offset + sum(np.arange(n).reshape([-1 if i == k else 1 for i in range(len(shape))]) * s for k, (n, s) in enumerate(zip(shape, strides)))
    return flat, torch.as_strided(flat, shape, strides, storage_offset=offset), at


def collect(flat, at, what):
    """The view's elements, after checking that every other element of the allocation still holds the sentinel."""
    got = flat.cpu().numpy()
    written = np.zeros(got.size, bool)
    written[at.ravel()] = True
    assert (got[~written] == SENTINEL).all(), what
    return got[at]


def run_mfcc(jsg, torch, S, D, *, chunk_frames=0, pad_frame=0, pad_row=0, pad_out=0, pad_out_row=0, offset=0, out_offset=None):
    S = S if S.ndim == 3 else S[None]
    d_in = pitched_in(torch, S, (pad_row, pad_frame), offset)
    d_table = torch.from_numpy(np.array(D, np.float32)).cuda()
    flat, view, at = pitched_out(torch, S.shape[:2] + (D.shape[0],), (pad_out_row, pad_out), offset if out_offset is None else out_offset)
    jsg.mfcc_launch(d_in, d_table, view, chunk_frames=chunk_frames)
    torch.cuda.synchronize()
    return collect(flat, at, "mfcc")


def run_delta(jsg, torch, X, w, mode, *, pad_frame=0, pad_row=0, pad_out=0, pad_out_row=0, offset=0):
    X = X if X.ndim == 3 else X[None]
    d_in = pitched_in(torch, X, (pad_row, pad_frame), offset)
    d_w = torch.from_numpy(np.array(w, np.float32)).cuda()
    flat, view, at = pitched_out(torch, X.shape, (pad_out_row, pad_out), offset)
    jsg.delta_launch(d_in, d_w, view, mode="interp" if mode == cr.INTERP else "nearest")
    torch.cuda.synchronize()
    return collect(flat, at, "delta")


def check_projection(got, S, D, what):
    """The bits of the restatement, and the stated bound against float64 (which the restatement meets on the CPU)."""
    want = cr.project32(S, D)
    assert same(got, want), (what, int((raw(got) != raw(want)).sum()), got.size)
    C64, bound = cr.project64(S, D)
    assert (np.abs(got.astype(np.float64) - C64) <= bound).all(), what


def check_delta(got, X, w, mode, what):
    want = cr.delta32(X, w, mode)
    assert same(got, want), (what, int((raw(got) != raw(want)).sum()), got.size)
    Y64, bound = cr.delta64(X, w, mode)
    assert (np.abs(got.astype(np.float64) - Y64) <= bound).all(), what


def test_graph_capture_of_a_first_chain(jsg, torch_cuda):
    """The first launches of the two kernels in this process (this test comes first in the file and no other file launches them) sit
    inside a capture, mfcc -> delta on one stream; replayed twice, equals eager."""
    torch = torch_cuda
    S = np.array(cr.planes()[:2, :100, :128])
    D, w = jsg.mfcc_table(128, 20), jsg.delta_weights(9, 1)
    d_S, d_D, d_w = torch.from_numpy(S).cuda(), torch.from_numpy(D).cuda(), torch.from_numpy(w).cuda()
    d_C = torch.zeros((2, 100, 20), dtype=torch.float32, device="cuda")
    d_Y = torch.zeros((2, 100, 20), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        jsg.mfcc_launch(d_S, d_D, d_C, stream=s.cuda_stream)
        jsg.delta_launch(d_C, d_w, d_Y, stream=s.cuda_stream)
    assert jsg.mfcc_kernel_name(d_S, d_D, d_C) == "mfcc_block5"
    C = run_mfcc(jsg, torch, S, D)
    Y = run_delta(jsg, torch, C, w, cr.INTERP)
    for _ in range(2):
        d_C.zero_()
        d_Y.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(d_C.cpu().numpy(), C) and same(d_Y.cpu().numpy(), Y)
    check_projection(C, S, D, "capture")
    check_delta(Y, C, w, cr.INTERP, "capture")


def test_first_mfcc_launch_of_a_path_with_more_than_48_kib_of_lds(jsg, torch_cuda):
    """The first launch of the 16-coefficient path in this process (only the capture above precedes it, on another path) asks for more
    dynamic LDS than a kernel may have without saying so: the launch itself has to say it."""
    torch = torch_cuda
    S = np.array(cr.planes()[:2, :3, :128])
    D = cr.tables(128, 128)
    name, _, lds = jsg.mfcc_plan(torch.from_numpy(S).cuda(), torch.from_numpy(np.array(D)).cuda(), torch.empty((2, 3, 128), dtype=torch.float32, device="cuda"))
    assert name == "mfcc_block16" and lds > 49152, (name, lds)
    check_projection(run_mfcc(jsg, torch, S, D, pad_frame=4, pad_out=1), S, D, "128 x 128, first on its path")


# ---------------------------------------------------------------------------------------------------- the projection
@pytest.mark.parametrize("B", [1, 2, 3, 31, 32, 33, 64, 65, 128, 257])
def test_mfcc_bits_equal_the_restatement(jsg, torch_cuda, B):
    for i, M in enumerate(sorted({1, 2, 13, 20, B})):
        if M * B > 32768:
            continue
        D = cr.tables(M, B)
        for T in (1, 2, 63, 64, 65, 200):
            S = cr.planes()[:2, :T, :B]
            # multiples of four (the 16-byte loads where B allows) and odd ones in turn
            pf, pr, off = ((0, 0, 0), (4, 8, 4), (1, 3, 1), (0, 5, 2))[(i + T) % 4]
            got = run_mfcc(jsg, torch_cuda, S, D, pad_frame=pf, pad_row=pr, pad_out=(T + M) % 3, pad_out_row=M % 2, offset=off)
            check_projection(got, S, D, (B, M, T))


@pytest.mark.parametrize("B,M,T", [(128, 256, 50), (256, 128, 70), (20, 128, 130), (13, 40, 65), (4096, 8, 3), (8, 4096, 5), (181, 181, 66)])
def test_mfcc_at_the_table_limit_and_inverse_shapes(jsg, torch_cuda, B, M, T):
    torch = torch_cuda
    rng = np.random.default_rng(B + M)
    S = (-40.0 + 12.0 * rng.standard_normal((2, T, B))).astype(np.float32)
    D = cr.tables(M, B, seed=3)
    d_S, d_D = torch.from_numpy(S).cuda(), torch.from_numpy(np.array(D)).cuda()
    name, F, lds = jsg.mfcc_plan(d_S, d_D, torch.empty((2, T, M), dtype=torch.float32, device="cuda"))
    assert lds <= 163840 and F == max(1, min(64, T, (40960 - B * M) // ((B | 1) + (M | 1))))
    assert F < min(64, T) or B * M < 20000              # the large tables leave room for fewer frames
    got = run_mfcc(jsg, torch, S, D, pad_frame=4 * (B % 2), pad_out=1)
    check_projection(got, S, D, (B, M, T, name, F))


def test_mfcc_on_every_path_of_the_plan(jsg, torch_cuda):
    torch = torch_cuda
    seen = set()
    S = cr.planes()[:2, :70, :32]
    d_S = torch.from_numpy(np.array(S)).cuda()
    for M in (3, 4, 5, 16, 17, 20, 21, 32, 33, 40, 41, 64, 65):
        D = cr.tables(M, 32, seed=1)
        name = jsg.mfcc_kernel_name(d_S, torch.from_numpy(np.array(D)).cuda(), torch.empty((2, 70, M), dtype=torch.float32, device="cuda"))
        seen.add(name)
        assert name == "mfcc_block%d" % next((mb for mb in (4, 5, 8, 10, 16) if 4 * mb >= M), 16)
        check_projection(run_mfcc(jsg, torch, S, D, pad_out=2), S, D, (M, name))
    assert len(seen) == 5


def test_mfcc_bits_do_not_depend_on_chunks_pitches_offsets_or_rows(jsg, torch_cuda):
    torch = torch_cuda
    S = np.array(cr.planes()[:3, :150, :128])
    D = jsg.mfcc_table(128, 20, lifter=22.0)
    base = run_mfcc(jsg, torch, S, D)
    check_projection(base, S, D, "base")
    for chunk in (1, 3, 63, 64, 65, 65536):
        assert same(run_mfcc(jsg, torch, S, D, chunk_frames=chunk), base), chunk
    d_S, d_D, d_o = torch.from_numpy(S).cuda(), torch.from_numpy(D).cuda(), torch.empty((3, 150, 20), dtype=torch.float32, device="cuda")
    assert [jsg.mfcc_plan(d_S, d_D, d_o, chunk_frames=c)[1] for c in (0, 1, 3, 64, 65536)] == [64, 1, 3, 64, 64]
    # a base that is only 4-byte aligned, pitches that are no multiple of four, an output elsewhere in its allocation
    for kw in (dict(offset=1), dict(offset=2, pad_frame=4), dict(offset=4, pad_frame=3), dict(pad_frame=4, pad_row=6), dict(pad_frame=8, pad_row=16, pad_out=5, pad_out_row=7),
               dict(offset=4, out_offset=3, pad_out=12)):
        assert same(run_mfcc(jsg, torch, S, D, **kw), base), kw
    for r in range(3):
        assert same(run_mfcc(jsg, torch, S[r], D), base[r:r + 1]), r
    assert same(run_mfcc(jsg, torch, S[:, 17:88], D), base[:, 17:88])           # nor on the frame index


def test_mfcc_65535_rows(jsg, torch_cuda):
    base = np.array(cr.planes()[:3, :2, :3])
    D = cr.tables(2, 3)
    three = run_mfcc(jsg, torch_cuda, base, D)
    check_projection(three, base, D, "three rows")
    S = np.tile(base, (21845, 1, 1))
    assert S.shape[0] == 65535
    got = run_mfcc(jsg, torch_cuda, S, D, pad_row=1, pad_out_row=2)
    assert same(got, np.tile(three, (21845, 1, 1)))


def test_mfcc_nan_and_infinity_stay_in_their_frame(jsg, torch_cuda):
    S0 = np.array(cr.planes()[:2, :130, :128])
    D = np.array(jsg.mfcc_table(128, 20))
    D[3, 77] = 0                                      # a zero in the table does not stop a NaN
    clean = run_mfcc(jsg, torch_cuda, S0, D)
    for (t0, b0), bad in zip(((0, 0), (63, 127), (64, 77), (129, 5)), (np.nan, np.inf, np.nan, -np.inf)):
        S = S0.copy()
        S[1, t0, b0] = bad
        got = run_mfcc(jsg, torch_cuda, S, D)
        assert same(got[0], clean[0]) and same(np.delete(got[1], t0, axis=0), np.delete(clean[1], t0, axis=0)), (t0, b0)
        assert same_but_nan(got, cr.project32(S, D)), (t0, b0)
        if np.isnan(bad):
            assert np.isnan(got[1, t0]).all()
        else:
            assert (~np.isfinite(got[1, t0])).sum() >= 19     # every coefficient whose table entry at b0 is not zero, as the chain gives them


# ---------------------------------------------------------------------------------------------------- delta
@pytest.mark.parametrize("width", [3, 5, 9, 255])
@pytest.mark.parametrize("order", [1, 2])
def test_delta_bits_equal_the_restatement(jsg, torch_cuda, width, order):
    w = jsg.delta_weights(width, order)
    long = np.concatenate([cr.planes(), cr.planes()[:, ::-1]], axis=1)      # 400 frames
    for mode in (cr.INTERP, cr.NEAREST):
        for T in sorted({1, width, width + 1, 200}):
            if mode == cr.INTERP and T < width:
                continue
            for i, M in enumerate((1, 13, 20, 65)):
                X = long[:2, :T, :M]
                got = run_delta(jsg, torch_cuda, X, w, mode, pad_frame=(i + T) % 3, pad_row=i % 2 * 5, pad_out=(T + M) % 2, pad_out_row=i, offset=i % 3)
                check_delta(got, X, w, mode, (width, order, mode, T, M))


def test_delta_wide_planes_pitches_and_rows(jsg, torch_cuda):
    """More coefficients than a workgroup has threads, and than an item has elements; then identical bits over pitches and row counts."""
    w = jsg.delta_weights(5, 2)
    rng = np.random.default_rng(11)
    for M, T in ((257, 9), (300, 20), (4097, 6), (65536, 5)):
        X = rng.standard_normal((2, T, M)).astype(np.float32)
        for mode in (cr.INTERP, cr.NEAREST):
            check_delta(run_delta(jsg, torch_cuda, X, w, mode, pad_frame=M % 2), X, w, mode, (M, T, mode))
    X = np.array(cr.planes()[:3, :, :20])
    w = jsg.delta_weights(9, 1)
    base = run_delta(jsg, torch_cuda, X, w, cr.INTERP)
    for kw in (dict(offset=1), dict(pad_frame=3, pad_row=7), dict(pad_out=4, pad_out_row=1, offset=2)):
        assert same(run_delta(jsg, torch_cuda, X, w, cr.INTERP, **kw), base), kw
    for r in range(3):
        assert same(run_delta(jsg, torch_cuda, X[r], w, cr.INTERP), base[r:r + 1])
    # the interior does not depend on the frame index or the frame count
    assert same(run_delta(jsg, torch_cuda, X[:, 30:90], w, cr.INTERP)[:, 4:-4], base[:, 34:86])


def test_delta_65535_rows(jsg, torch_cuda):
    base = np.array(cr.planes()[:3, :4, :2])
    w = jsg.delta_weights(3, 1)
    three = run_delta(jsg, torch_cuda, base, w, cr.INTERP)
    check_delta(three, base, w, cr.INTERP, "three rows")
    got = run_delta(jsg, torch_cuda, np.tile(base, (21845, 1, 1)), w, cr.INTERP, pad_row=1)
    assert same(got, np.tile(three, (21845, 1, 1)))


@pytest.mark.parametrize("mode", [cr.INTERP, cr.NEAREST])
def test_delta_nan_reaches_the_frames_whose_window_holds_it(jsg, torch_cuda, mode):
    X0 = np.array(cr.planes()[:2, :40, :13])
    w = jsg.delta_weights(9, 2)                       # no zero weight
    assert (w != 0).all()
    clean = run_delta(jsg, torch_cuda, X0, w, mode)
    idx = cr.window_frames(40, 9, mode)
    for t0, m0 in ((0, 0), (3, 12), (20, 5), (39, 7)):
        X = X0.copy()
        X[1, t0, m0] = np.nan
        got = run_delta(jsg, torch_cuda, X, w, mode)
        hit = np.zeros((2, 40, 13), bool)
        hit[1, (idx == t0).any(axis=1), m0] = True
        assert np.array_equal(np.isnan(got), hit), (t0, m0)
        assert same(got[~hit], clean[~hit])
        assert same_but_nan(got, cr.delta32(X, w, mode))


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_mfcc_audio_is_mfcc_of_the_mel_plane(jsg, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(3)
    sr = 22050
    t = np.arange(2048 + 512 * 40) / sr
    x = (0.5 * np.sin(2 * np.pi * 440 * t) + 0.05 * rng.standard_normal(t.size)).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    S = jsg.mel_spectrogram_db(d_x, sr, 2048, 512, 128)
    assert S.shape == (41, 128)
    for lifter in (0.0, 22.0):
        want = jsg.mfcc(S, 20, "ortho", lifter)
        got = jsg.mfcc_audio(d_x, sr, lifter=lifter)
        assert got.is_cuda and got.shape == (41, 20) and same(got.cpu().numpy(), want.cpu().numpy())
        host = jsg.mfcc_audio(x, sr, lifter=lifter)
        assert isinstance(host, np.ndarray) and same(host, want.cpu().numpy())
        check_projection(want.cpu().numpy()[None], S.cpu().numpy()[None], jsg.mfcc_table(128, 20, "ortho", lifter), lifter)
    got = jsg.mfcc_audio(d_x, sr, n_mfcc=13, n_mels=40, fmin=50.0, fmax=8000.0)
    assert same(got.cpu().numpy(), jsg.mfcc(jsg.mel_spectrogram_db(d_x, sr, 2048, 512, 40, 50.0, 8000.0), 13).cpu().numpy())


@pytest.mark.parametrize("norm,lifter", [("ortho", 0.0), ("ortho", 22.0), ("none", 0.0)])
def test_mfcc_round_trip_returns_the_plane(jsg, torch_cuda, norm, lifter):
    """mfcc_to_mel_db(mfcc(S, n_mfcc = n_mels)) = S within the sum of the two stated bounds: the first, carried through |I|, and the
    second on the coefficients the GPU returned."""
    S = np.array(cr.planes()[:2, :70, :128])
    Cg = jsg.mfcc(S, n_mfcc=128, norm=norm, lifter=lifter)
    back = jsg.mfcc_to_mel_db(Cg, n_mels=128, norm=norm, lifter=lifter)
    assert isinstance(back, np.ndarray) and back.shape == S.shape and back.dtype == np.float32
    D, I = jsg.mfcc_table(128, 128, norm, lifter), jsg.mfcc_table(128, 128, norm, lifter, inverse=True)
    _, bound1 = cr.project64(S, D)
    _, bound2 = cr.project64(Cg, I)
    total = bound1 @ np.abs(I.astype(np.float64)).T + bound2
    err = np.abs(back.astype(np.float64) - S.astype(np.float64))
    print(f"round trip {norm} lifter {lifter}: worst error {err.max():.3e}, in units of the bound {np.max(err / total):.4f}")
    assert (err <= total).all()
    # batch axes and CUDA in, CUDA out
    import torch
    d = torch.from_numpy(S.reshape(2, 1, 70, 128)).cuda()
    assert same(jsg.mfcc(d, 128, norm, lifter).cpu().numpy().reshape(2, 70, 128), Cg)


def test_delta_of_a_line_is_its_slope(jsg, torch_cuda):
    """X[t][m] = a_m + s_m t with values that float32 holds exactly.  The GPU against the slope (order 1) or zero (order 2), on the frames
    whose window lies on the line: the stated bound.  Beside that, the GPU against the float64 sum of the same float32 weights (the
    stated bound again), and that sum against the slope: the weights fit a line exactly before their one rounding (u, relative), so
    u sum |w| |X|."""
    t = np.arange(60, dtype=np.float64)[:, None]
    slope = np.array([0.25, -1.5, 3.0, 0.0, 0.125])[None, :]
    X = (np.array([3.0, -40.0, 0.5, 7.0, -2.0])[None, :] + slope * t).astype(np.float32)
    assert (X.astype(np.float64) == np.array([3.0, -40.0, 0.5, 7.0, -2.0])[None, :] + slope * t).all()
    for mode in ("interp", "nearest"):
        for order, want in ((1, np.broadcast_to(slope, X.shape)), (2, np.zeros(X.shape))):
            got = jsg.delta(X, 9, order, mode)
            assert isinstance(got, np.ndarray) and got.shape == X.shape and got.dtype == np.float32
            w = jsg.delta_weights(9, order)
            code = cr.INTERP if mode == "interp" else cr.NEAREST
            Y64, bound = cr.delta64(X, w, code)
            inside = slice(None) if mode == "interp" else slice(4, -4)            # repeated edge frames are not on the line
            direct = np.abs(got.astype(np.float64) - want)
            print(f"delta of a line, {mode}, order {order}: worst |got - want| in units of the bound {np.max(direct[inside][bound[inside] > 0] / bound[inside][bound[inside] > 0]):.3f}")
            assert (direct[inside] <= bound[inside]).all(), (mode, order)
            assert (np.abs(got.astype(np.float64) - Y64) <= bound).all()
            # bound / (Wd + 2) = u sum |w| |X|; the 1.001: its second order, and that Y64 is itself summed in float64
            assert (np.abs(Y64 - want)[inside] <= 1.001 * (bound / 11)[inside]).all(), (mode, order)
            assert same(got, cr.delta32(X, w, code))
    import torch
    d = torch.from_numpy(X[None, None]).cuda()
    assert same(jsg.delta(d).cpu().numpy()[0, 0], jsg.delta(X))
    with pytest.raises(jsg.JsgError):
        jsg.delta(X[:8])                                # interp needs width frames
    with pytest.raises(jsg.JsgError):
        jsg.delta(X, mode="reflect")
