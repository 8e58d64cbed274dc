"""Spectral shape descriptors on the GPU (include/jsg.h section 2l) against tests/spectral_ref.py: the GPU's bits equal the numpy
restatement of the stated orders.  A graph capture whose first launch is this kernel; pitched buffers (the input a view into NaN, the
outputs views into sentinels that must stay) over the bin corners and both sides of every path boundary of jsg_spectral_shape_plan,
the frame corners of a workgroup, more work than the grid holds, 1 to 65 535 rows; identical bits whichever outputs are NULL; the rolloff
on integer frames that reach the threshold exactly at a chosen bin; zero, denormal, NaN and infinite frames; the Python layer down to
spectral_shape_audio."""
import numpy as np
import pytest

import spectral_ref as sr
from spectral_ref import OUTPUTS

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
SENTINEL_BIN = -77777


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


def pitched_out(torch, shape, pads, offset, name):
    """(allocation filled with the sentinel, view of `shape` into it, flat indices of the view's elements)."""
    strides = strides_of(shape, pads)
    size = offset + sum((n - 1) * s for n, s in zip(shape, strides)) + 1 + 3
    if name == "rolloff_bin":
        flat = torch.full((size,), SENTINEL_BIN, dtype=torch.int32, device="cuda")
    else:
        flat = torch.full((size,), SENTINEL.item(), dtype=torch.float32, device="cuda")
    at = offset + sum(np.arange(n).reshape([-1 if i == k else 1 for i in range(len(shape))]) * s for k, (n, s) in enumerate(zip(shape, strides)))
    return flat, torch.as_strided(flat, shape, strides, storage_offset=offset), at


def collect(flat, at, name):
    """The view's elements, after checking that every other element of the allocation still holds the sentinel."""
    got = flat.cpu().numpy()
    written = np.zeros(got.size, bool)
    written[at.ravel()] = True
    assert (got[~written] == (SENTINEL_BIN if name == "rolloff_bin" else SENTINEL)).all(), name
    return got[at]


def run(jsg, torch, S, f, roll=0.85, names=OUTPUTS, *, pad_frame=0, pad_row=0, pad_out=0, offset=0, out_offset=0):
    """One launch over S [T][K] or [R][T][K] in pitched buffers -> dict of [R][T] arrays."""
    S = S if S.ndim == 3 else S[None]
    d_in = pitched_in(torch, S, (pad_row, pad_frame), offset)
    d_f = torch.from_numpy(np.array(f, np.float32)).cuda()
    outs = {n: pitched_out(torch, S.shape[:2], (pad_out,), out_offset, n) for n in names}
    jsg.spectral_shape_launch(d_in, d_f, roll_percent=roll, **{"d_" + n: view for n, (_, view, _) in outs.items()})
    torch.cuda.synchronize()
    return {n: collect(flat, at, n) for n, (flat, _, at) in outs.items()}


def check(got, S, f, roll=0.85, what=None):
    S = S if S.ndim == 3 else S[None]
    want = sr.shape32(S, f, roll)
    names = tuple(got)
    bad = sr.same_outputs(got, want, names)
    assert not bad, (what, bad, {n: int((sr.raw(got[n]) != sr.raw(want[n])).sum()) for n in bad}, got[names[0]].size)
    return want


def layout(i):
    """Pads and offsets in turn: dense, multiples of four, odd ones (an input at an odd float offset is not 16-byte aligned)."""
    pf, pr, po, off, ooff = ((0, 0, 0, 0, 0), (4, 8, 4, 4, 0), (1, 3, 1, 1, 3), (0, 5, 2, 3, 1))[i % 4]
    return dict(pad_frame=pf, pad_row=pr, pad_out=po, offset=off, out_offset=ooff)


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The first launch of the kernel in this process (this test comes first in the file and no other file launches it) sits inside a
    capture; replayed once, equals the eager launch and the restatement."""
    torch = torch_cuda
    K = 257
    S, f = np.array(sr.planes(2, 70, K)), sr.freqs(K)
    d_S, d_f = torch.from_numpy(S).cuda(), torch.from_numpy(np.array(f)).cuda()
    outs = {n: torch.zeros((2, 70), dtype=torch.int32 if n == "rolloff_bin" else torch.float32, device="cuda") for n in OUTPUTS}
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        jsg.spectral_shape_launch(d_S, d_f, stream=s.cuda_stream, **{"d_" + n: o for n, o in outs.items()})
    assert jsg.spectral_shape_kernel_name(d_S, d_f, d_energy=outs["energy"]) == "spectral_regs9"
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = {n: o.cpu().numpy() for n, o in outs.items()}
    check(got, S, f, what="capture")
    eager = run(jsg, torch, S, f)
    assert not sr.same_outputs(got, eager)


# both sides of every boundary of the plan (64 n | 64 n + 1 for the register paths 1, 2, 4, 9, 17, 33, 65), the lane-count corners below
# 64, and the engine's transforms (257, 513, 1025, 2049, 4097)
BINS = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 513, 576, 577, 1025, 1088, 1089, 2049, 2112, 2113, 4097, 4160, 4161]


@pytest.mark.parametrize("i,K", list(enumerate(BINS)))
def test_bits_equal_the_restatement_over_the_bins(jsg, torch_cuda, i, K):
    torch = torch_cuda
    path, W, FK = sr.plan(K)
    T = min(2 * FK * 256 // W + 3, 37 if K > 600 else 150)
    S, f = sr.planes(2, T, K), sr.freqs(K)
    d = torch.zeros((2, T, K), device="cuda")
    assert jsg.spectral_shape_plan(d, torch.zeros(K, device="cuda"), d_crest=torch.zeros((2, T), device="cuda")) == (path, W, FK, 0)
    got = run(jsg, torch, S, f, **layout(i))
    want = check(got, S, f, what=(K, path))
    # ... and the stated bounds against float64 (which the restatement meets on the CPU)
    w64, bound = sr.shape64(S, f), sr.bounds(K)
    for name in ("energy", "centroid"):
        assert (np.abs(got[name].astype(np.float64) - w64[name]) <= bound[name] * np.abs(w64[name])).all(), (K, name)
    assert want["rolloff_bin"].min() >= 0 and want["rolloff_bin"].max() < K


def test_the_largest_frame(jsg, torch_cuda):
    K = 65536
    S, f = sr.planes(1, 2, K), sr.freqs(K)
    check(run(jsg, torch_cuda, S, f, pad_frame=1, offset=1), S, f, what="65536 bins")


@pytest.mark.parametrize("K", [1, 5, 40, 129, 1025, 4200])
def test_frame_corners_of_a_workgroup(jsg, torch_cuda, K):
    """1 frame, and the frames a workgroup takes per step (frames in flight x 256 / lanes) and one fewer and one more."""
    _, W, FK = sr.plan(K)
    per = FK * 256 // W
    f = sr.freqs(K)
    for i, T in enumerate(sorted({1, 2, per - 1, per, per + 1})):
        if T < 1:
            continue
        S = sr.planes(2, T, K)
        check(run(jsg, torch_cuda, S, f, **layout(i + K)), S, f, what=(K, T))


def test_more_work_than_the_grid_holds(jsg, torch_cuda):
    """3 rows of 22 000 frames of 40 bins are 2064 work items of 32 frames; the grid is at most 8 workgroups per compute unit."""
    torch = torch_cuda
    K, T, R = 40, 22000, 3
    assert R * -(-T // 32) > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    S, f = sr.planes(R, T, K), sr.freqs(K)
    check(run(jsg, torch, S, f, pad_frame=1, pad_row=7, pad_out=5, offset=2), S, f, what="grid stride")


@pytest.mark.parametrize("R", [1, 2, 3])
def test_rows(jsg, torch_cuda, R):
    for i, K in enumerate((33, 300)):
        S, f = sr.planes(R, 21, K), sr.freqs(K)
        got = run(jsg, torch_cuda, S, f, **layout(R + i))
        check(got, S, f, what=(R, K))
        # a row's results do not depend on the other rows
        alone = run(jsg, torch_cuda, S[R - 1], f)
        assert not sr.same_outputs({n: v[R - 1:] for n, v in got.items()}, alone)


def test_65535_rows(jsg, torch_cuda):
    S, f = sr.planes(65535, 1, 5), sr.freqs(5)
    check(run(jsg, torch_cuda, S, f, pad_row=1, pad_out=2), S, f, what="65535 rows")


@pytest.mark.parametrize("K", [40, 257, 2049, 4200])
def test_which_outputs_are_null_does_not_change_a_bit(jsg, torch_cuda, K):
    S, f = sr.planes(2, 19, K), sr.freqs(K)
    every = run(jsg, torch_cuda, S, f, 0.7)
    check(every, S, f, 0.7, what=K)
    for name in OUTPUTS:
        alone = run(jsg, torch_cuda, S, f, 0.7, (name,), pad_out=3, out_offset=1)
        assert not sr.same_outputs(alone, every, (name,)), (K, name)
    pair = run(jsg, torch_cuda, S, f, 0.7, ("rolloff_bin", "spread"))
    assert not sr.same_outputs(pair, every, ("rolloff_bin", "spread"))


@pytest.mark.parametrize("K", [20, 64, 200, 1025, 4200])
def test_rolloff_reaches_the_threshold_exactly_at_a_chosen_bin(jsg, torch_cuda, K):
    """Integer frames (every sum exact): a one at bin k and a one at the last bin.  With p = 1/2 and with a tiny p the threshold is met
    exactly at k and cum then stays on it over a plateau of zeros: the lowest bin wins; with p = 1 and p = 0.85 at the last bin.  The
    table descends and is shuffled: the bin is searched, not the frequency."""
    W = sr.lanes(K)
    chosen = sorted({k for k in (0, W - 1, W, (K // (2 * W)) * W, (K // (2 * W)) * W - 1, K // 2, K - 1) if 0 <= k < K})
    S = np.zeros((len(chosen), K), np.float32)
    S[:, K - 1] = 1.0
    S[np.arange(len(chosen)), chosen] = 1.0
    f = np.random.default_rng(K).permutation(np.arange(K, 0, -1)).astype(np.float32)
    for roll, at in ((0.5, chosen), (1e-30, chosen), (1.0, [K - 1] * len(chosen)), (0.85, [K - 1] * len(chosen))):
        got = run(jsg, torch_cuda, S, f, roll, pad_frame=1, offset=1)
        check(got, S, f, roll, what=(K, roll))
        assert got["rolloff_bin"][0].tolist() == list(at), (K, roll)
        assert np.array_equal(got["rolloff"][0], f[list(at)])


@pytest.mark.parametrize("K", [33, 257, 4200])
def test_zero_denormal_nan_and_infinite_frames(jsg, torch_cuda, K):
    f = sr.freqs(K)
    S = np.array(sr.planes(2, 12, K))
    clean = run(jsg, torch_cuda, S, f)
    S[0, 3] = 0                                                 # silence between loud frames
    S[0, 5] = 0
    S[1, 4] = (np.minimum(S[1, 4], np.float32(2)) * np.float32(1e-40)).astype(np.float32)  # denormals only (and zeros)
    S[1, 6, :] = np.float32(1e-45)
    assert (S[1, 4] < np.float32(1.2e-38)).all() and (S[1, 4] > 0).any()
    got = run(jsg, torch_cuda, S, f, **layout(1))
    want = check(got, S, f, what=(K, "zero, denormal"))
    for name in ("energy", "centroid", "spread", "crest"):
        assert (got[name][0, [3, 5]] == 0).all() and not np.signbit(got[name][0, [3, 5]]).any()
    assert (got["rolloff_bin"][0, [3, 5]] == 0).all() and (got["energy"][1, [4, 6]] > 0).all() and (want["centroid"][1, 6] > 0)
    untouched = [t for t in range(12) if t not in (3, 5)]
    assert not sr.same_outputs({n: v[0, untouched] for n, v in got.items()}, {n: v[0, untouched] for n, v in clean.items()})
    for k0 in (0, K // 2, K - 1):
        N = np.array(S)
        N[1, 7, k0] = np.nan
        got = run(jsg, torch_cuda, N, f, **layout(k0))
        check(got, N, f, what=(K, "NaN", k0))
        for name in sr.FLOATS:
            nan = np.isnan(got[name])
            assert nan[1, 7] and nan.sum() == 1, (name, k0)             # exactly that frame
        assert got["rolloff_bin"][1, 7] == -1 and (np.delete(got["rolloff_bin"].ravel(), 12 + 7) >= 0).all()
    N = np.array(S)
    N[0, 2, K // 3] = np.inf
    got = run(jsg, torch_cuda, N, f)
    check(got, N, f, what=(K, "inf"))
    assert np.isposinf(got["energy"][0, 2]) and got["rolloff_bin"][0, 2] == K // 3


def test_python_layer(jsg, torch_cuda):
    torch = torch_cuda
    S = np.array(sr.planes(3, 10, 257)).reshape(3, 1, 10, 257)
    out = jsg.spectral_shape(S, sr=22050.0)
    assert set(out) == set(OUTPUTS) | {"flatness"}
    f = jsg.fft_frequencies(22050.0, 512)
    assert np.array_equal(f, sr.freqs(257, 22050.0 / 512)) and f.dtype == np.float32 and f.shape == (257,)
    want = sr.shape32(S, f)
    for name in OUTPUTS:
        assert isinstance(out[name], np.ndarray) and out[name].shape == (3, 1, 10), name
    assert not sr.same_outputs(out, want) and out["rolloff_bin"].dtype == np.int32
    assert np.allclose(out["flatness"], 10.0 ** (want["flatness_db"].astype(np.float64) / 10), rtol=1e-5, atol=0) and (out["flatness"] <= 1.0 + 1e-5).all()
    # CUDA in, CUDA out; a table of one's own
    d_S = torch.from_numpy(S).cuda()
    mel = np.linspace(100.0, 8000.0, 257).astype(np.float32)
    d_out = jsg.spectral_shape(d_S, freqs=mel, roll_percent=0.5)
    assert all(o.is_cuda and tuple(o.shape) == (3, 1, 10) for o in d_out.values())
    assert not sr.same_outputs({n: o.cpu().numpy() for n, o in d_out.items()}, sr.shape32(S, mel, 0.5))
    with pytest.raises(jsg.JsgError):
        jsg.spectral_shape(S)
    # each single-output convenience equals its entry
    assert sr.same_but_nan(jsg.spectral_centroid(S, sr=22050.0), out["centroid"])
    assert sr.same_but_nan(jsg.spectral_bandwidth(S, sr=22050.0), out["spread"])
    assert sr.same_but_nan(jsg.spectral_rolloff(S, sr=22050.0), out["rolloff"])
    assert sr.same_but_nan(jsg.spectral_rolloff(d_S, freqs=mel, roll_percent=0.5).cpu().numpy(), d_out["rolloff"].cpu().numpy())
    assert sr.same_but_nan(jsg.spectral_flatness(S), out["flatness"])
    assert sr.same_but_nan(jsg.spectral_crest(S), out["crest"])
    assert jsg.spectral_crest(d_S).is_cuda


def test_spectral_shape_audio_equals_the_explicit_chain(jsg, torch_cuda):
    torch = torch_cuda
    rng = np.random.default_rng(7)
    n, hop, rate = 1024, 256, 16000.0
    t = np.arange(n + 40 * hop) / rate
    x = (np.sin(2 * np.pi * 440.0 * t) + 0.1 * rng.standard_normal(t.size)).astype(np.float32)
    got = jsg.spectral_shape_audio(x, rate, n_fft=n, hop=hop, roll_percent=0.9)
    frames = 41
    d_x = torch.from_numpy(x).cuda()
    plan = jsg.Plan(n, jsg.window(jsg.capi.WIN_HANN, n))
    power = torch.empty((frames, n // 2 + 1), dtype=torch.float32, device="cuda")
    jsg.stft_db(plan, d_x[None, :], hop, frames, power, feedblocks=n // hop, linear_out=True)
    want = jsg.spectral_shape(power, sr=rate, roll_percent=0.9)
    assert set(got) == set(want) and all(isinstance(v, np.ndarray) and v.shape == (frames,) for v in got.values())
    assert not sr.same_outputs(got, {k: v.cpu().numpy() for k, v in want.items()}, tuple(OUTPUTS) + ("flatness",))
    # the chain is the restatement of the plane it made, and a 440 Hz tone sits where it should
    assert not sr.same_outputs(got, sr.shape32(power.cpu().numpy(), jsg.fft_frequencies(rate, n), 0.9))
    assert abs(np.median(got["centroid"]) - 440.0) < 200.0
    d_got = jsg.spectral_shape_audio(d_x, rate, n_fft=n, hop=hop, roll_percent=0.9)
    assert all(v.is_cuda for v in d_got.values()) and sr.same_but_nan(d_got["spread"].cpu().numpy(), got["spread"])
    with pytest.raises(jsg.JsgError):
        jsg.spectral_shape_audio(x, rate, n_fft=1024, hop=300)
