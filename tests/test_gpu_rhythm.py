"""Onset strength, autocorrelation tempogram and tempo on the GPU (include/jsg.h section 2j) against tests/rhythm_ref.py: graph capture
of a first launch, onset strength to the bit over band counts, lags and filter sizes, NaN containment, 65 535 rows; the tempogram under
both bounds in pitched buffers with sentinels over the window, lag, length and hop corners and where the plan changes its path,
identical bits over chunk lengths, pitches, offsets and row counts, silence, the NaN pattern; tempo to the bit from the GPU's own
tempogram, ties, NaN, frame counts around the blocks of the mean; and the Python layer down to estimate_tempo on a click track."""
import numpy as np
import pytest

import rhythm_ref as rr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
ISENTINEL = np.int32(-77777)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def same_but_nan(a, b):
    """same(), with a NaN of any sign and payload equal to any other NaN."""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and same(np.nan_to_num(a), np.nan_to_num(b))


def pitched_in(torch, x, pads, offset):
    """x numpy [..] -> a CUDA view of it whose axes lie pads[i] elements apart beyond their length (last axis: unit stride), starting
    `offset` floats into an allocation that holds NaN everywhere else."""
    shape = x.shape
    strides = [1]
    for n, pad in zip(reversed(shape[1:]), reversed(pads)):
        strides.append(strides[-1] * n + pad)
    strides = tuple(reversed(strides))
    size = offset + sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    flat = torch.full((size,), float("nan"), dtype=torch.float32, device="cuda")
    view = torch.as_strided(flat, shape, strides, storage_offset=offset)
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def pitched_out(torch, shape, pads, offset, dtype=None, sentinel=SENTINEL):
    """(allocation filled with the sentinel, view of `shape` into it, flat indices of the view's elements)."""
    strides = [1]
    for n, pad in zip(reversed(shape[1:]), reversed(pads)):
        strides.append(strides[-1] * n + pad)
    strides = tuple(reversed(strides))
    size = offset + sum((n - 1) * s for n, s in zip(shape, strides)) + 1 + 3
    flat = torch.full((size,), sentinel.item(), dtype=dtype or torch.float32, device="cuda")
    at = offset + sum(np.arange(n).reshape([-1 if i == k else 1 for i in range(len(shape))]) * s for k, (n, s) in enumerate(zip(shape, strides)))
    return flat, torch.as_strided(flat, shape, strides, storage_offset=offset), at


def collect(flat, at, what, sentinel=SENTINEL):
    """The view's elements, after checking that every other element of the allocation still holds the sentinel."""
    got = flat.cpu().numpy()
    written = np.zeros(got.size, bool)
    written[at.ravel()] = True
    assert (got[~written] == sentinel).all(), what
    return got[at]


def run_onset(jsg, torch, S, lag, m, *, pad_frame=0, pad_row=0, pad_out=0, offset=0):
    S = S if S.ndim == 3 else S[None]
    d_in = pitched_in(torch, S, (pad_row, pad_frame), offset)
    flat, view, at = pitched_out(torch, S.shape[:2], (pad_out,), offset)
    jsg.onset_strength_launch(d_in, view, lag=lag, max_size=m)
    torch.cuda.synchronize()
    return collect(flat, at, "onset")


def run_tg(jsg, torch, o, w, lags, hop, n_frames, normalise, *, chunk_frames=0, pad_in=0, pad_frame=0, pad_row=0, offset=0):
    o = np.atleast_2d(o)
    d_in = pitched_in(torch, o, (pad_in,), offset)
    d_w = torch.from_numpy(np.array(w, np.float32)).cuda()
    flat, view, at = pitched_out(torch, (o.shape[0], n_frames, lags), (pad_row, pad_frame), offset)
    jsg.tempogram_launch(d_in, d_w, view, lags=lags, hop=hop, n_frames=n_frames, normalise=bool(normalise), chunk_frames=chunk_frames)
    torch.cuda.synchronize()
    return collect(flat, at, "tempogram")


def run_tempo(jsg, torch, tg, prior, rate, *, outputs="blp", pad_frame=0, pad_row=0, pad_profile=0, offset=0):
    tg = tg if tg.ndim == 3 else tg[None]
    R, N, lags = tg.shape
    d_in = pitched_in(torch, tg, (pad_row, pad_frame), offset)
    d_prior = torch.from_numpy(np.array(prior, np.float32)).cuda()
    b = pitched_out(torch, (R,), (), offset) if "b" in outputs else None
    l = pitched_out(torch, (R,), (), offset, dtype=torch.int32, sentinel=ISENTINEL) if "l" in outputs else None
    p = pitched_out(torch, (R, lags), (pad_profile,), offset) if "p" in outputs else None
    jsg.tempo_launch(d_in, d_prior, rate, d_bpm=b and b[1], d_lag=l and l[1], d_profile=p and p[1])
    torch.cuda.synchronize()
    out = {}
    if b:
        out["bpm"] = collect(b[0], b[2], "bpm")
    if l:
        out["lag"] = collect(l[0], l[2], "lag", ISENTINEL)
    if p:
        out["g"] = collect(p[0], p[2], "profile")
    return out


def check_tg(got, ref, what):
    """Cap (b) per element, bound (a) per row; prints the figures first.  Elements whose float64 reference is NaN must be NaN."""
    e_gpu, e_ref = rr.cap_units(got, ref), rr.cap_units(ref["tg32"], ref)
    differ = int((raw(got) != raw(ref["tg32"])).sum())
    print(f"{what}: error in units of cap (b), GPU {e_gpu.max():.3f}, restatement {e_ref.max():.3f}; {differ} of {got.size} differ in bits from the restatement")
    ok = np.isfinite(ref["tg64"])
    assert (np.abs(got.astype(np.float64) - ref["tg64"])[ok] <= ref["cap"][ok]).all(), (what, e_gpu)
    assert (e_gpu <= rr.YARDSTICKS * e_ref).all(), (what, e_gpu, e_ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref["tg32"])), what
    return differ


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The first launches of the three kernels in this process (this test comes first in the file and no other file launches them) sit
    inside a capture; replayed twice, equals eager."""
    torch = torch_cuda
    S = np.array(rr.planes()[:2, :, :100])
    T = S.shape[1]
    w = rr.hann(100)
    prior = jsg.tempo_prior(100, rr.FRAME_RATE)
    d_S, d_w, d_prior = torch.from_numpy(S).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(prior).cuda()
    d_o = torch.zeros((2, T), dtype=torch.float32, device="cuda")
    d_tg = torch.zeros((2, T, 100), dtype=torch.float32, device="cuda")
    d_bpm, d_lag = torch.zeros(2, dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        jsg.onset_strength_launch(d_S, d_o, stream=s.cuda_stream)
        jsg.tempogram_launch(d_o, d_w, d_tg, stream=s.cuda_stream)
        jsg.tempo_launch(d_tg, d_prior, rr.FRAME_RATE, d_bpm=d_bpm, d_lag=d_lag, stream=s.cuda_stream)
    assert jsg.tempogram_kernel_name(d_o, d_w, d_tg) == "tempogram_lags2"
    o = run_onset(jsg, torch, S, 1, 1)
    tg = run_tg(jsg, torch, o, w, 100, 1, T, 1)
    tp = run_tempo(jsg, torch, tg, prior, rr.FRAME_RATE, outputs="bl")
    for _ in range(2):
        for d in (d_o, d_tg, d_bpm, d_lag):
            d.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert same(d_o.cpu().numpy(), o) and same(d_tg.cpu().numpy(), tg)
        assert same(d_bpm.cpu().numpy(), tp["bpm"]) and np.array_equal(d_lag.cpu().numpy(), tp["lag"])
    assert same(o, rr.onset32(S))
    check_tg(tg, rr.tempogram(o, w, 100, 1, T, 1), "capture, Wn 100")


def test_first_tempogram_launch_of_a_path_with_more_than_48_kib_of_lds(jsg, torch_cuda):
    """The first launch of the eight-lags-per-lane path in this process (only the capture above precedes it, on another path) asks for
    more dynamic LDS than a kernel may have without saying so: the launch itself has to say it."""
    Wn, n_frames = 4096, 2
    rng = np.random.default_rng(Wn)
    o = (0.2 * np.abs(rng.standard_normal((1, Wn + 1)))).astype(np.float32)
    o[0, ::7] += 1.0
    w = rr.hann(Wn) + np.float32(0.01)
    d_o, d_w, d_out = torch_cuda.zeros((1, Wn + 1), device="cuda"), torch_cuda.zeros(Wn, device="cuda"), torch_cuda.zeros((1, n_frames, Wn), device="cuda")
    name, _, lds = jsg.tempogram_plan(d_o, d_w, d_out, lags=Wn, hop=1, n_frames=n_frames)
    assert name == "tempogram_lags8" and lds > 49152, (name, lds)
    shared = rr.sums(o, w, Wn, 1, n_frames)
    for normalise in (0, 1):
        got = run_tg(jsg, torch_cuda, o, w, Wn, 1, n_frames, normalise, pad_frame=1, offset=normalise)
        check_tg(got, rr.tempogram(o, w, Wn, 1, n_frames, normalise, shared=shared), f"Wn = lags = {Wn}, first on its path, normalise {normalise}")


# ---------------------------------------------------------------------------------------------------- onset strength
@pytest.mark.parametrize("B", [1, 63, 64, 65, 128, 200])
def test_onset_bits_equal_the_restatement(jsg, torch_cuda, B):
    S = np.array(rr.planes()[:, :, :B])
    assert S.shape[1] == 40
    for lag in (1, 2, 3, 40, 41):
        for m in (1, 3, 4):
            got = run_onset(jsg, torch_cuda, S, lag, m, pad_frame=(lag + m) % 3, pad_row=m % 2 * 5, pad_out=lag % 2, offset=m % 2)
            want = rr.onset32(S, lag, m)
            assert same(got, want), (B, lag, m, int((raw(got) != raw(want)).sum()))
            assert (got[:, :lag] == 0).all() and not np.signbit(got[:, :lag]).any()
            if lag < 40:
                assert (np.abs(got - rr.onset64(S, lag, m)) <= (B / 64 + 9) * rr.U * rr.onset64(S, lag, m)).all()


def test_onset_small_band_counts_pack_frames_into_a_wave(jsg, torch_cuda):
    for B in (2, 3, 4, 5, 8, 16, 17, 32, 33):
        S = np.array(rr.planes()[:2, :37, :B])
        for lag, m in ((1, 1), (2, 3)):
            assert same(run_onset(jsg, torch_cuda, S, lag, m, pad_frame=1), rr.onset32(S, lag, m)), (B, lag, m)


def test_onset_nan_is_contained(jsg, torch_cuda):
    clean = run_onset(jsg, torch_cuda, np.array(rr.planes()), 2, 3)
    for t0, b0 in ((0, 0), (17, 199), (38, 100), (39, 5)):
        S = np.array(rr.planes())
        S[1, t0, b0] = np.nan
        got = run_onset(jsg, torch_cuda, S, 2, 3)
        hit = np.zeros(40, bool)
        hit[[t for t in (t0, t0 + 2) if 2 <= t < 40]] = True
        assert np.isnan(got[1][hit]).all() and same(got[1][~hit], clean[1][~hit])
        assert same(got[0], clean[0]) and same(got[2], clean[2])
        assert same_but_nan(got, rr.onset32(S, 2, 3))


def test_onset_65535_rows(jsg, torch_cuda):
    base = np.array(rr.planes()[:3, :5, :3])
    three = run_onset(jsg, torch_cuda, base, 1, 2)
    assert same(three, rr.onset32(base, 1, 2))
    for r in range(3):
        assert same(run_onset(jsg, torch_cuda, base[r], 1, 2), three[r:r + 1])
    many = run_onset(jsg, torch_cuda, np.tile(base, (21845, 1, 1)), 1, 2, pad_row=1)
    assert many.shape == (65535, 5) and same(many, np.tile(three, (21845, 1)))


# ---------------------------------------------------------------------------------------------------- tempogram
def envelope(T, seed):
    """[2][T] float32: noise with pulses every 7 samples, and a signed row (the sums cancel)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((2, T), np.float32)
    x[0] = np.abs(rng.standard_normal(T)) * 0.2
    x[0, ::7] += 1.0
    x[1] = rng.standard_normal(T)
    return x


@pytest.mark.parametrize("T_kind", ["one", "half", "three"])
@pytest.mark.parametrize("Lg_kind", ["one", "half", "all"])
@pytest.mark.parametrize("Wn", [2, 8, 64, 65, 384, 4096])
def test_tempogram_geometries(jsg, torch_cuda, Wn, Lg_kind, T_kind):
    """Every window, lag count, length and hop corner, both normalise values.  Where a row holds many frames the first ones are taken (at
    most 2^22 steps of the restatement per case, one frame at least)."""
    Lg = {"one": 1, "half": max(1, Wn // 2), "all": Wn}[Lg_kind]
    T = {"one": 1, "half": max(1, Wn // 2 - 1), "three": 3 * Wn}[T_kind]
    o = envelope(T, Wn + T)
    w = rr.hann(Wn) + np.float32(0.01)          # no zero in the table
    for hop in sorted({1, 3, Wn}):
        n_frames = min(rr.frames(T, hop), max(1, (1 << 22) // (Wn * Lg)))
        both = {}
        shared = rr.sums(o, w, Lg, hop, n_frames)
        for normalise in (0, 1):
            ref = rr.tempogram(o, w, Lg, hop, n_frames, normalise, shared=shared)
            got = run_tg(jsg, torch_cuda, o, w, Lg, hop, n_frames, normalise, pad_in=hop % 3, pad_frame=Wn % 3, pad_row=1, offset=normalise)
            check_tg(got, ref, f"Wn {Wn}, lags {Lg}, T {T}, hop {hop}, normalise {normalise}, {n_frames} frames")
            both[normalise] = got
        live = both[0][..., 0] != 0
        assert (both[1][..., 0][live] == 1).all() and (both[1][~live] == 0).all()


@pytest.mark.parametrize("Lg", [64, 65, 128, 129, 256, 257, 300])
def test_tempogram_where_the_plan_changes_its_path(jsg, torch_cuda, Lg):
    """The lags around the lane blocks against hops below, at and above the window (above it the frames lie back to back in LDS)."""
    Wn = 300
    w = rr.hann(Wn)
    for hop in (1, 7, Wn, Wn + 5):
        n_frames = 6 if hop <= 7 else 3
        T = (n_frames - 1) * hop + 2
        o = envelope(T, Lg + hop)
        x, dw, out = torch_cuda.zeros((2, T), device="cuda"), torch_cuda.zeros(Wn, device="cuda"), torch_cuda.zeros((2, n_frames, Lg), device="cuda")
        name = jsg.tempogram_plan(x, dw, out, lags=Lg, hop=hop, n_frames=n_frames)[0]
        assert name == ("tempogram_lags1" if Lg <= 64 else "tempogram_lags2" if Lg <= 128 else "tempogram_lags4" if Lg <= 256 else "tempogram_lags8")
        for normalise in (0, 1):
            ref = rr.tempogram(o, w, Lg, hop, n_frames, normalise)
            got = run_tg(jsg, torch_cuda, o, w, Lg, hop, n_frames, normalise, pad_frame=1)
            check_tg(got, ref, f"Wn {Wn}, lags {Lg}, hop {hop}, normalise {normalise}, {name}")


def test_tempogram_out_of_row_samples_are_left_out(jsg, torch_cuda):
    """Window values that only ever meet samples outside the row are Inf and NaN: those y are +0, not products."""
    for Wn, T in ((8, 1), (8, 3), (65, 2), (384, 5)):
        o = envelope(T, Wn)
        j = np.arange(T)[:, None] - Wn // 2 + np.arange(Wn)[None, :]          # frame i, hop 1: sample i - Wn / 2 + j
        used = ((j >= 0) & (j < T)).any(axis=0)
        assert used.any() and not used.all()
        w = rr.hann(Wn) + np.float32(0.5)
        w[~used] = np.inf
        w[np.flatnonzero(~used)[0]] = np.nan
        for normalise in (0, 1):
            ref = rr.tempogram(o, w, Wn, 1, T, normalise)
            assert np.isfinite(ref["tg32"]).all() and (ref["tg32"][..., 0] != 0).all()
            got = run_tg(jsg, torch_cuda, o, w, Wn, 1, T, normalise, pad_in=2, offset=1)
            check_tg(got, ref, f"Inf and NaN in the window outside the row, Wn {Wn}, T {T}, normalise {normalise}")
            assert same(got, ref["tg32"])


_tight = {}


def tight(jsg, torch):
    """The GPU's tempograms (normalise 0 and 1) of the shared envelopes at Wn = lags = 64, hop 1, in tight buffers with the default chunk."""
    if not _tight:
        for normalise in (0, 1):
            _tight[normalise] = run_tg(jsg, torch, rr.envelopes(), rr.hann(64), 64, 1, 600, normalise)
    return _tight


def test_tempogram_shared_envelopes(jsg, torch_cuda):
    for normalise in (0, 1):
        ref = rr.tempogram(rr.envelopes(), rr.hann(64), 64, 1, 600, normalise)
        got = tight(jsg, torch_cuda)[normalise]
        check_tg(got, ref, f"shared envelopes, normalise {normalise}")
        assert (got[3] == 0).all() and not np.signbit(got[3]).any()           # silence: +0 everywhere


def test_tempogram_bits_do_not_depend_on_the_chunk_the_pitches_or_the_rows(jsg, torch_cuda):
    want = tight(jsg, torch_cuda)
    w = rr.hann(64)
    for chunk in (1, 2, 3, 17, 605, 65536):
        for normalise in (0, 1):
            got = run_tg(jsg, torch_cuda, rr.envelopes(), w, 64, 1, 600, normalise, chunk_frames=chunk, pad_in=chunk % 7, pad_frame=chunk % 5, pad_row=chunk % 3,
                         offset=chunk % 2)
            assert same(got, want[normalise]), (chunk, normalise)
    # fewer frames than the row holds: the first frames, the same bits; fewer lags: the first lags
    assert same(run_tg(jsg, torch_cuda, rr.envelopes(), w, 64, 1, 593, 1), want[1][:, :593])
    assert same(run_tg(jsg, torch_cuda, rr.envelopes(), w, 33, 1, 600, 0), want[0][:, :, :33])
    # a hop takes every hop-th frame
    assert same(run_tg(jsg, torch_cuda, rr.envelopes(), w, 64, 7, 86, 1, chunk_frames=5), want[1][:, ::7])
    # rows on their own, and many rows
    for r in (0, 2):
        assert same(run_tg(jsg, torch_cuda, rr.envelopes()[r], w, 64, 1, 600, 1), want[1][r:r + 1])
    base = np.array(rr.envelopes()[:3, :9])
    three = run_tg(jsg, torch_cuda, base, rr.hann(4), 3, 4, 3, 1)
    many = run_tg(jsg, torch_cuda, np.tile(base, (21845, 1)), rr.hann(4), 3, 4, 3, 1, pad_in=1)
    assert many.shape == (65535, 3, 3) and same(many, np.tile(three, (21845, 1, 1)))


def test_tempogram_many_items_in_one_launch(jsg, torch_cuda):
    """8 rows x 1500 frames at chunk_frames = 1: 12000 work items, several times the grid."""
    o = np.tile(envelope(1500, 3), (4, 1))
    w = rr.hann(8)
    props = torch_cuda.cuda.get_device_properties(0)
    assert 8 * 1500 >= 3 * 8 * props.multi_processor_count
    got = run_tg(jsg, torch_cuda, o, w, 8, 1, 1500, 1, chunk_frames=1)
    assert same(got, run_tg(jsg, torch_cuda, o, w, 8, 1, 1500, 1, pad_frame=2))
    check_tg(got, rr.tempogram(o, w, 8, 1, 1500, 1), "tiny frames, chunk 1")


def test_tempogram_nan_pattern(jsg, torch_cuda):
    w = rr.hann(64)
    clean = tight(jsg, torch_cuda)
    for m0 in (0, 299, 599):
        x = np.array(rr.envelopes())
        x[1, m0] = np.nan
        for normalise in (0, 1):
            ref = rr.tempogram(x, w, 64, 1, 600, normalise)
            got = run_tg(jsg, torch_cuda, x, w, 64, 1, 600, normalise)
            assert same_but_nan(got, ref["tg32"])
            frames = np.arange(600)
            j0 = m0 - (frames - 32)                      # where the sample lies in each frame's window
            hit = (j0 >= 0) & (j0 < 64)
            for r in (0, 2, 3, 4):
                assert same(got[r], clean[normalise][r])
            assert same(got[1][~hit], clean[normalise][1][~hit]) and np.isnan(got[1][hit][:, 0]).all()
            if normalise:
                assert np.isnan(got[1][hit]).all()
            else:
                reach = np.maximum(j0, 63 - j0)[hit]     # exactly the lags whose sum pairs the sample
                assert np.array_equal(np.isnan(got[1][hit]), np.arange(64)[None, :] <= reach[:, None])


# ---------------------------------------------------------------------------------------------------- tempo
@pytest.mark.parametrize("Wn,T,period,margin", rr.DECIDED)
def test_tempo_on_the_decided_cases(jsg, torch_cuda, Wn, T, period, margin):
    o = rr.impulse_train(T, period)
    w = rr.hann(Wn)
    tg = run_tg(jsg, torch_cuda, o, w, Wn, 1, T, 1)
    check_tg(tg, rr.tempogram(o, w, Wn, 1, T, 1), f"impulse train, Wn {Wn}, period {period}")
    prior = jsg.tempo_prior(Wn, rr.FRAME_RATE)
    got = run_tempo(jsg, torch_cuda, tg, prior, rr.FRAME_RATE, pad_frame=3, pad_profile=2, offset=1)
    lag, bpm, g = rr.tempo32(tg[0], prior)
    assert lag == period and got["lag"][0] == lag
    assert same(got["bpm"], np.float32([bpm])) and same(got["g"][0], g)
    assert rr.tempo64(tg[0], prior)[0] == period


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_tempo_frame_counts_ties_and_nan(jsg, torch_cuda, N):
    rng = np.random.default_rng(N)
    lags = 300
    tg = rng.random((4, N, lags), dtype=np.float32)
    tg[1] = 0.25
    tg[1, :, 0] = 9.0                       # lag 0 is never chosen
    tg[2, N // 2, 7] = np.nan               # a NaN at a lag >= 1
    tg[3, N - 1, 0] = np.nan                # a NaN at lag 0 only: the profile shows it, the tempo does not
    prior = np.ones(lags, np.float32)
    prior[0] = 0
    prior[1:5] = 0
    got = run_tempo(jsg, torch_cuda, tg, prior, 50.0, pad_frame=N % 3, pad_row=1, pad_profile=1)
    for r in range(4):
        lag, bpm, g = rr.tempo32(tg[r], prior, 50.0)
        assert got["lag"][r] == lag and same_but_nan(got["bpm"][r:r + 1], np.float32([bpm])) and same_but_nan(got["g"][r], g), (N, r)
    assert got["lag"][1] == 5 and got["bpm"][1] == np.float32(3000.0) / np.float32(5)           # the lowest lag on a tie
    assert got["lag"][2] == -1 and np.isnan(got["bpm"][2]) and np.isnan(got["g"][2][7]) and np.isnan(got["g"][2]).sum() == 1
    assert got["lag"][3] >= 5 and np.isnan(got["g"][3][0])
    for outputs in ("b", "l", "p", "bl", "lp"):
        part = run_tempo(jsg, torch_cuda, tg, prior, 50.0, outputs=outputs)
        assert sorted(part) == sorted({"b": "bpm", "l": "lag", "p": "g"}[k] for k in outputs)
        assert all(same_but_nan(part[k], got[k]) for k in part), outputs
    one = run_tempo(jsg, torch_cuda, tg[0], prior, 50.0)
    assert all(same(one[k], got[k][:1]) for k in one)


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_python_layer(jsg, torch_cuda):
    torch = torch_cuda
    S = np.array(rr.planes())
    o = jsg.onset_strength(S, lag=2, max_size=3)                    # numpy in, numpy out
    assert isinstance(o, np.ndarray) and same(o, rr.onset32(S, 2, 3))
    St = torch.from_numpy(S).cuda()
    ot = jsg.onset_strength(St[1])
    assert ot.is_cuda and ot.shape == (40,) and same(ot.cpu().numpy(), rr.onset32(S[1]))
    env = np.array(rr.envelopes())
    tg = jsg.tempogram(env, win_length=64)
    assert isinstance(tg, np.ndarray) and tg.shape == (5, 600, 64)
    w = jsg.window(jsg.capi.WIN_HANN, 64)
    assert same(tg, run_tg(jsg, torch, env, w, 64, 1, 600, 1))
    envt = torch.from_numpy(env).cuda()
    tgt = jsg.tempogram(envt.reshape(5, 1, 600)[:2], win_length=64, hop_length=7, lags=20, normalise=False)
    assert tgt.is_cuda and tgt.shape == (2, 1, 86, 20) and same(tgt.reshape(2, 86, 20).cpu().numpy(), run_tg(jsg, torch, env[:2], w, 20, 7, 86, 0))
    assert same(jsg.tempogram(env[0], win_length=64, window_table=rr.hann(64)), run_tg(jsg, torch, env[0], rr.hann(64), 64, 1, 600, 1)[0])
    bpm, lag = jsg.tempo(tg, rr.FRAME_RATE)
    assert bpm.dtype == np.float32 and lag.dtype == np.int32 and bpm.shape == lag.shape == (5,)
    prior = jsg.tempo_prior(64, rr.FRAME_RATE)
    for r in range(5):
        want = rr.tempo32(tg[r], prior)
        assert lag[r] == want[0] and same(bpm[r:r + 1], np.float32([want[1]]))
    assert lag[0] == 20
    bt, lt = jsg.tempo(torch.from_numpy(tg).cuda()[0], rr.FRAME_RATE)
    assert bt.is_cuda and bt.shape == () and int(lt) == 20
    # the tempogram plane on its way through db_from_power and colormap
    one = torch.from_numpy(tg[0]).cuda().abs().contiguous()
    db = torch.empty_like(one)
    jsg.spectrogram.db_from_power(one, db)
    img = torch.zeros((64, 600), dtype=torch.int32, device="cuda")
    jsg.colormap(db, torch.from_numpy(jsg.colormap_lut(256, 6)).cuda(), -60.0, 0.0, d_argb=img)
    torch.cuda.synchronize()
    assert len(np.unique(img.cpu().numpy())) > 8


def test_estimate_tempo_on_a_click_track(jsg, torch_cuda):
    """12 s at 22 050 Hz, a click every 20 hops of 512 samples: lag 20, 60 * (22050 / 512) / 20 = 129.2 bpm."""
    sr, n = 22050, 12 * 22050
    x = np.zeros(n, np.float32)
    burst = (np.hanning(256) * np.sin(2 * np.pi * 1000.0 * np.arange(256) / sr)).astype(np.float32)
    for at in range(0, n - 256, 10240):
        x[at:at + 256] += burst
    x += np.float32(1e-4) * np.random.default_rng(5).standard_normal(n).astype(np.float32)
    bpm, lag = jsg.estimate_tempo(x, sr)
    assert isinstance(bpm, float) and isinstance(lag, int)
    assert lag == 20 and bpm == float(np.float32(np.float32(60.0) * np.float32(sr / 512)) / np.float32(20))
    bt, lt = jsg.estimate_tempo(torch_cuda.from_numpy(x).cuda(), sr)
    assert bt.is_cuda and int(lt) == 20 and float(bt) == bpm
