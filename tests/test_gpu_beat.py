"""The beat tracker of libjsgx.so on the GPU (include/jsgx.h section 1) against tests/beat_ref.py, bit for bit: graph capture of a first
launch; beats, their number, the local and the cumulative score over beat_ref.FORM_PERIODS (every (G, F) of the kernel and both periods at
each of the nine boundaries between them, which tests/test_jsgx_forms_host.py holds complete) at the lengths around one step, with
smoothing and normalisation on and off, on zero, constant, random and impulse-train rows; rows longer than the ring of 4096 frames with
64, 32, 16, 8, 4, 2 lanes and one lane per frame; periods read from a device buffer (bad ones among them); pitched buffers with guard elements; a NaN row between good rows; max_beats below the length of the chain; and the Python
layer down to beat_track_audio on a click track."""
import numpy as np
import pytest

import beat_ref as br

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
ISENTINEL = np.int32(-77777)
KINDS = ("zero", "const", "random", "train")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def d_log(jsg, torch_cuda):
    return torch_cuda.from_numpy(jsg.beat_log_table()).cuda()


def raw(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def run(jsg, torch, d_log, o, *, period=None, periods=None, smooth=True, normalise=True, max_beats=None, pads=(0, 0, 0, 0), tightness=100.0):
    """One launch on rows o [R][T] in pitched buffers full of sentinels: (beats [R][max_beats], n_beats [R], s [R][T], C [R][T]) as numpy,
    after checking that nothing outside these was written.  pads: extra elements per row of in, beats, local_score, cum_score."""
    R, T = o.shape
    max_beats = T if max_beats is None else max_beats
    fin = torch.full((R * (T + pads[0]) + 5,), float("nan"), dtype=torch.float32, device="cuda")
    d_in = torch.as_strided(fin, (R, T), (T + pads[0], 1), storage_offset=3)
    d_in.copy_(torch.from_numpy(np.array(o)))
    fb = torch.full((R * (max_beats + pads[1]) + 4,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_beats = torch.as_strided(fb, (R, max_beats), (max_beats + pads[1], 1), storage_offset=2)
    fn = torch.full((R + 2,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    fs = torch.full((R * (T + pads[2]) + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
    fc = torch.full((R * (T + pads[3]) + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_s = torch.as_strided(fs, (R, T), (T + pads[2], 1), storage_offset=1)
    d_c = torch.as_strided(fc, (R, T), (T + pads[3], 1), storage_offset=2)
    d_period = None if periods is None else torch.tensor(list(periods), dtype=torch.int32, device="cuda")
    jsg.beat_launch(d_in, d_log, d_beats, fn[1:R + 1], d_period=d_period, period=period, tightness=tightness, smooth=smooth, normalise=normalise,
                    max_beats=max_beats, d_local_score=d_s, d_cum_score=d_c)
    torch.cuda.synchronize()
    out = []
    for flat, view, sentinel, offset in ((fb, d_beats, ISENTINEL, 2), (fs, d_s, SENTINEL, 1), (fc, d_c, SENTINEL, 2)):
        got = flat.cpu().numpy()
        inside = np.zeros(got.size, bool)
        inside[(offset + np.arange(R)[:, None] * view.stride(0) + np.arange(view.shape[1])[None, :]).ravel()] = True
        assert (got[~inside] == sentinel).all(), "a guard element was written"
        out.append(view.cpu().numpy())
    n = fn.cpu().numpy()
    assert n[0] == ISENTINEL and n[-1] == ISENTINEL
    return out[0], n[1:R + 1], out[1], out[2]


def check_rows(got, want, what, max_beats=None):
    """got: what run() returns; want: one beat_ref dict per row."""
    beats, n, s, C = got
    for r, w in enumerate(want):
        assert n[r] == w["n"], (what, r, n[r], w["n"])
        if w["n"] < 0:      # a refused row: nothing but n_beats is written
            assert (beats[r] == ISENTINEL).all() and (s[r] == SENTINEL).all() and (C[r] == SENTINEL).all(), (what, r)
            continue
        kept = w["n"] if max_beats is None else min(w["n"], max_beats)
        assert (beats[r, :kept] == w["beats"][:kept]).all() and (beats[r, kept:] == ISENTINEL).all(), (what, r)
        assert same(s[r], w["s"]), (what, r, "local score")
        assert same(C[r], w["C"]), (what, r, "cumulative score")


def test_captured_first_launch_replays(jsg, torch_cuda, d_log):
    """The launch allocates nothing and synchronises nothing: captured (the first launch of the kernel in a fresh process), replayed once."""
    torch = torch_cuda
    P, T = 33, 500
    o = np.stack([br.envelope("train", T, P), br.envelope("random", T, P)])
    d_in = torch.from_numpy(o).cuda()
    d_beats = torch.full((2, T), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_n = torch.full((2,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_scratch = torch.empty((jsg.beat_scratch_bytes(d_in, d_log, d_beats, d_n, period=P) // 4,), dtype=torch.int32, device="cuda")
    assert d_scratch.numel() == 2 * 2 * T
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.beat_launch(d_in, d_log, d_beats, d_n, period=P, d_scratch=d_scratch, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert (d_n.cpu().numpy() == ISENTINEL).all()      # captured, not run
    g.replay()
    torch.cuda.synchronize()
    want = br.beat32_rows(o, P)
    n, beats = d_n.cpu().numpy(), d_beats.cpu().numpy()
    for r in range(2):
        assert n[r] == want[r]["n"] and (beats[r, :n[r]] == want[r]["beats"]).all() and (beats[r, n[r]:] == ISENTINEL).all()


@pytest.mark.parametrize("P", br.FORM_PERIODS)
def test_periods_and_lengths_to_the_bit(jsg, torch_cuda, d_log, P):
    """Four rows (zero, constant, random, impulse train) per launch; the lengths around a = (P + 1) // 2 (one step of the recurrence), 2P and
    5P + 3 (the ring of 4096 frames wraps for P = 1024 only; the look-back leaves the row at the start); P = 1, 2: one frame per step; 3..6:
    two and three; 7..14: four frames of 64 lanes; then 32, 16, 8, 4 and 2 lanes per frame, each from its first period (15, 31, 63, 127,
    255) to its last; 511 and 1024: one lane per frame, 256 frames per step, at 1024 two tiles of smoothing staged with the widest halo."""
    a = (P + 1) // 2
    lengths = sorted({1, max(1, a - 1), a, a + 1, 2 * P, 2 * P + 1, 5 * P + 3} | ({3000} if P == 33 else set()))
    assert jsg.beat_plan(P)[0] == ("beat_frames" if P >= 511 else "beat_split")
    assert br.form(P)[1] * br.form(P)[2] <= 256 and (br.form(P)[1] == 4) == (127 <= P <= 254)
    for T in lengths:
        o = np.stack([br.envelope(kind, T, P) for kind in KINDS])
        for smooth in (False, True):
            for normalise in (False, True):
                want = br.beat32_rows(o, P, smooth=smooth, normalise=normalise)
                got = run(jsg, torch_cuda, d_log, o, period=P, smooth=smooth, normalise=normalise)
                check_rows(got, want, (P, T, smooth, normalise))


@pytest.mark.parametrize("P", [5, 6, 20, 47, 100, 200, 255])
def test_long_rows(jsg, torch_cuda, d_log, P):
    """Rows longer than the ring of 4096 frames, so that it wraps, in every split of a frame over lanes (one lane per frame wraps at P = 1024
    above): three frames per step (P = 5, 6: a step count that is no power of two) over 4500 frames, the benchmark's period 47 over 9000
    frames with chains of more than 150 beats, whole and cut at max_beats, and 32, 8, 4 and 2 lanes per frame (P = 20, 100, 200, 255) over
    4500 frames; at P = 200 the backtrace walks 15 links or more."""
    T = 9000 if P == 47 else 4500
    assert br.form(P)[1:] == {5: (64, 3), 6: (64, 3), 20: (32, 8), 47: (16, 16), 100: (8, 32), 200: (4, 64), 255: (2, 128)}[P]
    o = np.stack([br.envelope(kind, T, P) for kind in KINDS])
    for smooth in (False, True):
        want = br.beat32_rows(o, P, smooth=smooth)
        assert P != 47 or min(w["n"] for w in want) > 150
        assert P != 200 or min(w["n"] for w in want) >= 15
        check_rows(run(jsg, torch_cuda, d_log, o, period=P, smooth=smooth), want, (P, smooth))
        if P == 47:
            check_rows(run(jsg, torch_cuda, d_log, o, period=P, smooth=smooth, max_beats=100), want, (P, smooth, 100), max_beats=100)


def test_periods_from_a_device_buffer(jsg, torch_cuda, d_log):
    """Nine rows, nine periods in device memory as tempo_launch leaves them, -1 (its NaN row) and 1025 among them, each good one in another
    form of the kernel (190: four lanes per frame); every buffer pitched."""
    periods = (7, -1, 100, 1025, 1, 257, 33, 600, 190)
    T = 1300
    assert sorted(br.form(P)[1] for P in periods if 1 <= P <= 1024) == [1, 2, 4, 8, 16, 64, 64]
    o = np.stack([br.envelope(KINDS[2 + r % 2], T, 40 + r) for r in range(9)])
    want = [br.beat32(o[r], P) for r, P in enumerate(periods)]
    assert [w["n"] < 0 for w in want] == [False, True, False, True, False, False, False, False, False]
    got = run(jsg, torch_cuda, d_log, o, periods=periods, pads=(5, 3, 7, 1))
    check_rows(got, want, "device periods")
    # ... and a row does not depend on its neighbours, on the pitches or on the number of rows
    alone = run(jsg, torch_cuda, d_log, o[5:6], periods=periods[5:6])
    check_rows(alone, want[5:6], "one row")
    # 0 and the largest period
    got = run(jsg, torch_cuda, d_log, o[:2], periods=(0, 1024))
    check_rows(got, [{"n": -1}, br.beat32(o[1], 1024)], "period 0 and 1024")


def test_nan_row_between_good_rows(jsg, torch_cuda, d_log):
    P, T = 16, 777
    o = np.stack([br.envelope("random", T, P), br.envelope("random", T, P + 1), br.envelope("train", T, P)]).copy()
    o[1, 700] = np.nan
    want = [br.beat32(row, P) for row in o]
    assert want[1]["n"] == -1 and want[0]["n"] > 10
    check_rows(run(jsg, torch_cuda, d_log, o, period=P, pads=(1, 2, 3, 4)), want, "NaN row")
    # ... also where the NaN is the very first or the very last frame, and without normalisation or smoothing
    for at in (0, T - 1):
        o[1] = br.envelope("random", T, P + 1)
        o[1, at] = np.nan
        check_rows(run(jsg, torch_cuda, d_log, o, period=P, smooth=False, normalise=False), [br.beat32(row, P, smooth=False, normalise=False) for row in o], at)


def test_max_beats_below_the_chain(jsg, torch_cuda, d_log):
    """The earliest beats are the ones kept, n_beats is the whole length, nothing behind max_beats is written."""
    P, T = 7, 400
    o = np.stack([br.envelope("train", T, P), br.envelope("zero", T, P)])
    want = br.beat32_rows(o, P)
    assert want[0]["n"] > 50
    for max_beats in (1, 5, want[0]["n"] - 1, want[0]["n"]):
        check_rows(run(jsg, torch_cuda, d_log, o, period=P, max_beats=max_beats, pads=(0, 2, 0, 0)), want, max_beats, max_beats=max_beats)


def test_tightness(jsg, torch_cuda, d_log):
    P, T = 33, 600
    o = np.stack([br.envelope("random", T, P)])
    for tightness in (1.0, 400.0):
        check_rows(run(jsg, torch_cuda, d_log, o, period=P, tightness=tightness), br.beat32_rows(o, P, tightness=tightness), tightness)


def test_beat_track(jsg, torch_cuda):
    """The Python layer: an int period, bpm and frame rate, a device tensor of periods; batch axes; numpy input."""
    torch = torch_cuda
    T = 640
    o = np.stack([br.envelope("train", T, 20), br.envelope("random", T, 20)]).reshape(2, 1, T)
    want = br.beat32_rows(o.reshape(2, T), 20)
    for kw in (dict(period=20), dict(bpm=120.0, frame_rate=40.0), dict(period=torch.tensor([20, 20], dtype=torch.int32, device="cuda"))):
        beats, n = jsg.beat_track(torch.from_numpy(o).cuda(), **kw)
        assert beats.is_cuda and beats.dtype == torch.int32 and n.shape == (2, 1) and beats.shape[:2] == (2, 1)
        beats, n = beats.cpu().numpy(), n.cpu().numpy()
        for r in range(2):
            assert n[r, 0] == want[r]["n"] and (beats[r, 0, :n[r, 0]] == want[r]["beats"]).all()
    assert (want[0]["beats"] == np.arange(6, T, 20)).all()
    beats, n = jsg.beat_track(o[0, 0], period=20, max_beats=4)
    assert (beats.cpu().numpy() == want[0]["beats"][:4]).all() and int(n.cpu()) == want[0]["n"]


def test_beat_track_audio_on_a_click_track(jsg, torch_cuda):
    """Four seconds of clicks at 120 bpm: the whole chain from audio to beats is enqueued without a host copy or synchronisation (after the
    first call of the geometry has uploaded its tables), and its beats are those of the restatement fed with the GPU's own envelope and lag."""
    torch = torch_cuda
    sr, hop = 22050, 512
    x = np.zeros(4 * sr, np.float32)
    for k in range(8):
        at = int(round((0.25 + 0.5 * k) * sr))
        x[at:at + 64] = np.hanning(64).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    jsg.beat_track_audio(d_x, sr)       # plans and tables
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bpm, beats, n = jsg.beat_track_audio(d_x, sr)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    env = jsg.onset_strength(jsg.mel_spectrogram_db(d_x, sr, 2048, hop, 128))
    _, lag = jsg.tempo(jsg.tempogram(env), sr / hop)
    lag, env = int(lag.cpu()), env.cpu().numpy()
    assert abs(float(bpm.cpu()) - 120.0) < 6.0 and abs(60.0 * (sr / hop) / lag - 120.0) < 6.0
    want = br.beat32(env, lag)
    n, beats = int(n.cpu()), beats.cpu().numpy()
    assert n == want["n"] and (beats[:n] == want["beats"]).all() and (beats[n:] == 0).all()
    assert n >= 7 and (np.abs(np.diff(beats[:n]) - lag) <= 2).all()
