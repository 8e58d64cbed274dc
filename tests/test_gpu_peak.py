"""Peak picking and onset backtracking of libjsgx.so on the GPU (include/jsgx.h section 14) against tests/peak_ref.py, exactly: the
counts, the peak frames, the backtracked frames and the candidate bytes are integers.  Every buffer is pitched and full of sentinels that
must come back untouched: the padding of every output, the entries behind a row's list, the inputs, the scratch's guard.  First the graph
capture of a first launch of each form; then the frame and row counts at which a block edge, the form change or the dealing of short
rows can go wrong; the reaches (the largest, one longer than the row, a halo that covers a whole short block and the row's end); the
waits (the off-by-one on the impulse train, waits around one and two blocks, the longest); a chain that leaves a block exactly onto the
next block's first candidate, and one frame off; the inputs; the thresholds; the list cut by max_peaks; backtracking through blocks
without a minimum; the containment of a NaN and an infinity; and the Python layer up to a click track behind the mel spectrogram."""
import functools

import numpy as np
import pytest

import peak_ref as pr

pytestmark = pytest.mark.gpu

B = pr.BLOCK
DEFAULT = pr.DEFAULT
INT_SENTINEL, BYTE_SENTINEL = -77, 7


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


class Guarded:
    """A flat buffer full of `sentinel` and the view [rows][cols] inside it with `pad` extra elements per row."""

    def __init__(self, torch, rows, cols, pad, sentinel, offset, dtype):
        self.flat = torch.full((rows * (cols + pad) + offset + 5,), sentinel, dtype=dtype, device="cuda")
        self.view = torch.as_strided(self.flat, (rows, cols), (cols + pad, 1), storage_offset=offset)
        self.sentinel, self.offset = sentinel, offset

    def outside(self):
        """The elements that are not the view's."""
        got = self.flat.cpu().numpy()
        inside = np.zeros(got.size, bool)
        R, W = self.view.shape
        inside[(self.offset + np.arange(R)[:, None] * self.view.stride(0) + np.arange(W)[None, :]).ravel()] = True
        return got[~inside]

    def untouched(self):
        out = self.outside()
        return bool(np.isnan(out).all() if self.sentinel != self.sentinel else (out == self.sentinel).all())


def run(jsg, torch, X, *, energy=None, want=("candidate",), max_peaks=None, pad=3, extra_scratch=0, **params):
    """One launch over X float32 [rows][T] (energy: None, "in" for the envelope itself, or another plane) -> per row (n, peaks, backtracked
    or None, candidates or None) as Python lists / numpy, after checking that nothing else was written."""
    params = dict(DEFAULT, **params)
    X = np.array(X, np.float32)
    R, T = X.shape
    most = T if max_peaks is None else max_peaks
    d_in = Guarded(torch, R, T, pad, float("nan"), 3, torch.float32)
    d_in.view.copy_(torch.from_numpy(X))
    d_energy = None
    if energy is not None and not isinstance(energy, str):
        d_energy = Guarded(torch, R, T, pad + 1, float("nan"), 1, torch.float32)
        d_energy.view.copy_(torch.from_numpy(np.asarray(energy, np.float32)))
    e_view = d_in.view if isinstance(energy, str) else None if d_energy is None else d_energy.view
    d_peaks, d_back = Guarded(torch, R, most, 2, INT_SENTINEL, 2, torch.int32), Guarded(torch, R, most, 2, INT_SENTINEL, 1, torch.int32)          # one pitch
    p_view, b_view = d_peaks.view, d_back.view
    d_n = torch.full((R + 4,), INT_SENTINEL, dtype=torch.int32, device="cuda")
    d_cand = Guarded(torch, R, T, pad + 2, BYTE_SENTINEL, 5, torch.uint8) if "candidate" in want else None
    before = [g.flat.clone() for g in (d_in, d_energy) if g is not None]
    kw = dict(params, d_energy=e_view, d_backtracked=b_view if energy is not None else None, d_candidate=None if d_cand is None else d_cand.view)
    need = jsg.peak_scratch_bytes(d_in.view, p_view, d_n[2:2 + R], **kw)
    nb = -(-T // B)
    assert need == (0 if nb == 1 else R * nb * (32 + 4 * min(params["wait"] + 1, B) + B))
    assert jsg.peak_plan(T, R, params["wait"]) == ("peak_single" if nb == 1 else "peak_blocked", 256, jsg.capix.PEAK_LDS_BYTES, 1 if nb == 1 else 5, nb)
    d_scratch = torch.full((need + extra_scratch + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    jsg.peak_launch(d_in.view, p_view, d_n[2:2 + R], d_scratch=d_scratch[:need + extra_scratch], **kw)
    torch.cuda.synchronize()
    assert d_peaks.untouched() and d_back.untouched() and (d_cand is None or d_cand.untouched()), "a guard element was written"
    for g, was in zip([g for g in (d_in, d_energy) if g is not None], before):
        assert torch.equal(g.flat.view(torch.int32), was.view(torch.int32)), "an input was written"
    assert (d_scratch[need + extra_scratch:].cpu().numpy() == 0x5A).all(), "the scratch's guard was written"
    n_all = d_n.cpu().numpy()
    assert (n_all[:2] == INT_SENTINEL).all() and (n_all[2 + R:] == INT_SENTINEL).all()
    peaks, backs = p_view.cpu().numpy(), b_view.cpu().numpy()
    cand = None if d_cand is None else d_cand.view.cpu().numpy()
    out = []
    for r in range(R):
        n = int(n_all[2 + r])
        kept = max(0, min(n, most))
        assert (peaks[r, kept:] == INT_SENTINEL).all(), "an entry behind the list was written"
        assert (backs[r, kept if energy is not None else 0:] == INT_SENTINEL).all(), "a backtracked entry behind the list was written"
        if n < 0 and cand is not None:
            assert (cand[r] == BYTE_SENTINEL).all(), "a refused row's candidates were written"
        out.append((n, peaks[r, :kept].tolist(), backs[r, :kept].tolist() if energy is not None else None, None if cand is None or n < 0 else cand[r]))
    return out


def expected(X, *, energy=None, max_peaks=None, **params):
    params = dict(DEFAULT, **params)
    X = np.asarray(X, np.float32)
    E = X if isinstance(energy, str) else energy
    return [pr.peak_pick32(X[r], energy=None if E is None else np.asarray(E, np.float32)[r], max_peaks=max_peaks, **params) for r in range(X.shape[0])]


def check(got, want, what):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (what, r, "n_peaks", g[0], w[0])
        if w[0] < 0:
            continue
        assert g[1] == w[1], (what, r, "peaks", [(i, a, b) for i, (a, b) in enumerate(zip(g[1], w[1])) if a != b][:4])
        assert g[2] == w[2], (what, r, "backtracked")
        if g[3] is not None:
            assert (g[3] == w[3]).all(), (what, r, "candidates", np.flatnonzero(g[3] != w[3])[:4])


def both(jsg, torch, X, what, **kw):
    got = run(jsg, torch, X, **kw)
    kw.pop("want", None), kw.pop("pad", None), kw.pop("extra_scratch", None)
    want = expected(X, **kw)
    check(got, want, what)
    return got


@functools.lru_cache(maxsize=None)
def noise(R, T, seed=0):
    X = pr.quantised(T, seed, R)
    X.setflags(write=False)
    return X


def test_the_sets_are_covered():
    assert {s[0] for s in pr.SHAPES} == set(pr.ROWS_SET) and {s[1] for s in pr.SHAPES} == set(pr.T_SET)
    assert {1, 2, 3, 63, 64, 65, 256, 257, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B + 7} == set(pr.T_SET)
    for corner in ((1, 1), (3, 1), (1, 3 * B + 7), (3, 3 * B + 7)):
        assert corner in pr.SHAPES


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The kernels of each form (a wavefront a row, a workgroup a row, the five of "peak_blocked") are launched here for the first time in
    the process, under capture, on one stream: the graph is a chain."""
    torch = torch_cuda
    for R, T in ((5, 37), (2, 300), (2, 2 * B + 1)):
        X = noise(R, T, 3)
        want = expected(X, energy="in")
        d_in = torch.zeros((R, T), dtype=torch.float32, device="cuda")
        d_peaks, d_back = torch.full((R, T), INT_SENTINEL, dtype=torch.int32, device="cuda"), torch.full((R, T), INT_SENTINEL, dtype=torch.int32, device="cuda")
        d_n = torch.full((R,), INT_SENTINEL, dtype=torch.int32, device="cuda")
        d_cand = torch.full((R, T), BYTE_SENTINEL, dtype=torch.uint8, device="cuda")
        kw = dict(DEFAULT, d_energy=d_in, d_backtracked=d_back, d_candidate=d_cand)
        d_scratch = torch.empty(max(4, jsg.peak_scratch_bytes(d_in, d_peaks, d_n, **kw)), dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                jsg.peak_launch(d_in, d_peaks, d_n, d_scratch=d_scratch, stream=side.cuda_stream, **kw)
        torch.cuda.synchronize()
        assert (d_n.cpu().numpy() == INT_SENTINEL).all() and (d_cand.cpu().numpy() == BYTE_SENTINEL).all()          # captured, not run
        d_in.copy_(torch.from_numpy(np.array(X)))
        g.replay()
        torch.cuda.synchronize()
        n, peaks, back, cand = d_n.cpu().numpy(), d_peaks.cpu().numpy(), d_back.cpu().numpy(), d_cand.cpu().numpy()
        check([(int(n[r]), peaks[r, :n[r]].tolist(), back[r, :n[r]].tolist(), cand[r]) for r in range(R)], want, ("replayed", T))


@pytest.mark.parametrize("R, T", pr.SHAPES)
def test_shapes(jsg, torch_cuda, R, T):
    got = both(jsg, torch_cuda, noise(R, T), (R, T), energy="in")
    if T >= 63:
        assert all(0 < g[0] < T for g in got)          # neither list is empty or full


def test_many_short_rows(jsg, torch_cuda):
    """300 rows of 37 frames: a wavefront a row, four rows a workgroup, the last workgroup not full."""
    R, T = pr.MANY_SHORT
    got = both(jsg, torch_cuda, noise(R, T, 5), "short rows", energy="in")
    assert len({tuple(g[1]) for g in got}) > 250          # the rows are not each other's
    both(jsg, torch_cuda, noise(301, 64, 6), "301 rows of 64 frames")
    both(jsg, torch_cuda, noise(7, 65, 6), "rows of 65 frames")


@pytest.mark.parametrize("reaches", pr.REACHES, ids=[str(r) for r in pr.REACHES])
def test_reaches(jsg, torch_cuda, reaches):
    kw = dict(zip(("pre_max", "post_max", "pre_avg", "post_avg"), reaches))
    both(jsg, torch_cuda, noise(3, 3 * B + 7, 1), reaches, **kw)
    # a reach longer than the row; a halo that covers the whole last block and the row's end, on both sides of the edge in front of it
    both(jsg, torch_cuda, noise(3, 100, 1), (reaches, "short"), **kw)
    both(jsg, torch_cuda, noise(1, 2 * B + 1, 2), (reaches, "2B+1"), **kw)
    both(jsg, torch_cuda, pr.smooth(2 * B + 200, 2, 2), (reaches, "smooth"), delta=0.0, **kw)


@pytest.mark.parametrize("wait", [0, 1, 2, 5, 6])
def test_waits_on_the_impulse_train(jsg, torch_cuda, wait):
    for T in (64, 301, 3 * B + 7):
        X = np.stack([pr.impulses(T), pr.impulses(T)])
        got = both(jsg, torch_cuda, X, (wait, T), pre_max=1, post_max=1, pre_avg=2, post_avg=2, delta=0.07, wait=wait)
        assert got[0][1] == list(range(0, T, 6 * -(-(wait + 1) // 6)))


@pytest.mark.parametrize("wait", [B - 1, B, B + 1, 2 * B + 3, 3 * B + 7, pr.MAX_FRAMES])
def test_long_waits(jsg, torch_cuda, wait):
    T = 3 * B + 7
    both(jsg, torch_cuda, noise(3, T, 7), wait, wait=wait, energy="in")
    got = both(jsg, torch_cuda, np.zeros((1, T), np.float32), (wait, "zeros"), wait=wait, delta=0.0)
    assert got[0][1] == list(range(0, T, wait + 1)) and got[0][3].all()


@pytest.mark.parametrize("first, second, wait, kept", [(B - 1, B + 4, 4, 2), (B - 1, B + 4, 5, 1), (B - 2, B + 3, 4, 2), (B, B + 5, 4, 2), (B - 1, B, 0, 2),
                                                       (B - 1, 2 * B, B, 2), (B - 1, 2 * B, B + 1, 1), (B - 1, 2 * B + 1, B + 1, 2)])
def test_a_chain_across_a_block_edge(jsg, torch_cuda, first, second, wait, kept):
    """A candidate on a block's last frame whose wait ends exactly on the next block's first candidate, then the same one frame off."""
    X = np.zeros((1, 3 * B), np.float32)
    X[0, [first, second]] = 1
    got = both(jsg, torch_cuda, X, (first, second, wait), pre_max=1, post_max=1, pre_avg=2, post_avg=2, delta=0.07, wait=wait, energy="in")
    assert list(np.flatnonzero(got[0][3])) == [first, second] and got[0][1] == [first, second][:kept]


def special_rows(T):
    ramp = np.arange(T, dtype=np.float32)
    lone = lambda t: np.eye(1, T, t, dtype=np.float32)[0]
    rows = [np.zeros(T, np.float32), np.full(T, 2.5, np.float32), ramp, ramp[::-1].copy(), lone(0), lone(T - 1)]
    rows += [lone(t) for t in (B - 1, B) if t < T]
    return np.stack(rows)


@pytest.mark.parametrize("T", [300, 2 * B + 5])
@pytest.mark.parametrize("normalise", [False, True])
def test_inputs(jsg, torch_cuda, T, normalise):
    for delta in pr.DELTAS:
        both(jsg, torch_cuda, special_rows(T), (T, normalise, delta), normalise=normalise, delta=delta, energy="in")
    both(jsg, torch_cuda, pr.smooth(T, 3, 3), (T, normalise, "smooth"), normalise=normalise, energy="in")
    both(jsg, torch_cuda, noise(3, T, 9) * np.float32(0.37) - np.float32(5), (T, normalise, "scaled"), normalise=normalise, delta=0.07)


def test_one_frame(jsg, torch_cuda):
    for v in (0.0, 1.0, 3.0e7):
        for delta in (-0.1, 0.0, 0.07, 1.0):
            for normalise in (False, True):
                got = both(jsg, torch_cuda, np.full((3, 1), v, np.float32), (v, delta), delta=delta, normalise=normalise, energy="in")
                assert got[1][0] == int(0 >= delta if normalise else np.float32(v) >= np.float32(np.float32(v) + np.float32(delta)))


@pytest.mark.parametrize("T", [200, 3 * B + 7])
def test_max_peaks_cuts_the_list(jsg, torch_cuda, T):
    X = noise(3, T, 4)
    whole = both(jsg, torch_cuda, X, "whole", energy="in")
    for most in (1, 5, 17) + ((B // 4,) if T > B else ()):          # the last one cuts behind the first block
        cut = both(jsg, torch_cuda, X, ("cut", most), energy="in", max_peaks=most)
        for c, w in zip(cut, whole):
            assert c[0] == w[0] > most and c[1] == w[1][:most] and c[2] == w[2][:most]


def test_backtracking(jsg, torch_cuda):
    T = 3 * B + 7
    X = noise(3, T, 8)
    other = pr.smooth(T, 9, 3)
    both(jsg, torch_cuda, X, "another plane", energy=other)
    # minima in the first block alone: the carry reaches back two blocks, and every peak behind the last minimum shares it
    rising = np.tile(np.arange(T, dtype=np.float32), (3, 1))
    rising[1, :40] = pr.quantised(40, 1)[0]
    got = both(jsg, torch_cuda, X, "rising energy", energy=rising)
    assert set(got[0][2]) == {0} and len(set(got[1][2])) > 1 and got[1][2][-1] == got[1][2][-2] < 40 and got[1][1][-1] > 2 * B
    # every optional output absent and present in turn
    want = expected(X, energy=other)
    for energy, wanted in ((None, ()), (None, ("candidate",)), (other, ()), (other, ("candidate",))):
        got = run(jsg, torch_cuda, X, energy=energy, want=wanted)
        for g, w in zip(got, want):
            assert g[0] == w[0] and g[1] == w[1] and (energy is None or g[2] == w[2]) and (g[3] is None or (g[3] == w[3]).all())
    both(jsg, torch_cuda, noise(3, 300, 8), "one block", energy=pr.smooth(300, 2, 3), want=())


@pytest.mark.parametrize("T", [40, 300, 2 * B + 5])
def test_containment(jsg, torch_cuda, T):
    """A row with a NaN, a row with an infinity and a row with a NaN in its energy alone, each between two clean rows: -1 for it, nothing
    else written for it, and the neighbours as in their lone runs."""
    clean = noise(7, T, 11)
    X, E = np.array(clean), np.array(pr.smooth(T, 12, 7))
    X[1, T // 3] = np.nan
    X[3, T - 1] = -np.inf
    E[5, 0] = np.nan
    got = run(jsg, torch_cuda, X, energy=E)
    assert [g[0] < 0 for g in got] == [False, True, False, True, False, True, False] and [got[r][0] for r in (1, 3, 5)] == [-1, -1, -1]
    for r in (0, 2, 4, 6):
        lone = run(jsg, torch_cuda, X[r:r + 1], energy=E[r:r + 1])[0]
        assert got[r][:3] == lone[:3] and (got[r][3] == lone[3]).all()
    check(got, expected(X, energy=E), "against the restatement")
    got = run(jsg, torch_cuda, X)          # without energy its NaN is not looked at
    assert [g[0] < 0 for g in got] == [False, True, False, True, False, False, False]


def test_two_scratch_sizes(jsg, torch_cuda):
    X = noise(3, 2 * B + 1, 13)
    first = both(jsg, torch_cuda, X, "exact", energy="in")
    second = run(jsg, torch_cuda, X, energy="in", extra_scratch=12345)
    check(second, expected(X, energy="in"), "larger")
    assert [g[:3] for g in first] == [g[:3] for g in second]


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_peak_pick_and_onset_detect(jsg, torch_cuda):
    torch = torch_cuda
    X = noise(3, 2 * B + 5, 14)
    d = torch.from_numpy(np.array(X)).cuda()
    want = expected(X, **dict(DEFAULT, normalise=False))
    got = jsg.peak_pick(d, 3, 1, 5, 5, 0.07, 3)
    assert [g.cpu().tolist() for g in got] == [w[1] for w in want] and got[0].dtype == torch.int32
    assert jsg.peak_pick(d[1], 3, 1, 5, 5, 0.07, 3).cpu().tolist() == want[1][1]
    assert jsg.peak_pick(X[1], 3, 1, 5, 5, 0.07, 3, max_peaks=4).cpu().tolist() == want[1][1][:4]
    bad = d.clone()
    bad[1, 5] = float("nan")
    got = jsg.peak_pick(bad, 3, 1, 5, 5, 0.07, 3, normalise=True)
    assert got[1] is None and got[0].cpu().tolist() == expected(X[:1])[0][1]
    # onset_detect: the defaults at 22050 / 512 are the reaches (1, 0, 4, 4), wait 1, delta 0.07, normalised
    defaults = dict(pre_max=1, post_max=0, pre_avg=4, post_avg=4, delta=0.07, wait=1, normalise=True)
    want = expected(X, energy="in", **defaults)
    frames = jsg.onset_detect(d)
    assert [f.cpu().tolist() for f in frames] == [w[1] for w in want]
    assert [f.cpu().tolist() for f in jsg.onset_detect(d, backtrack=True)] == [w[2] for w in want]
    other = pr.smooth(2 * B + 5, 15, 3)
    assert [f.cpu().tolist() for f in jsg.onset_detect(d, backtrack=True, energy=other)] == [w[2] for w in expected(X, energy=other, **defaults)]
    one = jsg.onset_detect(d[2], units="samples")
    assert one.dtype == np.int64 and one.tolist() == [512 * f for f in want[2][1]]
    t = jsg.onset_detect(d[2], units="time", sr=16000, hop_length=256, pre_max=0.02, pre_avg=0.08, post_avg=0.08, wait=0.04)
    w = expected(X[2:], pre_max=1, post_max=0, pre_avg=5, post_avg=5, delta=0.07, wait=2, normalise=True)[0][1]
    assert t.dtype == np.float64 and t.tolist() == [f * 256 / 16000 for f in w]
    with pytest.raises(AssertionError):
        jsg.onset_detect(d, units="beats")


def test_onset_backtrack(jsg, torch_cuda):
    torch = torch_cuda
    for T in (1, 50, 2 * B + 5):
        e = pr.smooth(T, 16)[0]
        rng = np.random.default_rng(T)
        events = rng.integers(0, T, 40)          # any order, duplicates, neighbours
        got = jsg.onset_backtrack(events, torch.from_numpy(e).cuda())
        assert got.dtype == torch.int32 and got.cpu().tolist() == pr.back_serial(events.tolist(), e)
    assert jsg.onset_backtrack([], e).numel() == 0
    assert jsg.onset_backtrack(torch.tensor([7, 0, T - 1], device="cuda"), e).cpu().tolist() == pr.back_serial([7, 0, T - 1], e)


def click_track():
    sr, hop, n_fft = 22050, 512, 2048
    x = np.zeros(4 * sr, np.float32)
    clicks = np.arange(sr // 2, 4 * sr - n_fft, sr // 2)
    x[clicks] = 1.0
    return x, clicks, sr, hop, n_fft


def test_onset_detect_audio_on_a_click_track(jsg, torch_cuda):
    """Unit clicks every 0.5 s at 22050 Hz, 4 s, default settings: one onset per click, each within 2 frames of click_sample // hop.  No
    centring is applied to the audio (include/jsg.h section 2j): frame t covers the samples t * hop .. t * hop + n_fft - 1, a click lies in
    the n_fft / hop = 4 frames click // hop - 3 .. click // hop and the flux rises in the first of them.  onset_detect_audio reports an
    onset where its window is centred, n_fft // (2 hop) = 2 frames on, which leaves it one frame before the click; reported at the
    window's first sample it lay 3 frames before (measured: clicks at 21, 43, 64, ..., envelope peaks at 18, 40, 61, ...)."""
    x, clicks, sr, hop, _ = click_track()
    frames = jsg.onset_detect_audio(torch_cuda.from_numpy(x).cuda(), sr).cpu().numpy()
    print("clicks at frames", (clicks // hop).tolist(), "onsets at", frames.tolist())
    assert len(frames) == len(clicks) and (np.abs(frames - clicks // hop) <= 2).all()


@pytest.mark.parametrize("n_fft, hop", [(2048, 512), (1024, 256), (1024, 512)])
def test_onset_detect_audio_reports_the_centre_of_a_window_that_holds_the_click(jsg, torch_cuda, n_fft, hop):
    """Every click has an onset and every onset, less the centring offset n_fft // (2 hop), is one of the frames whose samples t * hop ..
    t * hop + n_fft - 1 hold a click (the flux is zero elsewhere); it equals onset_detect on the envelope shifted by that offset;
    backtracked, at or before the onset; in samples and in seconds, the same frames converted."""
    x, clicks, sr, _, _ = click_track()
    d = torch_cuda.from_numpy(x).cuda()
    offset = n_fft // (2 * hop)
    frames = jsg.onset_detect_audio(d, sr, n_fft, hop).cpu().numpy()
    first = (clicks - n_fft) // hop + 1
    holds = (first[None, :] <= frames[:, None] - offset) & (frames[:, None] - offset <= clicks[None, :] // hop)          # [onset][click]
    assert holds.any(1).all() and holds.any(0).all()
    env = jsg.onset_strength(jsg.mel_spectrogram_db(d, sr, n_fft, hop, 128))
    assert (jsg.onset_detect(env, sr=sr, hop_length=hop).cpu().numpy() + offset).tolist() == frames.tolist()
    back = jsg.onset_detect_audio(d, sr, n_fft, hop, backtrack=True).cpu().numpy()
    assert len(back) == len(frames) and (back <= frames).all() and (back >= offset).all() and (np.diff(back) >= 0).all()
    assert jsg.onset_detect_audio(d, sr, n_fft, hop, units="samples").tolist() == (frames.astype(np.int64) * hop).tolist()
    assert jsg.onset_detect_audio(d, sr, n_fft, hop, units="time").tolist() == [int(f) * hop / sr for f in frames]
