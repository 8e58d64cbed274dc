"""pYIN of libjsgx.so on the GPU (include/jsgx.h section 5) against tests/pyin_ref.py, bit for bit (NaN positions equal, all other bits
equal).  The observation on hand-made d' planes: no trough, one, one at tau_min, equal minima, troughs at h >= 1 only, two troughs in one
bin, periods past both ends of the bin table, the most troughs a frame can hold, one bin, tau_min == tau_max, NaN inside and outside the
lag range, N in 1, 7, 100, 256, tau_max in 2, 63, 64, 65, 1024, one row and three rows in pitched buffers, every optional output missing.
The decoder over pyin_ref.FORM_BINS x FORM_WIDTHS and FORM_PAIRS (every lane split G with both bin counts and both widths at each
boundary, which tests/test_pyin_host.py holds complete) and bands wider than the matrix, frame counts around the block edges of the backtrace, three sequences, the known
answers, a dead frame, a NaN emission, the dense decoder of section 4 on the equivalent matrix on the GPU, graph capture of a first
launch, and pyin() end to end on a tone followed by silence."""
import functools

import numpy as np
import pytest

import pyin_ref as pr
from test_gpu_viterbi import ISENTINEL, SENTINEL, guarded, untouched

pytestmark = pytest.mark.gpu

T_SHAPES = 37
KINDS = ["eighths", "floats"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def block(jsg):
    return jsg.capix.VITERBI_BLOCK


# ---------------------------------------------------------------------------------------------------------------- the decoder
@functools.lru_cache(maxsize=None)
def decoded(kind, T, P, W, seed, dead=0.0):
    """(inputs, V, states, logp) of the restatement; computed once and shared."""
    inp = pr.decode_inputs(kind, T, P, W, seed, dead)
    V, psi, states, logp = pr.decode32(*inp)
    for a in inp + (V, states):
        a.setflags(write=False)
    return inp, V, states, logp


def run_decode(jsg, torch, emits, tables, pad=3, want_value=True, want_logp=True):
    """One launch over the sequences `emits` (equal shapes) in pitched buffers full of sentinels, with a scratch of exactly
    pyin_decode_scratch_bytes and a guard behind it -> (V [Q][T][2P] or None, states [Q][T], logp [Q] or None) as numpy, after checking
    that nothing outside these was written."""
    Q, (T, S) = len(emits), emits[0].shape
    p0, lw, off, sw = tables
    fb, d_emit = guarded(torch, Q, T, S, pad, torch.float32, float("nan"), 3)
    d_emit.copy_(torch.from_numpy(np.stack(emits)))
    d_tab = [torch.from_numpy(np.array(a)).cuda() for a in (p0, lw, off, sw)]
    fv, d_value = guarded(torch, Q, T, S, 2 * pad, torch.float32, float(SENTINEL), 1)
    fs, d_states = guarded(torch, 1, Q, T, pad, torch.int32, int(ISENTINEL), 2)
    d_logp = torch.full((Q + 2,), float(SENTINEL), dtype=torch.float32, device="cuda")
    kw = dict(d_logp=d_logp[1:Q + 1] if want_logp else None, d_value=d_value if want_value else None)
    need = jsg.pyin_decode_scratch_bytes(d_emit, *d_tab, d_states[0], **kw)
    blocks = -(-T // jsg.capix.VITERBI_BLOCK)
    assert need == -(-(4 * Q * S + 4 * Q * blocks + 2 * Q * T * S + 2 * Q * blocks * S) // 4) * 4
    d_scratch = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    jsg.pyin_decode_launch(d_emit, *d_tab, d_states[0], d_scratch=d_scratch[:need], **kw)
    torch.cuda.synchronize()
    assert (d_scratch[need:].cpu().numpy() == 0xA5).all(), "the guard behind the scratch was written"
    assert untouched(fs, d_states, ISENTINEL, 2) and untouched(fv, d_value, SENTINEL, 1), "a guard element was written"
    assert untouched(fb, d_emit, float("nan"), 3) and pr.same_bits(d_emit.cpu().numpy(), np.stack(emits)), "the emissions were written"
    for d, a in zip(d_tab, (p0, lw, off, sw)):
        assert pr.same_bits(d.cpu().numpy(), a), "a table was written"
    lp = d_logp.cpu().numpy()
    assert lp[0] == lp[-1] == SENTINEL
    if not want_logp:
        assert (lp == SENTINEL).all()
    if not want_value:
        assert (fv.cpu().numpy() == SENTINEL).all()
    return d_value.cpu().numpy() if want_value else None, d_states[0].cpu().numpy(), lp[1:Q + 1] if want_logp else None


def check_seq(got, q, want, what):
    V, states, logp = got
    _, wV, wstates, wlogp = want
    if V is not None:
        assert pr.same_bits(V[q], wV), (what, "V", np.argwhere(V[q].view(np.uint32) != wV.view(np.uint32))[:4])
    assert (states[q] == wstates).all(), (what, "states", np.flatnonzero(states[q] != wstates)[:8])
    if logp is not None:
        assert pr.same_bits(logp[q:q + 1], np.asarray([wlogp])), (what, "logp", logp[q], wlogp)


# the first test of the file: no other has launched these kernels before it
def test_graph_capture_of_a_first_launch(jsg, torch_cuda, block):
    """The observation and the decoder (forward, jump, ends, trace) captured on one stream as their first launches and replayed twice
    with changed input."""
    torch = torch_cuda
    R, T, P, W, tau_min, tau_max, N = 2, block + 9, 24, 24, 2, 40, 7      # a band over all bins: a frame with voiced_prob 1 leaves a way on
    tab = observe_tables(P, N, tau_min, tau_max, 100.0, 100.0 / 30.0, 1)
    lw, off, sw = pr.transition_tables(P, np.concatenate([np.arange(1, W + 2), np.arange(W, 0, -1)]).astype(np.float64), 0.01)
    p0 = np.concatenate([np.full(P, -np.inf, np.float32), np.full(P, np.float32(np.log(1.0 / P)), np.float32)])
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(tab, lw=lw, off=off, sw=sw, p0=p0).items()}
    d_plane = torch.ones((R, T, tau_max + 1), dtype=torch.float32, device="cuda")
    d_emit = torch.full((R, T, 2 * P), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_states = torch.full((R, T), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_logp = torch.full((R,), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_scratch = torch.empty((jsg.pyin_decode_scratch_bytes(d_emit, d["p0"], d["lw"], d["off"], d["sw"], d_states, d_logp=d_logp),), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.pyin_observe_launch(d_plane, tau_min, tau_max, d["prior"], d["decay"], d["norm"], d["edges"], d_emit, stream=side.cuda_stream)
            jsg.pyin_decode_launch(d_emit, d["p0"], d["lw"], d["off"], d["sw"], d_states, d_logp=d_logp, d_scratch=d_scratch, stream=side.cuda_stream)
    torch.cuda.synchronize()
    assert (d_states.cpu().numpy() == ISENTINEL).all() and (d_emit.cpu().numpy() == SENTINEL).all()      # captured, not run
    rng = np.random.default_rng(5)
    for _ in range(2):
        plane = np.stack([[smooth_frame(rng, tau_max) for _ in range(T)] for _ in range(R)])
        plane[:, 0] = 1.0           # the model starts unvoiced: a first frame with voiced_prob 1 would leave no path
        d_plane.copy_(torch.from_numpy(plane))
        d_states.fill_(int(ISENTINEL))
        g.replay()
        torch.cuda.synchronize()
        for r in range(R):
            emit = np.stack([pr.observe32(plane[r, t], tau_min, tau_max, tab["prior"], tab["decay"], tab["norm"], tab["edges"], 0.01)[0] for t in range(T)])
            assert pr.same_bits(d_emit[r].cpu().numpy(), emit)
            V, psi, states, logp = pr.decode32(emit, p0, lw, off, sw)
            assert (d_states[r].cpu().numpy() == states).all() and pr.same_bits(d_logp[r:r + 1].cpu().numpy(), np.asarray([logp]))
            assert (states < P).any() and np.isfinite(logp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", pr.FORM_WIDTHS)
@pytest.mark.parametrize("P", pr.FORM_BINS)
def test_decode_over_bins_and_widths(jsg, torch_cuda, P, W, kind):
    """Every lane split that the bin count limits (32 lanes per bin at P <= 16 and W = 128 down to 1 above 256) from its first bin count to
    its last, with no band, a band of one, librosa's 50 and the widest; on inputs with many ties and -inf emissions and on inputs with none."""
    name, G, threads, lds, launches = jsg.pyin_decode_plan(P, W, T_SHAPES)
    assert (name, G, threads, launches) == ("pyin_decode",) + pr.form(P, W) + (3,) and lds == 4 * (4 * (P + 2 * W) + 2 * W + 1)
    want = decoded(kind, T_SHAPES, P, W, 100 + P + W, 0.1 if kind == "eighths" else 0.0)
    check_seq(run_decode(jsg, torch_cuda, [want[0][0]], want[0][1:]), 0, want, (P, W, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P, W", pr.FORM_PAIRS + pr.FORM_WIDE)
def test_decode_on_both_sides_of_the_width_limits_and_with_a_band_wider_than_the_matrix(jsg, torch_cuda, P, W, kind):
    """At P = 16 the width alone decides the lanes per bin: both widths at every change (G = 1 | 2 at W = 7 | 8 ... 16 | 32 at 127 | 128); and
    bands that reach past both ends of the pitch axis from every bin."""
    assert jsg.pyin_decode_plan(P, W, T_SHAPES)[1:3] == pr.form(P, W)
    want = decoded(kind, T_SHAPES, P, W, 300 + P + W, 0.1 if kind == "eighths" else 0.0)
    check_seq(run_decode(jsg, torch_cuda, [want[0][0]], want[0][1:]), 0, want, (P, W, kind))


@pytest.mark.parametrize("seqs", [1, 3])
@pytest.mark.parametrize("P, W", [(7, 2), (129, 50)])
@pytest.mark.parametrize("T", pr.FORM_FRAMES)
def test_decode_frame_counts_and_sequences(jsg, torch_cuda, block, T, P, W, seqs):
    """One frame, two, both sides of a block of the backtrace and three blocks with a short last one; one sequence and three in pitched
    buffers sharing the tables."""
    assert jsg.pyin_decode_plan(P, W, T, seqs)[4] == (3 if T <= block else 4)
    first = decoded("floats", T, P, W, 400 + T)
    wants = [first]
    for q in range(1, seqs):
        b = pr.decode_inputs("eighths" if q == 2 else "floats", T, P, W, 410 + T + q)[0]
        V, psi, states, logp = pr.decode32(b, *first[0][1:])
        wants.append(((b,) + first[0][1:], V, states, logp))
    got = run_decode(jsg, torch_cuda, [w[0][0] for w in wants], first[0][1:])
    for q, want in enumerate(wants):
        check_seq(got, q, want, (T, P, W, q))


@pytest.mark.parametrize("want_value, want_logp", [(False, False), (True, False), (False, True)])
def test_decode_optional_outputs_missing(jsg, torch_cuda, block, want_value, want_logp):
    want = decoded("floats", block + 3, 65, 4, 60)
    check_seq(run_decode(jsg, torch_cuda, [want[0][0]], want[0][1:], want_value=want_value, want_logp=want_logp), 0, want, (want_value, want_logp))


def test_decode_known_answers(jsg, torch_cuda, block):
    """All inputs +0: V = +0, the states are all 0, logp = +0.  A frame of -inf emissions: logp = -inf with JSGX_OK, in its sequence
    only.  A NaN emission on the clean path: V shows it, the path goes round it, nothing else changes."""
    T, P, W = block + 20, 33, 2
    z = lambda *shape: np.zeros(shape, np.float32)
    V, states, logp = run_decode(jsg, torch_cuda, [z(T, 2 * P)], (z(2 * P), z(2 * W + 1), z(P), z(4)))
    assert (V.view(np.uint32) == 0).all() and (states == 0).all() and logp.view(np.uint32)[0] == 0
    inp, V0, states0, logp0 = decoded("floats", T, P, W, 70)
    b = inp[0]
    dead, with_nan = b.copy(), b.copy()
    dead[T // 2] = -np.inf
    with_nan[block - 1, states0[block - 1]] = np.nan
    wants = []
    for e in (with_nan, b, dead):
        Ve, _, se, le = pr.decode32(e, *inp[1:])
        wants.append(((e,) + inp[1:], Ve, se, le))
    assert np.isnan(wants[0][1]).sum() == 1 and np.isfinite(wants[0][3]) and (wants[0][2] != states0).any()
    assert wants[2][3] == -np.inf and np.isneginf(wants[2][1][T // 2:]).all() and pr.same_bits(wants[1][1], V0)
    got = run_decode(jsg, torch_cuda, [w[0][0] for w in wants], inp[1:])
    for q, want in enumerate(wants):
        check_seq(got, q, want, q)


@pytest.mark.parametrize("P, W", [(40, 3), (300, 25)])
def test_decode_equals_the_dense_decoder_on_the_gpu(jsg, torch_cuda, block, P, W):
    """Multiples of 1/8: every sum is exact, so jsgx_viterbi_launch on the dense 2P x 2P matrix of the same model gives the same V, logp
    and states bit for bit (S = 80: "viterbi_dense_lds", S = 600: "viterbi_dense_mem")."""
    torch = torch_cuda
    T = block + 5
    inp, V, states, logp = decoded("eighths", T, P, W, 500 + P, 0.05)
    assert np.isfinite(logp)
    A = pr.dense_of(*inp[2:])
    d_emit, d_init, d_A = (torch.from_numpy(np.array(a)).cuda() for a in (inp[0], inp[1], A))
    d_states = torch.empty((T,), dtype=torch.int32, device="cuda")
    d_logp = torch.empty((1,), dtype=torch.float32, device="cuda")
    d_value = torch.empty((T, 2 * P), dtype=torch.float32, device="cuda")
    jsg.viterbi_launch(d_emit, d_init, d_A, d_states, d_logp=d_logp, d_value=d_value)
    torch.cuda.synchronize()
    dense = (d_value.cpu().numpy()[None], d_states.cpu().numpy()[None], d_logp.cpu().numpy())
    got = run_decode(jsg, torch, [inp[0]], inp[1:])
    assert pr.same_bits(got[0], dense[0]) and (got[1] == dense[1]).all() and pr.same_bits(got[2], dense[2])
    check_seq(got, 0, (inp, V, states, logp), (P, W))


# ---------------------------------------------------------------------------------------------------------------- the observation
def observe_tables(P, N, tau_min, tau_max, sr, fmin, bps, ab=(2, 18)):
    from scipy import stats
    prior = np.diff(stats.beta.cdf(np.linspace(0, 1, N + 1), *ab)).astype(np.float32)
    decay, norm = pr.boltzmann_tables(2.0, max(1, pr.max_troughs(tau_min, tau_max)))
    edges, _ = pr.bins_tables(sr, fmin, bps, P)
    return dict(prior=prior, decay=decay, norm=norm, edges=edges)


def smooth_frame(rng, tau_max):
    h = 1.0 + 0.02 * rng.random(tau_max + 1)
    tau = np.arange(tau_max + 1)
    for c in rng.integers(0, tau_max + 1, int(rng.integers(1, 5))):
        h -= 1.3 * rng.random() * np.exp(-0.5 * ((tau - c) / 1.5) ** 2)
    return np.maximum(h, 1e-4).astype(np.float32)


def hand_made(tau_min, tau_max, seed):
    """Named frames of tau_max + 1 lags; those that need room are left out where the lag range is too short."""
    rng = np.random.default_rng(seed)
    n = tau_max + 1
    tau = np.arange(n)
    f = {"silent": np.ones(n), "falling: no trough": 2.0 - tau / n, "rising: a trough at tau_min": 0.05 + tau / n,
         "random: a trough at every third lag or so": 1.4 * rng.random(n), "smooth dips": smooth_frame(rng, tau_max), "smooth dips 2": smooth_frame(rng, tau_max),
         "comb: the most troughs": np.where((tau - tau_min) % 2 == 0, 0.1, 0.9), "comb above 1": np.where((tau - tau_min) % 2 == 0, 1.0, 1.5)}
    room = tau_max - tau_min
    if room >= 3:
        one = np.full(n, 0.8)
        one[tau_min + 1] = 0.3
        f["one trough"] = one
        f["the only trough at h >= 1"] = np.where(tau == tau_min + 1, 1.0, 2.0)
        flat = np.full(n, 0.8)
        flat[tau_min + 1:tau_min + 3] = 0.3
        f["a flat trough"] = flat
    if room >= 6:
        two = np.full(n, 0.9)
        two[[tau_min + 1, tau_max - 2]] = 0.25
        f["two equal minima at both ends"] = two
        near = np.full(n, 0.9)
        near[[tau_max - 4, tau_max - 2]] = (0.2, 0.4)
        f["two troughs next to each other"] = near
    return {k: np.asarray(v, np.float32) for k, v in f.items()}


@functools.lru_cache(maxsize=None)
def observed(tau_min, tau_max, N, P, seed, rows=1):
    """(names, plane [rows][frames][tau_max + 1], tables, emit, obs, voiced) of the restatement; the rows hold the frames in rotated order."""
    frames = hand_made(tau_min, tau_max, seed)
    names = list(frames)
    # bins: the longest periods lie above edges[0], the shortest at or below edges[P]
    sr, fmin = 1000.0, 1000.0 / (0.7 * tau_max + 1.0)
    tab = observe_tables(P, N, tau_min, tau_max, sr, fmin, 1)
    plane = np.stack([np.stack([frames[names[(i + 2 * r) % len(names)]] for i in range(len(names))]) for r in range(rows)])
    out = [[pr.observe32(h, tau_min, tau_max, tab["prior"], tab["decay"], tab["norm"], tab["edges"], 0.01) for h in row] for row in plane]
    emit, obs, voiced = (np.stack([np.stack([o[i] for o in row]) for row in out]).astype(np.float32) for i in range(3))
    return names, plane, tab, emit, obs, voiced


def run_observe(jsg, torch, plane, tau_min, tau_max, tab, pad=3, want_obs=True, want_voiced=True, no_trough_prob=0.01):
    R, T, lags = plane.shape
    P = tab["edges"].size - 1
    fc, d_plane = guarded(torch, R, T, lags, pad, torch.float32, float("nan"), 3)
    d_plane.copy_(torch.from_numpy(plane))
    d = {k: torch.from_numpy(v).cuda() for k, v in tab.items()}
    fe, d_emit = guarded(torch, R, T, 2 * P, 2 * pad, torch.float32, float(SENTINEL), 1)
    fo, d_obs = guarded(torch, R, T, P, pad, torch.float32, float(SENTINEL), 2)
    fv, d_voiced = guarded(torch, 1, R, T, pad, torch.float32, float(SENTINEL), 1)
    jsg.pyin_observe_launch(d_plane, tau_min, tau_max, d["prior"], d["decay"], d["norm"], d["edges"], d_emit, no_trough_prob=no_trough_prob,
                            d_obs=d_obs if want_obs else None, d_voiced_prob=d_voiced[0] if want_voiced else None)
    torch.cuda.synchronize()
    assert untouched(fe, d_emit, SENTINEL, 1) and untouched(fo, d_obs, SENTINEL, 2) and untouched(fv, d_voiced, SENTINEL, 1), "a guard element was written"
    assert untouched(fc, d_plane, float("nan"), 3) and pr.same_bits(d_plane.cpu().numpy(), plane), "the plane was written"
    for k, v in tab.items():
        assert pr.same_bits(d[k].cpu().numpy(), v), "a table was written"
    if not want_obs:
        assert (fo.cpu().numpy() == SENTINEL).all()
    if not want_voiced:
        assert (fv.cpu().numpy() == SENTINEL).all()
    return d_emit.cpu().numpy(), d_obs.cpu().numpy() if want_obs else None, d_voiced[0].cpu().numpy() if want_voiced else None


def check_observation(got, want, names, what):
    for g, w, part in zip(got, want, ("log_emit", "obs", "voiced_prob")):
        if g is None:
            continue
        for r in range(w.shape[0]):
            for t in range(w.shape[1]):
                assert pr.same_bits(g[r, t], w[r, t]), (what, part, r, names[(t + 2 * r) % len(names)], g[r, t], w[r, t])


@pytest.mark.parametrize("tau_min, tau_max", [(1, 2), (2, 2), (1, 63), (5, 64), (2, 65), (64, 64), (10, 338), (7, 1024), (1, 1024)])
def test_observation_over_lag_ranges(jsg, torch_cuda, tau_min, tau_max):
    """Lag ranges of one, two and many lags, on both sides of one wavefront's 64 lags, librosa's and a long one; tau_min == tau_max holds
    no trough.  Every named frame of hand_made, with 20 bins whose table is shorter than the lag range at both ends."""
    P, N = 20, 100
    names, plane, tab, emit, obs, voiced = observed(tau_min, tau_max, N, P, tau_max)
    assert jsg.pyin_observe_plan(tau_min, tau_max, P) == ("pyin_observe", 64, 4 * (tau_max + 1 + 3 * (pr.max_troughs(tau_min, tau_max) + 1) + P), 1)
    if tau_min == tau_max:
        assert (obs == 0).all() and (voiced == 0).all()
    elif tau_max - tau_min >= 6:
        comb = names.index("comb: the most troughs")
        assert len(pr.troughs_of(plane[0, comb], tau_min, tau_max)) == pr.max_troughs(tau_min, tau_max)
        assert (np.count_nonzero(obs[0], axis=1) > 1).any() and (voiced[0] > 0.5).any() and obs[0][:, 0].any() and obs[0][:, P - 1].any()
        one = names.index("the only trough at h >= 1")
        assert np.count_nonzero(obs[0, one]) == 1 and voiced[0, one] == np.float32(np.float32(0.01) * pr.lane_sum(tab["prior"]))
    check_observation(run_observe(jsg, torch_cuda, plane, tau_min, tau_max, tab), (emit, obs, voiced), names, (tau_min, tau_max))


@pytest.mark.parametrize("N", [1, 7, 100, 256])
@pytest.mark.parametrize("P", [1, 2, 65, 601])
def test_observation_over_thresholds_and_bins(jsg, torch_cuda, N, P):
    """One threshold, fewer than a wavefront, librosa's 100 and all four of a lane; one bin, two, more than a wavefront, librosa's 601.
    With few bins several troughs share one and their probabilities add in lag order."""
    tau_min, tau_max = 3, 90
    names, plane, tab, emit, obs, voiced = observed(tau_min, tau_max, N, P, 1000 + N + P)
    if P <= 2:
        comb = names.index("comb: the most troughs")
        assert len(pr.troughs_of(plane[0, comb], tau_min, tau_max)) > P
    check_observation(run_observe(jsg, torch_cuda, plane, tau_min, tau_max, tab), (emit, obs, voiced), names, (N, P))


def test_observation_of_three_rows_in_pitched_buffers(jsg, torch_cuda):
    tau_min, tau_max, N, P = 4, 70, 100, 33
    names, plane, tab, emit, obs, voiced = observed(tau_min, tau_max, N, P, 77, rows=3)
    together = run_observe(jsg, torch_cuda, plane, tau_min, tau_max, tab)
    check_observation(together, (emit, obs, voiced), names, "three rows")
    alone = run_observe(jsg, torch_cuda, plane[1:2], tau_min, tau_max, tab, pad=0)
    for a, b in zip(alone, together):
        assert pr.same_bits(a[0], b[1])


@pytest.mark.parametrize("want_obs, want_voiced", [(False, False), (True, False), (False, True)])
def test_observation_optional_outputs_missing(jsg, torch_cuda, want_obs, want_voiced):
    tau_min, tau_max, N, P = 4, 70, 100, 33
    names, plane, tab, emit, obs, voiced = observed(tau_min, tau_max, N, P, 77, rows=3)
    got = run_observe(jsg, torch_cuda, plane, tau_min, tau_max, tab, want_obs=want_obs, want_voiced=want_voiced)
    assert (got[1] is None) == (not want_obs) and (got[2] is None) == (not want_voiced)
    check_observation(got, (emit, obs, voiced), names, (want_obs, want_voiced))


def test_observation_with_a_nan_inside_and_outside_the_lag_range(jsg, torch_cuda):
    """A NaN inside tau_min..tau_max: the frame is unobserved (obs 0, voiced_prob NaN, voiced emissions -inf, unvoiced L(1 / P)); a NaN at
    tau_min - 1 or at lag 0 changes at most the parabola of a trough at tau_min, as the restatement has it; the neighbouring frames keep
    their bits."""
    tau_min, tau_max, N, P = 4, 70, 100, 33
    names, plane, tab, emit, obs, voiced = observed(tau_min, tau_max, N, P, 77)
    plane = plane.copy()
    inside, outside, low = names.index("smooth dips"), names.index("smooth dips 2"), names.index("rising: a trough at tau_min")
    plane[0, inside, 30] = np.nan
    plane[0, outside, 0] = np.nan
    plane[0, low, tau_min - 1] = np.nan
    want = [pr.observe32(h, tau_min, tau_max, tab["prior"], tab["decay"], tab["norm"], tab["edges"], 0.01) for h in plane[0]]
    w_emit, w_obs, w_voiced = (np.stack([w[i] for w in want])[None].astype(np.float32) for i in range(3))
    assert np.isnan(w_voiced[0, inside]) and np.isnan(w_voiced).sum() == 1 and np.isneginf(w_emit[0, inside, :P]).all()
    assert (w_emit[0, inside, P:] == pr.log32(np.float32(1) / np.float32(P))).all()
    others = [i for i in range(len(names)) if i not in (inside, low)]
    assert pr.same_bits(w_emit[0, others], emit[0, others]) and pr.same_bits(w_voiced[0, others], voiced[0, others])
    got = run_observe(jsg, torch_cuda, plane, tau_min, tau_max, tab)
    check_observation(got, (w_emit, w_obs, w_voiced), names, "nan")
    # the decoder goes through the unobserved frame
    lw, off, sw = pr.transition_tables(P, [1.0, 2.0, 1.0], 0.01)
    p0 = np.concatenate([np.full(P, -np.inf, np.float32), np.full(P, np.float32(np.log(1.0 / P)), np.float32)])
    want_dec = pr.decode32(got[0][0], p0, lw, off, sw)
    assert np.isfinite(want_dec[3]) and want_dec[2][inside] >= P
    V, states, logp = run_decode(jsg, torch_cuda, [got[0][0]], (p0, lw, off, sw))
    assert (states[0] == want_dec[2]).all() and pr.same_bits(logp, np.asarray([want_dec[3]])) and pr.same_bits(V[0], want_dec[0])


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_pyin_on_a_tone_followed_by_silence(jsg, torch_cuda):
    """0.5 s of a 220 Hz sine, then 0.5 s of zeros, at 22 050 Hz with the default arguments between C2 and C7 (601 bins, W = 50, tau
    10..338).  Frame t covers the samples t * 512 - 1024 .. t * 512 + 1024: the frames 2..19 lie wholly in the tone and must be voiced with
    f0 within 10 cents of 220 Hz (one bin of the 0.1-semitone grid); the frames from 24 on lie wholly in the zeros and must be unvoiced
    with voiced_prob == 0 and f0 = fill_na."""
    torch = torch_cuda
    sr, hop, n = 22050, 512, 11025
    x = np.concatenate([np.sin(2 * np.pi * 220.0 * np.arange(n) / sr), np.zeros(n)]).astype(np.float32)
    fmin, fmax = 65.40639132514966, 2093.004522404789
    assert jsg.pyin_geometry(sr, fmin, fmax) == (10, 601, 50, 10, 338)
    f0, flag, prob = jsg.pyin(x, sr, fmin, fmax)
    T = 1 + len(x) // hop
    assert f0.shape == flag.shape == prob.shape == (T,) and f0.dtype == np.float32 and flag.dtype == bool and prob.dtype == np.float32
    tone = [t for t in range(T) if t * hop - 1024 >= 0 and t * hop + 1024 <= n]
    zeros = [t for t in range(T) if t * hop - 1024 >= n]
    assert tone == list(range(2, 20)) and zeros[0] == 24 and len(zeros) >= 18
    cents = 1200 * np.log2(f0[tone].astype(np.float64) / 220.0)
    print("tone: voiced_prob", prob[tone].min(), "..", prob[tone].max(), "cents", cents.min(), "..", cents.max())
    assert flag[tone].all() and (np.abs(cents) <= 10).all()
    assert (~flag[zeros]).all() and (prob[zeros] == 0).all() and np.isnan(f0[zeros]).all()
    f0b, flagb, probb = jsg.pyin(torch.from_numpy(np.stack([x, x])).cuda(), sr, fmin, fmax, fill_na=-1.0)
    assert f0b.is_cuda and tuple(f0b.shape) == (2, T) and flagb.dtype == torch.bool
    for r in range(2):
        assert (flagb[r].cpu().numpy() == flag).all() and pr.same_bits(probb[r].cpu().numpy(), prob)
        assert (f0b[r].cpu().numpy()[zeros] == -1).all() and pr.same_bits(f0b[r].cpu().numpy()[tone], f0[tone])
    with pytest.raises(jsg.JsgError, match="pitch bins"):
        jsg.pyin(x, sr, 30.0, 8000.0, resolution=0.05)
    with pytest.raises(jsg.JsgError, match="half-width"):
        jsg.pyin(x, sr, fmin, fmax, hop_length=2048, frame_length=4096)
