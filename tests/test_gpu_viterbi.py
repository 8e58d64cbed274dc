"""Viterbi decoding of libjsgx.so on the GPU (include/jsgx.h section 4) against tests/viterbi_ref.py, bit for bit (NaN positions equal, all
other bits equal): V, the states and logp over viterbi_ref.FORM_STATES (every lane split G = 64 ... 1 in both dense forms with both state
counts at each of the seven boundaries, which tests/test_jsgx_forms_host.py holds complete, and a lane's second state), with maxima tied
across the lanes of a destination; viterbi_ref.FORM_BANDS (for every G a band narrower than, next to and wider than the lane split, both
band forms on both sides of the LDS limit, the never-read entries poisoned); frame counts around the block edges of the backtrace and over
several blocks; three sequences in pitched buffers full of sentinels; missing optional outputs; a NaN emission and a dead frame that stay
in their sequence, dense and band; an exact scratch with a guard behind it; graph capture of a first launch of a large-LDS form and a
first launch of the band form at its largest LDS; and the Python layer end to end."""
import functools

import numpy as np
import pytest

import viterbi_ref as vr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
ISENTINEL = np.int32(-77777)
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
    assert jsg.viterbi_plan(7, jsg.capix.VITERBI_BLOCK)[3] == 3 and jsg.viterbi_plan(7, jsg.capix.VITERBI_BLOCK + 1)[3] == 4
    return jsg.capix.VITERBI_BLOCK


@functools.lru_cache(maxsize=None)
def reference(kind, T, S, seed, W=None):
    """(log_emit, log_init, trans, V, states, logp) of the restatement; computed once and shared."""
    b, p0, A = vr.inputs(kind, T, S, seed, band_half=W)
    V, psi, states, logp = vr.viterbi32(b, p0, A, band_half=W)
    for a in (b, p0, A, V, states):
        a.setflags(write=False)
    return b, p0, A, V, states, logp


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


def run(jsg, torch, emits, p0, trans, W=None, pad=3, want_value=True, want_logp=True):
    """One launch over the sequences `emits` (equal shapes) in pitched buffers full of sentinels, with a scratch of exactly
    viterbi_scratch_bytes and a guard behind it -> (V [Q][T][S] or None, states [Q][T], logp [Q] or None) as numpy, after checking that
    nothing outside these was written and that the inputs are as they were."""
    Q, (T, S) = len(emits), emits[0].shape
    fb, d_emit = guarded(torch, Q, T, S, pad, torch.float32, float("nan"), 3)
    d_emit.copy_(torch.from_numpy(np.stack(emits)))
    fa, d_trans = guarded(torch, 1, trans.shape[0], S, 2 * pad, torch.float32, float("nan"), 1)
    d_trans.copy_(torch.from_numpy(np.array(trans)[None]))
    d_init = torch.from_numpy(np.array(p0)).cuda()
    fv, d_value = guarded(torch, Q, T, S, 2 * pad, torch.float32, float(SENTINEL), 1)
    fs, d_states = guarded(torch, 1, Q, T, pad, torch.int32, int(ISENTINEL), 2)
    d_logp = torch.full((Q + 2,), float(SENTINEL), dtype=torch.float32, device="cuda")
    kw = dict(band_half=W, d_logp=d_logp[1:Q + 1] if want_logp else None, d_value=d_value if want_value else None)
    need = jsg.viterbi_scratch_bytes(d_emit, d_init, d_trans[0], d_states[0], **kw)
    blocks = -(-T // jsg.capix.VITERBI_BLOCK)
    assert need == -(-(4 * Q * S + 4 * Q * blocks + 2 * Q * T * S + 2 * Q * blocks * S) // 4) * 4
    d_scratch = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    jsg.viterbi_launch(d_emit, d_init, d_trans[0], d_states[0], d_scratch=d_scratch[:need], **kw)
    torch.cuda.synchronize()
    assert (d_scratch[need:].cpu().numpy() == 0xA5).all(), "the guard behind the scratch was written"
    assert untouched(fs, d_states, ISENTINEL, 2) and untouched(fv, d_value, SENTINEL, 1), "a guard element was written"
    assert untouched(fb, d_emit, float("nan"), 3) and vr.same_bits(d_emit.cpu().numpy(), np.stack(emits)), "the emissions were written"
    assert untouched(fa, d_trans, float("nan"), 1) and vr.same_bits(d_trans[0].cpu().numpy(), trans) and vr.same_bits(d_init.cpu().numpy(), p0), "an input was written"
    lp = d_logp.cpu().numpy()
    assert lp[0] == lp[-1] == SENTINEL
    if not want_logp:
        assert (lp == SENTINEL).all()
    if not want_value:
        assert (fv.cpu().numpy() == SENTINEL).all()
    return d_value.cpu().numpy() if want_value else None, d_states[0].cpu().numpy(), lp[1:Q + 1] if want_logp else None


def check_seq(got, q, want, what):
    V, states, logp = got
    _, _, _, wV, wstates, wlogp = want
    if V is not None:
        assert vr.same_bits(V[q], wV), (what, "V", np.argwhere(V[q].view(np.uint32) != wV.view(np.uint32))[:4])
    assert (states[q] == wstates).all(), (what, "states", np.flatnonzero(states[q] != wstates)[:8])
    if logp is not None:
        assert vr.same_bits(logp[q:q + 1], np.asarray([wlogp])), (what, "logp", logp[q], wlogp)


# the first test of the file: no other has launched this form before it
def test_graph_capture_of_a_first_launch_of_a_large_lds_form(jsg, torch_cuda, block):
    """"viterbi_dense_lds" at S = 192 holds 148992 bytes of LDS, which takes the per-device opt-in: a first launch of it captured
    (forward, jump, ends, trace on the one stream: a plain chain) and replayed twice with changed input."""
    torch = torch_cuda
    S, T = 192, block + 9
    assert jsg.viterbi_plan(S, T, seqs=2) == ("viterbi_dense_lds", 768, 148992, 4)
    d_emit = torch.zeros((2, T, S), dtype=torch.float32, device="cuda")
    d_init = torch.zeros((S,), dtype=torch.float32, device="cuda")
    d_trans = torch.zeros((S, S), dtype=torch.float32, device="cuda")
    d_states = torch.full((2, T), int(ISENTINEL), dtype=torch.int32, device="cuda")
    d_logp = torch.full((2,), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_value = torch.full((2, T, S), float(SENTINEL), dtype=torch.float32, device="cuda")
    kw = dict(d_logp=d_logp, d_value=d_value)
    d_scratch = torch.empty((jsg.viterbi_scratch_bytes(d_emit, d_init, d_trans, d_states, **kw),), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            jsg.viterbi_launch(d_emit, d_init, d_trans, d_states, d_scratch=d_scratch, stream=side.cuda_stream, **kw)
    torch.cuda.synchronize()
    assert (d_states.cpu().numpy() == ISENTINEL).all() and (d_logp.cpu().numpy() == SENTINEL).all()      # captured, not run
    for seeds in ((21, 22), (23, 24)):
        wants = [reference("floats", T, S, seed) for seed in seeds]
        assert vr.same_bits(wants[0][1], wants[1][1]) is False      # the shared inputs are those of the first sequence
        d_emit.copy_(torch.from_numpy(np.stack([w[0] for w in wants])))
        d_init.copy_(torch.from_numpy(np.array(wants[0][1])))
        d_trans.copy_(torch.from_numpy(np.array(wants[0][2])))
        d_states.fill_(int(ISENTINEL))
        g.replay()
        torch.cuda.synchronize()
        got = (d_value.cpu().numpy(), d_states.cpu().numpy(), d_logp.cpu().numpy())
        check_seq(got, 0, wants[0], ("replay", seeds, 0))
        V, psi, states, logp = vr.viterbi32(wants[1][0], wants[0][1], wants[0][2])
        check_seq(got, 1, (None, None, None, V, states, logp), ("replay", seeds, 1))


# the second test of the file: no other has launched a band form before it
def test_first_launch_of_the_band_form_at_its_largest_lds(jsg, torch_cuda):
    """"viterbi_band_lds" at S = 312, W = 64 holds 163488 of the 163840 bytes of LDS: the first launch of the form tells the device the limit."""
    S, W = 312, 64
    assert jsg.viterbi_plan(S, T_SHAPES, band_half=W) == ("viterbi_band_lds", 640, 163488, 3)
    want = reference("floats", T_SHAPES, S, 200 + S + W, W)
    assert len(np.unique(want[4])) > 3 and np.isfinite(want[5])
    check_seq(run(jsg, torch_cuda, [want[0]], want[1], want[2], W=W), 0, want, (S, W, "first launch"))


def ties_across_lanes(want, G):
    """The number of (t, j), t >= 1, whose maximum over the sources is attained by sources that different lanes of the G hold (i % G differs),
    from the reference's V and the dense matrix."""
    b, p0, A, V, states, logp = want
    count = 0
    with np.errstate(invalid="ignore"):
        for t in range(1, V.shape[0]):
            w = V[t - 1][:, None] + A                                    # [i][j]
            w = np.where(np.isnan(w), vr.NEG_INF, w)
            at_top = w == w.max(axis=0)[None, :]
            lanes = np.zeros((G, A.shape[1]), bool)
            np.logical_or.at(lanes, np.arange(A.shape[0]) % G, at_top)
            count += int((lanes.sum(axis=0) > 1).sum())
    return count


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", vr.FORM_STATES)
def test_dense_over_state_counts(jsg, torch_cuda, S, kind):
    """Every lane split (64 lanes per destination at S <= 16, 32 up to 32, ... 1 above 512) from its first state count to its last, both
    dense forms (192 | 193) and a lane owning a second destination (1025, 2048), on inputs with many ties and -inf and on inputs with
    none.  From S = 16 on, wherever G > 1, the eighths tie the maximum of 20 destinations or more across lanes (28 at S = 16, 3163 at 512),
    so that the xor reduction has to apply the pair rule."""
    name, threads, lds, launches = jsg.viterbi_plan(S, T_SHAPES)
    assert name == ("viterbi_dense_lds" if S <= 192 else "viterbi_dense_mem") and launches == 3 and threads == vr.form(S)[1] <= 1024
    want = reference(kind, T_SHAPES, S, 100 + S)
    G = vr.form(S)[0]
    if kind == "eighths" and S >= 16 and G > 1:
        tied = ties_across_lanes(want, G)
        print(f"S={S} G={G}: {tied} destinations with a maximum tied across lanes")
        assert tied >= 20, (S, G, tied)
    check_seq(run(jsg, torch_cuda, [want[0]], want[1], want[2]), 0, want, (S, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S, W", vr.FORM_BANDS)
def test_band_shapes(jsg, torch_cuda, S, W, kind):
    """Both band forms on both sides of the LDS limit (312 | 313 at W = 64); for every lane split G a band with fewer sources per destination
    than lanes, one next to G and one with more; W = 0, a band as wide as the matrix and one wider; the entries of the table whose source
    lies outside the matrix hold 1e30 and must not show."""
    name = jsg.viterbi_plan(S, T_SHAPES, band_half=W)[0]
    assert name == ("viterbi_band_mem" if (S, W) in ((1200, 25), (2048, 64), (313, 64)) else "viterbi_band_lds")
    want = reference(kind, T_SHAPES, S, 200 + S + W, W)
    assert W == 0 or (want[2] == np.float32(1e30)).any()
    check_seq(run(jsg, torch_cuda, [want[0]], want[1], want[2], W=W), 0, want, (S, W, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", [7, 193])
@pytest.mark.parametrize("index", range(8))
def test_frame_counts_around_the_block_edges(jsg, torch_cuda, block, index, S, kind):
    """T from {1, 2, B-1, B, B+1, 2B, 2B+1, 5B+7}: one frame, the launch without the jump kernel up to T = B, a last block of one frame,
    and six blocks with a short last one."""
    B = block
    T = [1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 5 * B + 7][index]
    assert jsg.viterbi_plan(S, T)[3] == (3 if T <= B else 4)
    want = reference(kind, T, S, 300 + index)
    check_seq(run(jsg, torch_cuda, [want[0]], want[1], want[2]), 0, want, (T, S, kind))


def test_a_band_over_several_blocks(jsg, torch_cuda, block):
    T, S, W = 3 * block + 5, 70, 2
    want = reference("floats", T, S, 41, W)
    assert len(np.unique(want[4])) > 3
    check_seq(run(jsg, torch_cuda, [want[0]], want[1], want[2], W=W), 0, want, (T, S, W))


@pytest.mark.parametrize("S, W", [(70, None), (300, None), (33, 5)])
def test_three_sequences_against_three_single_launches(jsg, torch_cuda, block, S, W):
    T = block + 30
    wants = [reference("floats", T, S, 50, W)]
    for seed in (51, 52):
        b = vr.inputs("eighths" if seed == 52 else "floats", T, S, seed, band_half=W)[0]
        V, psi, states, logp = vr.viterbi32(b, wants[0][1], wants[0][2], band_half=W)
        wants.append((b, wants[0][1], wants[0][2], V, states, logp))
    together = run(jsg, torch_cuda, [w[0] for w in wants], wants[0][1], wants[0][2], W=W)
    for q, want in enumerate(wants):
        check_seq(together, q, want, ("together", q))
        alone = run(jsg, torch_cuda, [want[0]], want[1], want[2], W=W, pad=0)
        check_seq(alone, 0, want, ("alone", q))
        assert vr.same_bits(alone[0][0], together[0][q]) and (alone[1][0] == together[1][q]).all() and vr.same_bits(alone[2], together[2][q:q + 1])


@pytest.mark.parametrize("want_value, want_logp", [(False, False), (True, False), (False, True)])
def test_optional_outputs_missing(jsg, torch_cuda, block, want_value, want_logp):
    first = reference("floats", block + 3, 65, 60)
    b = vr.inputs("eighths", block + 3, 65, 61)[0]
    V, psi, states, logp = vr.viterbi32(b, first[1], first[2])
    wants = [first, (b, first[1], first[2], V, states, logp)]
    got = run(jsg, torch_cuda, [w[0] for w in wants], wants[0][1], wants[0][2], want_value=want_value, want_logp=want_logp)
    for q, want in enumerate(wants):
        check_seq(got, q, want, (want_value, want_logp, q))


def test_a_nan_emission_and_a_dead_frame_stay_in_their_sequence(jsg, torch_cuda, block):
    T, S = block + 20, 40
    b, p0, A, V, states, logp = reference("floats", T, S, 70)
    with_nan, dead = b.copy(), b.copy()
    with_nan[block - 1, states[block - 1]] = np.nan         # on the clean path, at the last frame of a block
    dead[T // 2] = -np.inf
    wants = []
    for e in (with_nan, b, dead):
        Ve, _, se, le = vr.viterbi32(e, p0, A)
        wants.append((e, p0, A, Ve, se, le))
    assert np.isnan(wants[0][3]).sum() == 1 and np.isfinite(wants[0][5]) and (wants[0][4] != states).any()
    assert wants[2][5] == -np.inf and (wants[2][4][T // 2:] == 0).all() and vr.same_bits(wants[1][3], V)
    got = run(jsg, torch_cuda, [w[0] for w in wants], p0, A)
    for q, want in enumerate(wants):
        check_seq(got, q, want, q)


def test_a_dead_frame_in_the_band_form(jsg, torch_cuda, block):
    """S = 24 (32 lanes per destination, 7 sources at the most: most lanes of a destination hold no source), W = 3, the table of the
    builder from a window with zero weights, so that the table itself holds -inf inside the band; one frame of one sequence all -inf.
    From there on every source of a destination ties at -inf and the lowest one inside the band wins, max(0, j - W)."""
    T, S, W = block + 20, 24, 3
    band = jsg.viterbi_band_transition(S, [0.0, 0.5, 0.0, 1.0, 0.25, 0.0, 0.125])
    assert band.shape == (2 * W + 1, S) and np.isneginf(band[[1, 4, 6]]).all() and np.isfinite(band[3]).all()      # row r holds window[2W - r]
    b, p0, _ = vr.inputs("floats", T, S, 75)
    dead = b.copy()
    dead[T // 2] = -np.inf
    wants = []
    for e in (b, dead, b):
        Ve, psi, se, le = vr.viterbi32(e, p0, band, band_half=W)
        wants.append((e, p0, band, Ve, se, le))
    assert np.isfinite(wants[0][5]) and len(np.unique(wants[0][4])) > 3
    assert wants[1][5] == -np.inf and np.isneginf(wants[1][3][T // 2:]).all() and np.isfinite(wants[1][3][:T // 2]).all()
    assert (wants[1][4][T // 2:] == 0).all() and (wants[1][4][:T // 2] != 0).any()      # from the end state 0 down max(0, j - W) = 0
    got = run(jsg, torch_cuda, [w[0] for w in wants], p0, band, W=W)
    for q, want in enumerate(wants):
        check_seq(got, q, want, q)


@pytest.mark.parametrize("kind", KINDS)
def test_several_backtrace_blocks_in_the_32_lane_form(jsg, torch_cuda, block, kind):
    """S = 24 over 3 B + 5 frames: four blocks with a short last one; the jump kernel composes psi of the form with 32 lanes per destination."""
    T, S = 3 * block + 5, 24
    assert vr.form(S)[0] == 32 and jsg.viterbi_plan(S, T)[3] == 4
    want = reference(kind, T, S, 330)
    assert kind == "eighths" or len(np.unique(want[4])) > 3
    check_seq(run(jsg, torch_cuda, [want[0]], want[1], want[2]), 0, want, (T, S, kind))


def test_all_zero_inputs(jsg, torch_cuda, block):
    """The header's known answer: states all 0, logp +0, V +0 everywhere, dense and band."""
    T, S = block + 2, 66
    z = lambda *shape: np.zeros(shape, np.float32)
    for W in (None, 3):
        V, states, logp = run(jsg, torch_cuda, [z(T, S)], z(S), z(S, S) if W is None else z(2 * W + 1, S), W=W)
        assert (V.view(np.uint32) == 0).all() and (states == 0).all() and logp.view(np.uint32)[0] == 0


def test_a_scratch_one_byte_short_is_refused(jsg, torch_cuda):
    """run() gives every launch exactly viterbi_scratch_bytes with a guard behind; one byte fewer is refused and nothing is enqueued."""
    torch = torch_cuda
    T, S = 10, 9
    b, p0, A = (torch.from_numpy(x).cuda() for x in vr.inputs("floats", T, S, 80))
    d_states = torch.full((T,), int(ISENTINEL), dtype=torch.int32, device="cuda")
    need = jsg.viterbi_scratch_bytes(b, p0, A, d_states)
    assert need == 4 * S + 4 + 2 * T * S + 2 * S + 2       # rounded up to a multiple of 4
    d_scratch = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    with pytest.raises(jsg.JsgError, match="scratch smaller than jsgx_viterbi_scratch_bytes"):
        jsg.viterbi_launch(b, p0, A, d_states, d_scratch=d_scratch[:need - 1])
    torch.cuda.synchronize()
    assert (d_states.cpu().numpy() == ISENTINEL).all()
    jsg.viterbi_launch(b, p0, A, d_states, d_scratch=d_scratch)
    torch.cuda.synchronize()
    assert (d_states.cpu().numpy() == vr.viterbi32(*vr.inputs("floats", T, S, 80))[2]).all()


def test_viterbi_end_to_end(jsg, torch_cuda, block):
    """viterbi(...) from numpy and from CUDA tensors, one sequence and a batch, dense and band, with the default (uniform) log_init."""
    torch = torch_cuda
    T, S, W = block + 11, 48, 4
    b, _, A = vr.inputs("floats", T, S, 90)
    uniform = np.full(S, np.float32(np.log(1.0 / S)), np.float32)
    V, psi, want_states, want_logp = vr.viterbi32(b, uniform, A)
    for emit, trans in ((b, A), (torch.from_numpy(b).cuda(), torch.from_numpy(A).cuda())):
        states, logp = jsg.viterbi(emit, trans)
        assert states.is_cuda and states.dtype == torch.int32 and tuple(states.shape) == (T,) and logp.dtype == torch.float32 and logp.dim() == 0
        assert (states.cpu().numpy() == want_states).all() and vr.same_bits(logp.cpu().numpy(), want_logp)
    # a batch, a given log_init, the band form from the builder
    window = np.hanning(2 * W + 3)[1:-1]
    band = jsg.viterbi_band_transition(S, window)
    b2, p0, _ = vr.inputs("floats", T, S, 91)
    states, logp = jsg.viterbi(np.stack([b, b2]), band, p0, band_half=W)
    assert tuple(states.shape) == (2, T) and tuple(logp.shape) == (2,)
    for q, e in enumerate((b, b2)):
        V, psi, s, lp = vr.viterbi32(e, p0, band, band_half=W)
        assert (states[q].cpu().numpy() == s).all() and vr.same_bits(logp[q].cpu().numpy(), lp) and (np.abs(np.diff(s)) <= W).all()
