"""Per-channel energy normalisation of libjsgx.so on the GPU (include/jsgx.h section 13) against tests/pcen_ref.py, bit for bit (NaN
positions equal), in pitched buffers full of sentinels that must come back untouched, the input included.  First the graph capture of a
first launch of both forms; then every frame count, band count and row count at which a chunk boundary or the dealing of the chains to
the lanes can go wrong (crossed sparsely: every value appears, and so do the corners); the state in and out and the optional outputs;
three parameter sets, b = 1, subnormal values and values near 2^31; the containment of a NaN; two scratch sizes; a row more than 2^31
elements behind the first; and the Python layer: pcen_audio behind stft_fb on two tones, and the property the operation exists for, a
plane scaled by 1000 with eps scaled alike."""
import functools

import numpy as np
import pytest

import pcen_ref as pr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)
DEFAULTS = dict(pr.PARAMS[0][1])
OUT_BOUND = pr.OUT_BOUND          # |out32 - out64| / (out64 + bias^power) of the definition against the float64 route: profiles/pcen_accuracy.md


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def test_the_sets_are_covered():
    assert {s[0] for s in pr.SHAPES} == set(pr.ROWS_SET) and {s[1] for s in pr.SHAPES} == set(pr.T_SET) and {s[2] for s in pr.SHAPES} == set(pr.B_SET)
    for corner in ((pr.T_SET[0], pr.B_SET[0]), (pr.T_SET[0], pr.B_SET[-1]), (pr.T_SET[-1], pr.B_SET[0]), (pr.T_SET[-1], pr.B_SET[-1])):
        assert corner in {s[1:] for s in pr.SHAPES}


class Guarded:
    """A flat buffer full of `sentinel` and the view [planes][rows][cols] inside it with `pad` extra elements per row and 3 * pad per plane."""

    def __init__(self, torch, planes, rows, cols, pad, sentinel, offset):
        pitch, size = cols + pad, rows * (cols + pad) + 3 * pad
        self.flat = torch.full((planes * size + offset + 5,), sentinel, dtype=torch.float32, device="cuda")
        self.view = torch.as_strided(self.flat, (planes, rows, cols), (size, pitch, 1), storage_offset=offset)
        self.sentinel, self.offset = sentinel, offset

    def untouched(self):
        got = self.flat.cpu().numpy()
        inside = np.zeros(got.size, bool)
        P, R, W = self.view.shape
        v = self.view
        inside[(self.offset + np.arange(P)[:, None, None] * v.stride(0) + np.arange(R)[None, :, None] * v.stride(1) + np.arange(W)[None, None, :]).ravel()] = True
        return bool((got[~inside] == self.sentinel).all() if self.sentinel == self.sentinel else np.isnan(got[~inside]).all())


def run(jsg, torch, M, params=DEFAULTS, *, state=None, want=("state", "smooth"), pad=3, extra_scratch=0):
    """One launch over M float32 [rows][T][B] -> (out, smooth or None, state_out or None) as numpy, after checking that nothing else was
    written: not the padding of any output, not the input buffer, not the state that entered, not the scratch's guard."""
    R, T, B = M.shape
    d_in = Guarded(torch, R, T, B, pad, float("nan"), 3)
    d_out = Guarded(torch, R, T, B, 2 * pad, float(SENTINEL), 1)
    d_smooth = Guarded(torch, R, T, B, pad + 1, float(SENTINEL), 2) if "smooth" in want else None
    d_state = Guarded(torch, 1, R, B, pad, float(SENTINEL), 4) if "state" in want else None
    d_entering = Guarded(torch, 1, R, B, pad + 2, float("nan"), 0) if state is not None else None
    d_in.view.copy_(torch.from_numpy(M))
    if state is not None:
        d_entering.view[0].copy_(torch.from_numpy(np.array(state, np.float32).reshape(R, B)))
    before = [g.flat.clone() for g in (d_in, d_entering) if g is not None]
    d_decay = torch.from_numpy(jsg.pcen_decay(params["b"])).cuda()
    assert pr.same_bits(d_decay.cpu().numpy(), pr.decay(params["b"])), "the table against the restatement"
    kw = dict(params, d_state_in=None if state is None else d_entering.view[0], d_state_out=None if d_state is None else d_state.view[0],
              d_smooth=None if d_smooth is None else d_smooth.view)
    need = jsg.pcen_scratch_bytes(d_in.view, d_decay, d_out.view, **kw)
    chunks = -(-T // pr.CHUNK)
    assert need == (0 if chunks == 1 else 4 * R * chunks * B)
    assert jsg.pcen_plan(T, B, R) == ("pcen_single" if chunks == 1 else "pcen_chunked", 256, 0, 1 if chunks == 1 else 3, chunks)
    d_scratch = torch.full((need // 4 + extra_scratch + 4,), float(SENTINEL), dtype=torch.float32, device="cuda")
    jsg.pcen_launch(d_in.view, d_decay, d_out.view, d_scratch=d_scratch[:need // 4 + extra_scratch], **kw)
    torch.cuda.synchronize()
    for g in (d_out, d_smooth, d_state):
        assert g is None or g.untouched(), "a guard element was written"
    for g, was in zip([g for g in (d_in, d_entering) if g is not None], before):
        assert torch.equal(g.flat.view(torch.int32), was.view(torch.int32)), "an input was written"
    assert (d_scratch[need // 4 + extra_scratch:].cpu().numpy() == SENTINEL).all(), "the scratch's guard was written"
    return (d_out.view.cpu().numpy(), None if d_smooth is None else d_smooth.view.cpu().numpy(), None if d_state is None else d_state.view[0].cpu().numpy())


def check(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert pr.same_bits(got, want), (what, np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))[:4])


def check_all(got, want, what):
    for g, w, name in zip(got, want, ("out", "smooth", "state_out")):
        if g is not None:
            check(g, w, (what, name))


@functools.lru_cache(maxsize=None)
def reference(R, T, B, seed=0, which=0, scale=1.0):
    M = pr.plane(T, B, seed, scale, rows=R)
    out, S, s = pr.pcen32(M, **pr.PARAMS[which][1])
    for a in (M, out, S, s):
        a.setflags(write=False)
    return M, (out, S, s)


def test_graph_capture_of_a_first_launch(jsg, torch_cuda):
    """The three kernels of "pcen_chunked" and the one of "pcen_single" are launched here for the first time in the process, under capture."""
    torch = torch_cuda
    for R, T, B in ((2, 600, 40), (2, 100, 40)):
        M, want = reference(R, T, B, 3)
        d_in = torch.zeros((R, T, B), dtype=torch.float32, device="cuda")
        d_out, d_smooth = torch.full_like(d_in, float(SENTINEL)), torch.full_like(d_in, float(SENTINEL))
        d_state = torch.full((R, B), float(SENTINEL), dtype=torch.float32, device="cuda")
        d_decay = torch.from_numpy(jsg.pcen_decay(DEFAULTS["b"])).cuda()
        d_scratch = torch.empty(max(1, jsg.pcen_scratch_bytes(d_in, d_decay, d_out, **DEFAULTS) // 4), dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                jsg.pcen_launch(d_in, d_decay, d_out, d_state_out=d_state, d_smooth=d_smooth, d_scratch=d_scratch, stream=side.cuda_stream, **DEFAULTS)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == SENTINEL).all() and (d_state.cpu().numpy() == SENTINEL).all()          # captured, not run
        d_in.copy_(torch.from_numpy(np.array(M)))
        g.replay()
        torch.cuda.synchronize()
        check_all((d_out.cpu().numpy(), d_smooth.cpu().numpy(), d_state.cpu().numpy()), want, ("replayed", T))


@pytest.mark.parametrize("R, T, B", pr.SHAPES)
def test_shapes(jsg, torch_cuda, R, T, B):
    M, want = reference(R, T, B)
    check_all(run(jsg, torch_cuda, np.array(M)), want, (R, T, B))


def test_optional_outputs(jsg, torch_cuda):
    """Each optional output absent leaves the others as they are."""
    R, T, B = 3, 513, 40
    M, want = reference(R, T, B)
    for wanted in ((), ("state",), ("smooth",)):
        check_all(run(jsg, torch_cuda, np.array(M), want=wanted), want, wanted)
    M, want = reference(3, 255, 65)
    for wanted in ((), ("state",), ("smooth",)):
        check_all(run(jsg, torch_cuda, np.array(M), want=wanted, pad=0), want, wanted)


@pytest.mark.parametrize("R, T, B", [(3, 513, 40), (1, 100, 65)])
def test_state_in(jsg, torch_cuda, R, T, B):
    """The first frame given as the state equals the default; another state equals the restatement."""
    M, want = reference(R, T, B)
    check_all(run(jsg, torch_cuda, np.array(M), state=M[:, 0, :]), want, "the first frame as the state")
    state = pr.plane(R, B, 11)
    check_all(run(jsg, torch_cuda, np.array(M), state=state), pr.pcen32(M, state=state, **DEFAULTS), "a state of its own")


def test_one_plane_in_two_calls(jsg, torch_cuda):
    """Split at 512 frames with state_out fed to state_in: the single call in every bit."""
    R, T, B = 3, 1000, 31
    M, want = reference(R, T, B)
    first = run(jsg, torch_cuda, np.array(M[:, :512]))
    second = run(jsg, torch_cuda, np.array(M[:, 512:]), state=first[2])
    check(np.concatenate([first[0], second[0]], axis=1), want[0], "out")
    check(np.concatenate([first[1], second[1]], axis=1), want[1], "smooth")
    check(second[2], want[2], "state_out")


@pytest.mark.parametrize("which", range(len(pr.PARAMS)), ids=[p[0] for p in pr.PARAMS])
def test_parameter_sets(jsg, torch_cuda, which):
    M, want = reference(2, 300, 40, 1, which)
    got = run(jsg, torch_cuda, np.array(M), pr.PARAMS[which][1])
    check_all(got, want, pr.PARAMS[which][0])
    assert (got[0][M == 0].view(np.uint32) == 0).all() and (M == 0).any()          # a silent frame gives +0


def test_b_of_one(jsg, torch_cuda):
    M = pr.plane(300, 40, 2, rows=2)
    params = dict(DEFAULTS, b=1.0)
    got = run(jsg, torch_cuda, M, params)
    check(got[1], M, "S = M")
    check_all(got, pr.pcen32(M, **params), "b = 1")


@pytest.mark.parametrize("scale", [2.0 ** 31, 1e-42], ids=["2^31", "subnormal"])
def test_scales(jsg, torch_cuda, scale):
    M = pr.plane(300, 40, 4, scale, rows=2)
    if scale < 1:
        assert (M[M > 0] < 1.1754944e-38).all() and (M > 0).any()
    check_all(run(jsg, torch_cuda, M), pr.pcen32(M, **DEFAULTS), scale)


def test_nan_containment(jsg, torch_cuda):
    R, T, B = 3, 600, 40
    M, clean = reference(R, T, B)
    M = np.array(M)
    r, t0, m = 1, 300, 17
    M[r, t0, m] = np.nan
    got = run(jsg, torch_cuda, M)
    poisoned = np.zeros(M.shape, bool)
    poisoned[r, t0:, m] = True
    for g, c, name in zip(got[:2], clean[:2], ("out", "smooth")):
        assert np.isnan(g[poisoned]).all(), name
        check(np.where(poisoned, 0, g), np.where(poisoned, 0, c), name)
    assert np.isnan(got[2][r, m])
    check(np.delete(got[2].ravel(), r * B + m), np.delete(clean[2].ravel(), r * B + m), "state_out")


def test_two_scratch_sizes(jsg, torch_cuda):
    M, want = reference(3, 513, 63)
    first = run(jsg, torch_cuda, np.array(M))
    second = run(jsg, torch_cuda, np.array(M), extra_scratch=12345)
    check_all(first, second, "two sizes")
    check_all(first, want, "against the restatement")


def test_a_row_pitch_beyond_2_to_31(jsg, torch_cuda):
    """The second row's plane lies more than 2^31 elements behind the first, in the input and in the output (two allocations of 8.6 GB, not
    filled): the kernels' offsets are 64-bit."""
    torch = torch_cuda
    T, B = 300, 40
    M, want = reference(2, T, B, 6)
    pitch = (1 << 31) + 64
    flats = [torch.empty(pitch + T * (B + 1) + 8, dtype=torch.float32, device="cuda") for _ in range(2)]
    d_in, d_out = (torch.as_strided(f, (2, T, B), (pitch, B + 1, 1), storage_offset=3) for f in flats)
    d_in.copy_(torch.from_numpy(np.array(M)))
    d_decay = torch.from_numpy(jsg.pcen_decay(DEFAULTS["b"])).cuda()
    d_state = torch.empty((2, B), dtype=torch.float32, device="cuda")
    jsg.pcen_launch(d_in, d_decay, d_out, d_state_out=d_state, **DEFAULTS)
    torch.cuda.synchronize()
    check(d_out.cpu().numpy(), want[0], "out")
    check(d_state.cpu().numpy(), want[2], "state_out")
    del flats, d_in, d_out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_pcen_returns(jsg, torch_cuda):
    torch = torch_cuda
    M, want = reference(3, 513, 40)
    d = torch.from_numpy(np.array(M)).cuda()
    p = DEFAULTS
    out = jsg.pcen(d, b=p["b"])
    assert tuple(out.shape) == (3, 513, 40)
    check(out.cpu().numpy(), want[0], "out")
    out, state, smooth = jsg.pcen(d, b=p["b"], return_state=True, return_smooth=True)
    check_all((out.cpu().numpy(), smooth.cpu().numpy(), state.cpu().numpy()), want, "all three")
    assert tuple(state.shape) == (3, 40)
    # b from the time constant is the default set's; one plane, block by block with the state
    whole = jsg.pcen(d[0])
    check(whole.cpu().numpy(), want[0][0], "one plane, b from the time constant")
    head, state = jsg.pcen(d[0, :256], return_state=True)
    tail = jsg.pcen(d[0, 256:], state=state)
    assert torch.equal(torch.cat([head, tail]), whole)


def test_pcen_audio_two_tones(jsg, torch_cuda):
    """Two tones at levels 40 dB apart: pcen_audio equals stft_fb with linear_out followed by pcen in every bit, and the quiet tone's band
    comes out of the normalisation within a factor of four of the loud one's, where the band powers themselves are 10^4 apart."""
    torch = torch_cuda
    fs, n, hop, bands = 22050.0, 512, 256, 40
    t = np.arange(300 * hop + n) / fs
    half = t.size // 2
    x = np.where(np.arange(t.size) < half, np.sin(2 * np.pi * 440.0 * t), 0.01 * np.sin(2 * np.pi * 2500.0 * t)).astype(np.float32)
    d_x = torch.from_numpy(x).cuda()
    frames = 1 + (x.size - n) // hop
    plan = jsg.Plan(n, jsg.window(jsg.capi.WIN_HANN, n))
    fb = jsg.Filterbank(n, fs, bands, 0.0, None, scale=jsg.capi.FB_MEL_SLANEY, norm=jsg.capi.FB_NORM_SLANEY)
    S = torch.empty((frames, bands), dtype=torch.float32, device="cuda")
    jsg.stft_fb_db(plan, fb, d_x[None], hop, frames, S, feedblocks=n // hop, linear_out=True)
    torch.cuda.synchronize()
    want = jsg.pcen(S, sr=fs, hop_length=hop)
    got = jsg.pcen_audio(d_x, fs, n, hop, bands)
    assert tuple(got.shape) == (frames, bands) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    V, P = S.cpu().numpy(), got.cpu().numpy()
    check(P, pr.pcen32(V, jsg.pcen_coefficient(0.4, fs, hop))[0], "against the restatement")
    loud, quiet = int(V[:frames // 2 - 2].sum(0).argmax()), int(V[frames // 2 + 2:].sum(0).argmax())
    assert loud != quiet and V[20:frames // 2 - 2, loud].mean() > 3e3 * V[-100:, quiet].mean()
    assert 0.25 < P[-100:, quiet].mean() / P[50:frames // 2 - 2, loud].mean() < 4.0


def test_a_plane_scaled_by_1000(jsg, torch_cuda):
    """With gain = 1 the gain control divides the level out: 1000 M with 1000 eps has 1000 (eps + S), so M g is the same number and so is the
    output.  Each result is within OUT_BOUND (out + bias^power) of its exact value, so the two differ by at most twice that."""
    torch = torch_cuda
    M = pr.plane(600, 40, 8, rows=2)
    d = torch.from_numpy(M).cuda()
    kw = dict(gain=1.0, bias=2.0, power=0.5, b=0.05)
    one, other = jsg.pcen(d, eps=1e-6, **kw).cpu().numpy().astype(np.float64), jsg.pcen(d * 1000.0, eps=1e-3, **kw).cpu().numpy().astype(np.float64)
    worst = float(np.max(np.abs(one - other) / (one + 2.0 ** 0.5)))
    print(f"scaled by 1000: worst difference {worst:.3g} of out + bias^power (bound {2 * OUT_BOUND:.3g})")
    assert worst <= 2 * OUT_BOUND and one.max() > 1.0
