"""Harmonic-percussive separation on the GPU (include/jsg.h section 2f).  Every comparison is bit for bit against the float32 numpy
restatement of tests/hpss_ref.py, masks and outputs: geometries at the tile and window edges, margins, ties and zero windows, chunk
lengths, real power input, output subsets, rows, pitched buffers, containment of NaN / Inf / negative values, graph capture, the
Python layer (hpss, hpss_audio) and the round trip y_h + y_p."""
import functools

import numpy as np
import pytest

import hpss_ref as hr

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25e11)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


@functools.lru_cache(maxsize=64)
def mirror(T, K, W_t, W_f, m_h=1.0, m_p=1.0, kind="noise", real=False):
    """The restatement of a shared input, computed once: (mask_h, mask_p, out_h, out_p)."""
    X = hr.tie_input(T, K) if kind == "ties" else hr.make_input(T, K)
    return hr.mirror(hr.power(X) if real else X, W_t, W_f, m_h, m_p)[:4]


def raw(a):
    """The bits of a float32 or complex64 numpy array."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(raw(a), raw(b))


def run(jsg, torch, X, W, margin=1.0, want=(True, True, True, True), **kw):
    """X: numpy [T][K] or [rows][T][K], complex64 or float32 power -> the requested of (mask_h, mask_p, out_h, out_p) as numpy arrays
    of one launch into dense sentinel-filled buffers (None for those not requested)."""
    d_X = torch.from_numpy(np.array(X)).cuda()      # a copy: the shared inputs are read-only
    new = lambda dtype: torch.full(d_X.shape, float(SENTINEL), dtype=dtype, device="cuda")
    mh, mp, oh, op = (new(dt) if w else None for w, dt in zip(want, (torch.float32, torch.float32, d_X.dtype, d_X.dtype)))
    jsg.hpss_launch(d_X, d_harm=oh, d_perc=op, d_mask_h=mh, d_mask_p=mp, kernel_size=W, margin=margin, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (mh, mp, oh, op))


def check_all(got, want, where=None):
    for name, g, w in zip(("mask_h", "mask_p", "out_h", "out_p"), got, want):
        if where is not None:
            g, w = g[where], w[where]
        assert same(g, w), name


@pytest.mark.parametrize("g", hr.GEOMETRIES, ids=hr.geometry_id)
def test_bits_equal_the_restatement(jsg, torch_cuda, g):
    T, K, W_t, W_f = g
    check_all(run(jsg, torch_cuda, hr.make_input(T, K), (W_t, W_f)), mirror(T, K, W_t, W_f))


@pytest.mark.parametrize("g", [(96, 257, 31, 31), (200, 130, 17, 9)], ids=hr.geometry_id)
@pytest.mark.parametrize("margins", [(1.0, 1.0), (2.0, 1.0), (1.0, 3.5)], ids=str)
def test_margins(jsg, torch_cuda, g, margins):
    T, K, W_t, W_f = g
    check_all(run(jsg, torch_cuda, hr.make_input(T, K), (W_t, W_f), margins), mirror(T, K, W_t, W_f, *margins))


@pytest.mark.parametrize("g", [(96, 257, 31, 31), (200, 130, 17, 9)], ids=hr.geometry_id)
def test_ties_and_zero_windows(jsg, torch_cuda, g):
    """Parts drawn from {0, 1, 2, 3} and a block of zeros: equal values in every window, and the zero-denominator branch."""
    T, K, W_t, W_f = g
    got, want = run(jsg, torch_cuda, hr.tie_input(T, K), (W_t, W_f)), mirror(T, K, W_t, W_f, kind="ties")
    check_all(got, want)
    dead = (want[0] == 0) & (want[1] == 0)
    assert dead.sum() > 0 and (raw(got[0])[dead] == 0).all() and (raw(got[1])[dead] == 0).all()


def test_same_bits_for_every_chunk_length_and_on_repeat(jsg, torch_cuda):
    T, K, W = 96, 257, (31, 31)
    X, want = hr.make_input(T, K), mirror(T, K, *W)
    for chunk in (1, 7, 32, 0, 0):
        check_all(run(jsg, torch_cuda, X, W, chunk_frames=chunk), want)


@pytest.mark.parametrize("g", [(96, 257, 31, 31), (67, 129, 3, 5)], ids=hr.geometry_id)
def test_real_power_input(jsg, torch_cuda, g):
    """The masks of the complex call whose power it is; the outputs are M * P."""
    T, K, W_t, W_f = g
    got = run(jsg, torch_cuda, hr.power(hr.make_input(T, K)), (W_t, W_f))
    check_all(got, mirror(T, K, W_t, W_f, real=True))
    check_all(got[:2], mirror(T, K, W_t, W_f)[:2])
    assert got[2].dtype == np.float32 and same(got[2], got[0] * hr.power(hr.make_input(T, K)))


@pytest.mark.parametrize("only", range(4), ids=["mask_h", "mask_p", "out_h", "out_p"])
def test_each_output_alone(jsg, torch_cuda, only):
    T, K, W = 67, 129, (3, 5)
    got = run(jsg, torch_cuda, hr.make_input(T, K), W, want=tuple(i == only for i in range(4)))
    assert [g is not None for g in got] == [i == only for i in range(4)]
    assert same(got[only], mirror(T, K, *W)[only])


def test_rows_together_equal_rows_alone(jsg, torch_cuda):
    T, K, W = 70, 65, (63, 63)
    X = np.stack([hr.make_input(T, K, seed=s) for s in (0, 1, 2)])
    together = run(jsg, torch_cuda, X, W, chunk_frames=50)
    for r in range(3):
        alone = run(jsg, torch_cuda, X[r], W)
        check_all([t[r] for t in together], alone)
    check_all([t[0] for t in together], mirror(T, K, *W))


@pytest.mark.parametrize("real", [False, True], ids=["complex", "power"])
def test_pitched_buffers(jsg, torch_cuda, real):
    """Pitched input, output and mask buffers give the dense bits; the sentinel-filled padding is untouched."""
    torch = torch_cuda
    T, K, W, rows = 40, 65, (31, 31), 2
    X = np.stack([hr.make_input(T, K, seed=s) for s in range(rows)])
    X = hr.power(X) if real else X
    dense = run(jsg, torch, X, W)
    dt = torch.float32 if real else torch.complex64

    def pitched(dtype, pitch, extra):
        return torch.full((rows, T + extra, pitch), float(SENTINEL), dtype=dtype, device="cuda")

    b_in, b_oh, b_op, b_mh, b_mp = pitched(dt, 72, 1), pitched(dt, 80, 2), pitched(dt, 80, 2), pitched(torch.float32, 67, 3), pitched(torch.float32, 67, 3)
    b_in[:, :T, :K] = torch.from_numpy(np.array(X)).cuda()
    view = lambda b: b[:, :T, :K]
    jsg.hpss_launch(view(b_in), d_harm=view(b_oh), d_perc=view(b_op), d_mask_h=view(b_mh), d_mask_p=view(b_mp), kernel_size=W)
    torch.cuda.synchronize()
    check_all([view(b).cpu().numpy() for b in (b_mh, b_mp, b_oh, b_op)], dense)
    for b in (b_oh, b_op, b_mh, b_mp):
        pad = b.clone()
        pad[:, :T, :K] = float(SENTINEL)
        assert same(pad.cpu().numpy(), np.full(tuple(b.shape), SENTINEL, dtype=pad.cpu().numpy().dtype))


@pytest.mark.parametrize("chunk", [0, 64])
@pytest.mark.parametrize("kind", ["nan", "inf", "negative"])
def test_containment(jsg, torch_cuda, kind, chunk):
    """A NaN, an Inf or (real input) a -1 at (40, 77) may change only column 77 in frames 25..55 and frame 40 in bins 73..81: every
    other output equals the restatement of the same input, frames 56..63 of the same chunk included."""
    T, K, W = 120, 130, (31, 9)
    X = np.array(hr.make_input(T, K))
    if kind == "negative":
        X = hr.power(X)
        X[40, 77] = -1.0
    else:
        X[40, 77] = complex(np.nan, 1.0) if kind == "nan" else complex(1.0, -np.inf)
    clean = np.ones((T, K), bool)
    clean[25:56, 77] = False
    clean[40, 73:82] = False
    got, want = run(jsg, torch_cuda, X, W, chunk_frames=chunk), hr.mirror(X, *W)[:4]
    check_all(got, want, clean)
    assert same(got[0][56:64, 77], want[0][56:64, 77]) and np.isfinite(want[0][clean]).all()
    if kind != "negative":      # and the real power plane with the same fault
        P = hr.power(X)
        check_all(run(jsg, torch_cuda, P, W, chunk_frames=chunk), hr.mirror(P, *W)[:4], clean)


def test_graph_capture(jsg, torch_cuda):
    """A captured graph on one stream that holds the launch, replayed twice, equals eager."""
    torch = torch_cuda
    T, K, W = 96, 257, (31, 31)
    d_X = torch.from_numpy(np.array(hr.make_input(T, K))).cuda()[None]
    oh, op = (torch.zeros(d_X.shape, dtype=torch.complex64, device="cuda") for _ in range(2))
    mh, mp = (torch.zeros(d_X.shape, dtype=torch.float32, device="cuda") for _ in range(2))
    scratch = torch.empty(jsg.hpss_scratch_bytes(d_X, d_harm=oh, d_perc=op, d_mask_h=mh, d_mask_p=mp) // 4 + 4, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):      # warm-up outside capture
        jsg.hpss_launch(d_X, d_harm=oh, d_perc=op, d_mask_h=mh, d_mask_p=mp, d_scratch=scratch, stream=s.cuda_stream)
    s.synchronize()
    with torch.cuda.graph(graph, stream=s):
        jsg.hpss_launch(d_X, d_harm=oh, d_perc=op, d_mask_h=mh, d_mask_p=mp, d_scratch=scratch, stream=s.cuda_stream)
    for _ in range(2):
        for t in (oh, op, mh, mp, scratch):
            t.zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        check_all([t[0].cpu().numpy() for t in (mh, mp, oh, op)], mirror(T, K, *W))


def test_python_hpss_batch_and_masks(jsg, torch_cuda):
    torch = torch_cuda
    T, K = 67, 129
    X = np.stack([hr.make_input(T, K, seed=s) for s in (0, 1)])                        # [2][T][K]
    d_X = torch.from_numpy(X).cuda().transpose(1, 2)                                    # [2][bins][frames], as stft returns
    H, P = jsg.hpss(d_X, (3, 5))
    M_h, M_p = jsg.hpss(d_X, (3, 5), (1.0, 3.5), masks=True)
    assert H.shape == P.shape == M_h.shape == d_X.shape and H.dtype == torch.complex64 and M_h.dtype == torch.float32
    for i in range(2):
        Hi, Pi = jsg.hpss(d_X[i], (3, 5))
        assert Hi.shape == d_X[i].shape and torch.equal(torch.view_as_real(Hi.contiguous()), torch.view_as_real(H[i].contiguous()))
        assert torch.equal(torch.view_as_real(Pi.contiguous()), torch.view_as_real(P[i].contiguous()))
        want = hr.mirror(X[i], 3, 5, 1.0, 3.5)
        assert same(M_h[i].cpu().numpy().T, want[0]) and same(M_p[i].cpu().numpy().T, want[1])
        want = hr.mirror(X[i], 3, 5)
        assert same(H[i].cpu().numpy().T, want[2]) and same(P[i].cpu().numpy().T, want[3])
    # a float32 power tensor of the same shape: real parts
    Hr, Pr = jsg.hpss(torch.from_numpy(hr.power(X)).cuda().transpose(1, 2), (3, 5))
    want = hr.mirror(hr.power(X[1]), 3, 5)
    assert Hr.dtype == torch.float32 and same(Hr[1].cpu().numpy().T, want[2]) and same(Pr[1].cpu().numpy().T, want[3])


def audio(torch, L=6000, seed=5):
    rng = np.random.default_rng(seed)
    s = np.arange(L)
    x = 0.2 * rng.standard_normal(L) + np.sin(2 * np.pi * 0.031 * s) + 2.0 * (s % 1500 == 700)
    return torch.from_numpy(x.astype(np.float32)).cuda()


def test_hpss_audio_is_its_composition(jsg, torch_cuda):
    torch = torch_cuda
    x = torch.stack([audio(torch), audio(torch, seed=6)])
    n_fft, hop = 512, 128
    y_h, y_p = jsg.hpss_audio(x, n_fft, hop, kernel_size=(17, 9), margin=(1.0, 2.0))
    assert y_h.shape == y_p.shape == x.shape and y_h.dtype == torch.float32
    X = jsg.stft(x, n_fft, hop, None, jsg.capi.WIN_HANN)
    H, P = jsg.hpss(X, (17, 9), (1.0, 2.0))
    for y, Y in ((y_h, H), (y_p, P)):
        assert torch.equal(y.view(torch.int32), jsg.istft(Y, n_fft, hop, None, jsg.capi.WIN_HANN, length=x.shape[-1]).view(torch.int32))


def test_round_trip_of_the_two_parts(jsg, torch_cuda):
    """With margins 1 the masks sum to one, so y_h + y_p returns the input: e = max |y_h + y_p - y_id| against e_id = max |y_id - x|,
    the library's own round trip at the same settings, over the span where the envelope is full.  Bound: e <= 4 e_id (a per-bin
    relative perturbation of about 3u before the inverse FFT should land near the FFT's own round-off)."""
    torch = torch_cuda
    x = audio(torch, 16000)
    n_fft, hop = 1024, 256
    y_h, y_p = jsg.hpss_audio(x, n_fft, hop)
    y_id = jsg.istft(jsg.stft(x, n_fft, hop, None, jsg.capi.WIN_HANN), n_fft, hop, None, jsg.capi.WIN_HANN, length=x.shape[-1])
    span = slice(n_fft, x.shape[-1] - n_fft)
    e = float((y_h.double() + y_p.double() - y_id.double())[span].abs().max())
    e_id = float((y_id.double() - x.double())[span].abs().max())
    print(f"round trip: e = max|y_h + y_p - y_id| = {e:.3e}, e_id = max|y_id - x| = {e_id:.3e}, e / e_id = {e / e_id:.3f}")
    assert e_id > 0 and e <= 4 * e_id
