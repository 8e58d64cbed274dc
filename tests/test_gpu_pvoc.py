"""Phase vocoder on the GPU (include/jsg.h section 2e): accuracy against the float64 reference of tests/pvoc_ref.py under both bounds,
the identity at rate 1, bit-identical results across chunk lengths, rows, pitches and repeats, NaN containment, graph capture, and
the Python layer (phase_vocoder, time_stretch)."""
import numpy as np
import pytest

import pvoc_ref as pr

pytestmark = pytest.mark.gpu

POISON = complex(np.float32(-7.25e11), np.float32(3.5e-9))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    torch.cuda.set_device(0)
    return torch


def bits(torch, t):
    return torch.view_as_real(t.contiguous()).view(torch.int32)


def same_bits(torch, a, b):
    return a.shape == b.shape and torch.equal(bits(torch, a), bits(torch, b))


def run(jsg, torch, X, rate, hop, n, **kw):
    """X: numpy [T][K] or [rows][T][K], or a CUDA tensor -> the CUDA result [rows][T_out][K] of one launch into a dense buffer."""
    d_X = X if hasattr(X, "is_cuda") else torch.from_numpy(np.array(X)).cuda()     # a copy: the shared inputs are read-only
    if d_X.dim() == 2:
        d_X = d_X[None]
    out = torch.full((d_X.shape[0], jsg.pvoc_frames(d_X.shape[1], rate), n // 2 + 1), POISON, dtype=torch.complex64, device="cuda")
    jsg.phase_vocoder_launch(d_X, rate, hop, n, out, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", pr.accuracy_cases(), ids=pr.case_id)
def test_accuracy_against_float64(jsg, torch_cuda, case):
    """Per element |Y - R| <= B max(|R|, 2^-100) with (a) B = pr.YARDSTICKS x the float32 restatement's own worst relative error on the case and
    (b) the analytic cap 2^-20 + (i+1) 3 2^-20 of output frame i; exactly 0+0j where both interpolated magnitudes are zero."""
    n, hop, rate, T = case
    X = pr.make_input(n, hop, T)
    Y = run(jsg, torch_cuda, X, rate, hop, n)[0].cpu().numpy()
    assert Y.shape == (pr.n_frames_out(T, rate), n // 2 + 1)
    f = pr.accuracy_figures(X, Y, rate, hop, n)
    print(f"{pr.case_id(case)}: yardstick {f['yardstick']:.3e}, GPU worst {f['worst']:.3e}, GPU / yardstick {f['worst'] / f['yardstick']:.3f}, "
          f"worst ratio to the cap {f['cap_ratio']:.4f}, {f['n_zero']} zero elements exact: {f['zeros_exact']}")
    assert f["worst"] <= pr.YARDSTICKS * f["yardstick"]
    assert f["cap_ratio"] <= 1.0
    assert f["n_zero"] > 0 and f["zeros_exact"]


@pytest.mark.parametrize("n,hop", [(512, 128), (2048, 100)])
def test_rate_one_is_the_identity(jsg, torch_cuda, n, hop):
    X = pr.make_input(n, hop, 2000)
    Y = run(jsg, torch_cuda, X, 1.0, hop, n)[0].cpu().numpy()
    assert Y.shape == X.shape
    assert (pr.rel_error(Y, X.astype(np.complex128)) <= pr.bound_cap(2000)[:, None]).all()
    assert (Y[X == 0] == 0).all()


@pytest.mark.parametrize("rate", [0.8, 1.0, 1.3, 2.0])
def test_same_bits_for_every_chunk_length_and_on_repeat(jsg, torch_cuda, rate):
    torch = torch_cuda
    n, hop = 512, 100
    X = pr.make_input(n, hop, pr.frames_for(rate, 700))
    base = run(jsg, torch, X, rate, hop, n)
    assert not (base == POISON).any()
    for chunk in (1, 7, 64, 0):
        assert same_bits(torch, run(jsg, torch, X, rate, hop, n, chunk_frames=chunk), base), chunk
    # one buffer of the exact size for a chunk length of 64, reused
    a = jsg.spectrogram._pvoc_args(torch.from_numpy(np.array(X)).cuda(), rate, hop, n, base, 64)
    import ctypes as C
    sc = torch.empty(jsg.capi.lib().jsg_pvoc_scratch_bytes(C.byref(a)) // 4, dtype=torch.int32, device="cuda")
    for _ in range(2):
        sc.fill_(-1)
        assert same_bits(torch, run(jsg, torch, X, rate, hop, n, chunk_frames=64, d_scratch=sc), base)


def test_rows_together_equal_rows_alone(jsg, torch_cuda):
    torch = torch_cuda
    n, hop, rate, T = 2048, 512, 1 / 0.9, 333
    X = np.stack([pr.make_input(n, hop, T, seed=s) for s in (0, 1, 2)])
    together = run(jsg, torch, X, rate, hop, n, chunk_frames=50)
    for r in range(3):
        assert same_bits(torch, together[r], run(jsg, torch, X[r], rate, hop, n)[0]), r


@pytest.mark.parametrize("rate", [0.8, 1.3])
def test_pitched_buffers_equal_dense_and_padding_is_untouched(jsg, torch_cuda, rate):
    torch = torch_cuda
    n, hop, T, rows = 512, 128, 150, 3
    K = n // 2 + 1
    X = np.stack([pr.make_input(n, hop, T, seed=s) for s in range(rows)])
    dense = run(jsg, torch, X, rate, hop, n)
    T_out = dense.shape[1]
    big_in = torch.full((rows, T + 2, K + 7), POISON, dtype=torch.complex64, device="cuda")
    big_in[:, :T, :K] = torch.from_numpy(X).cuda()
    big_out = torch.full((rows, T_out + 3, K + 5), POISON, dtype=torch.complex64, device="cuda")
    jsg.phase_vocoder_launch(big_in[:, :T, :K], rate, hop, n, big_out[:, :T_out, :K], chunk_frames=33)
    torch.cuda.synchronize()
    assert same_bits(torch, big_out[:, :T_out, :K], dense)
    mask = torch.ones(big_out.shape, dtype=torch.bool, device="cuda")
    mask[:, :T_out, :K] = False
    untouched = torch.full_like(big_out, POISON)
    assert torch.equal(bits(torch, big_out)[mask], bits(torch, untouched)[mask])


@pytest.mark.parametrize("rate", [0.8, 1.0, 2.0])
def test_nan_stays_in_its_bin_and_after_its_frame(jsg, torch_cuda, rate):
    torch = torch_cuda
    n, hop, T, j_nan, k_nan = 512, 128, 240, 101, 77
    X = pr.make_input(n, hop, T)
    clean = run(jsg, torch, X, rate, hop, n, chunk_frames=16)
    Xn = X.copy()
    Xn[j_nan, k_nan] = complex(np.nan, 1.0)
    dirty = run(jsg, torch, Xn, rate, hop, n, chunk_frames=16)
    others = [k for k in range(n // 2 + 1) if k != k_nan]
    assert same_bits(torch, dirty[:, :, others], clean[:, :, others])
    t = np.arange(clean.shape[1], dtype=np.float64) * rate
    before = torch.from_numpy(np.floor(t) + 1 < j_nan).cuda()
    assert before.any() and not before.all()
    assert same_bits(torch, dirty[0, before][:, k_nan], clean[0, before][:, k_nan])
    reads = torch.from_numpy((np.floor(t) == j_nan) | (np.floor(t) + 1 == j_nan)).cuda()
    assert reads.any() and torch.isnan(torch.view_as_real(dirty[0, reads][:, k_nan])).any(dim=-1).all()


def test_graph_capture_matches_eager(jsg, torch_cuda):
    torch = torch_cuda
    n, hop, rate, T, rows = 2048, 100, 0.8, 120, 2
    K = n // 2 + 1
    d_X = torch.zeros((rows, T, K), dtype=torch.complex64, device="cuda")
    out = torch.zeros((rows, jsg.pvoc_frames(T, rate), K), dtype=torch.complex64, device="cuda")
    sc = torch.empty(rows * out.shape[1] * K, dtype=torch.int32, device="cuda")     # enough for any chunk length
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        jsg.phase_vocoder_launch(d_X, rate, hop, n, out, chunk_frames=16, d_scratch=sc, stream=s.cuda_stream)     # warm-up outside capture
    s.synchronize()
    with torch.cuda.graph(g, stream=s):
        jsg.phase_vocoder_launch(d_X, rate, hop, n, out, chunk_frames=16, d_scratch=sc, stream=s.cuda_stream)
    for seed in (1, 2):
        d_X.copy_(torch.from_numpy(np.stack([pr.make_input(n, hop, T, seed=seed + r) for r in range(rows)])))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(torch, out, run(jsg, torch, d_X, rate, hop, n))


def test_python_phase_vocoder_on_a_batch(jsg, torch_cuda):
    torch = torch_cuda
    n, hop, rate, T = 512, 128, 1.3, 90
    K = n // 2 + 1
    X = np.stack([pr.make_input(n, hop, T, seed=s) for s in range(6)]).reshape(2, 3, T, K)
    d_X = torch.from_numpy(X).cuda().transpose(-1, -2)                      # torchaudio's layout [..., bins, frames]
    Y = jsg.phase_vocoder(d_X, rate, hop)
    torch.cuda.synchronize()
    assert Y.shape == (2, 3, K, pr.n_frames_out(T, rate)) and Y.dtype == torch.complex64
    assert Y.transpose(-1, -2).is_contiguous()                              # the transposed view of the frame-major buffer
    for a in range(2):
        for b in range(3):
            assert same_bits(torch, Y[a, b].transpose(0, 1), run(jsg, torch, X[a, b], rate, hop, n)[0]), (a, b)
    assert same_bits(torch, jsg.phase_vocoder(d_X, rate, hop, n_fft=n), Y)
    with pytest.raises(jsg.JsgError):
        jsg.phase_vocoder(d_X, rate, hop, n_fft=1024)


@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_time_stretch_is_its_composition_and_keeps_the_pitch(jsg, torch_cuda, rate):
    torch = torch_cuda
    fs, f0, L, N = 16000.0, 440.0, 32000, 8192
    x = torch.from_numpy(np.sin(2 * np.pi * f0 * np.arange(L) / fs).astype(np.float32)).cuda()
    y = jsg.time_stretch(x, rate)
    assert y.shape == (int(round(L / rate)),) and y.dtype == torch.float32
    n_fft, hop = 2048, 512
    hann = jsg.capi.WIN_HANN
    want = jsg.istft(jsg.phase_vocoder(jsg.stft(x, n_fft, hop, None, hann, True), rate, hop, n_fft), n_fft, hop, None, hann, True,
                     length=int(round(L / rate)))
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
    assert jsg.time_stretch(x, rate, length=12345).shape == (12345,)
    assert jsg.time_stretch(x[None].repeat(2, 1), rate, n_fft=1024, hop_length=100).shape == (2, int(round(L / rate)))
    w = np.hanning(N)

    def peak(v):
        v = np.asarray(v, np.float64)
        mid = v[(v.size - N) // 2:(v.size - N) // 2 + N]
        return int(np.argmax(np.abs(np.fft.rfft(mid * w))))

    assert peak(y.cpu().numpy()) == peak(x.cpu().numpy()) == int(round(f0 * N / fs))
